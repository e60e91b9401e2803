"""What agents missing anywhere cost ("Agents missing anywhere").

Times, in ONE process and in alternation, the replayed eval forward of one MultiScaleHGNN block on one stream; every
scene holds the same number of valid agents on every side (about 80 % of N):
  prefix       `GraphedMultiScale(ragged=True)`, the counts set once: the ragged replay without the subset route;
  subset       `GraphedMultiScale(ragged="subset")` with the same counts as a prefix mask, set once;
  holes        the same graph with random holes of the same counts, set once;
  holes-reset  the same, the mask set before every replay (`g(agent_mask=m)`): one subset launch more.
Protocol of tools/ragged_replay_time.py: device Philox noise, device events around 10 forwards, 40 alternations after 10
warm-up forwards of each side; median (min-max) per forward in ms, and the library launches of one forward.  The last
line per shape is the bytes one compaction and one expansion launch move (read + written), for the achieved bandwidth
of remap_rows_kernel from a kernel trace of this tool.

    python tools/agent_subset_time.py                  # both shapes of the table
    python tools/agent_subset_time.py 512 11 2,5,11 fp32
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # repo root
import groupnet_amd as G  # noqa: E402
from groupnet_amd import ops  # noqa: E402
from groupnet_amd.graphs import GraphedMultiScale  # noqa: E402
from groupnet_amd.multiscale import MultiScaleHGNN  # noqa: E402

SHAPES = [(1024, 50, [2, 4, 8, 16], "bf16"), (512, 11, [2, 5, 11], "fp32")]
INNER, ROUNDS, WARM, SEED = 10, 40, 10, 7


def launches_of(fn) -> int:
    """Library launches issued by one call of fn (every launcher asks `ops.stream_handle` once)."""
    seen, real = [], ops.stream_handle
    ops.stream_handle = lambda: seen.append(1) or real()
    try:
        with torch.no_grad():
            fn()
    finally:
        ops.stream_handle = real
    return len(seen)


def remap_bytes(B, N, scales, es):
    """(compaction, expansion) bytes read + written by the two remap launches of one device-noise forward: a
    destination position is always written; a source row is read where the position is mapped (counted in full: an
    upper bound by the share of invalid agents)."""
    S = len(scales)
    compaction = 2 * B * N * 64 * es
    final = B * N * 64 * (2 + S) * es
    new_H = sum(B * (1 if s == N else N) * N * es for s in scales)
    return compaction, 2 * (final + new_H)


def measure(B, N, scales, storage, dev):
    dtype = torch.bfloat16 if storage == "bf16" else torch.float32
    torch.manual_seed(0)
    blk = MultiScaleHGNN(scales).to(dev).eval()
    f = torch.randn(B, N, 64, device=dev).to(dtype)
    n = max(1, round(0.8 * N))
    counts = [n] * B
    prefix = (torch.arange(N)[None] < torch.tensor(counts)[:, None]).to(torch.uint8).to(dev)
    gen = torch.Generator().manual_seed(SEED)
    holes = torch.zeros(B, N, dtype=torch.uint8)
    for b in range(B):
        holes[b, torch.randperm(N, generator=gen)[:n]] = 1
    holes = holes.to(dev)
    g_prefix = GraphedMultiScale(blk, B, N, seed=SEED, dtype=dtype, ragged=True)
    g_subset = GraphedMultiScale(blk, B, N, seed=SEED, dtype=dtype, ragged="subset")
    g_holes = GraphedMultiScale(blk, B, N, seed=SEED, dtype=dtype, ragged="subset")
    g_prefix(f, n_agents=counts)
    g_subset(f, agent_mask=prefix)
    g_holes(f, agent_mask=holes)
    sides = {"prefix": lambda: g_prefix(), "subset": lambda: g_subset(), "holes": lambda: g_holes(),
             "holes-reset": lambda: g_holes(agent_mask=holes)}
    G.set_noise_mode("device", seed=SEED, offset=0)
    try:
        n_launch = {"prefix": launches_of(g_prefix._step), "subset": launches_of(g_subset._step)}
        n_launch["holes"] = n_launch["subset"]
        n_launch["holes-reset"] = n_launch["subset"] + launches_of(lambda: g_holes.counts.set_from_mask(holes))
        G.set_noise_mode("device", seed=SEED, offset=0)         # (_step left the graphs' counter mode behind)
        times = {k: [] for k in sides}
        with torch.no_grad():
            for fn in sides.values():
                for _ in range(WARM):
                    fn()
            torch.cuda.synchronize()
            for _ in range(ROUNDS):
                for name, fn in sides.items():
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(INNER):
                        fn()
                    t1.record()
                    t1.synchronize()
                    times[name].append(t0.elapsed_time(t1) / INNER)
    finally:
        G.set_noise_mode("host", seed=0, offset=0)
    return {k: dict(median=statistics.median(v), min=min(v), max=max(v), launches=n_launch[k]) for k, v in times.items()}


def main(argv):
    dev = torch.device("cuda:0")
    shapes = [(int(argv[0]), int(argv[1]), [int(s) for s in argv[2].split(",")], argv[3])] if len(argv) == 4 else SHAPES
    cell = lambda r: f"{r['median']:.3f} ms ({r['min']:.3f}–{r['max']:.3f}), {r['launches']} launches"
    rows = []
    for B, N, scales, storage in shapes:
        res = measure(B, N, scales, storage, dev)
        moved = remap_bytes(B, N, scales, 2 if storage == "bf16" else 4)
        print(json.dumps(dict(B=B, N=N, scales=scales, storage=storage, per_forward_ms=res, compaction_bytes=moved[0],
                              expansion_bytes=moved[1])))
        rows.append(f"| B = {B}, N = {N}, scales {{{', '.join(map(str, scales))}}}, {storage} storage | {cell(res['prefix'])} | "
                    f"{cell(res['subset'])} | {cell(res['holes'])} | {cell(res['holes-reset'])} |")
    print("| shape | prefix ragged replay | subset replay, the same counts as a prefix mask | subset replay, random holes | "
          "subset replay, the mask set every time |\n|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main(sys.argv[1:])
