"""What a ragged batch costs eagerly and replayed ("Ragged batches from a captured graph").

Times, in ONE process and in alternation, the eval forward of one MultiScaleHGNN block on one stream, every count N - 1:
  eager    the eager ragged forward, `block(f, n_agents=held)`, the holder made once outside the timed region;
  replay   `GraphedMultiScale(ragged=True)`, the counts set once;
  reset    the same graph, the counts set again before every replay (`g(n_agents=counts)`);
  full     the full-batch capture `GraphedMultiScale()`: no counts, the fused forms.
Protocol of the ragged table of DESIGN.md §7: device Philox noise, device events around 10 forwards, 40 alternations
after 10 warm-up forwards of each side; median (min-max) per forward in ms, and the library launches of one forward.

    python tools/ragged_replay_time.py                  # both shapes of the table
    python tools/ragged_replay_time.py 512 11 2,5,11 fp32
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


def measure(B, N, scales, storage, dev):
    dtype = torch.bfloat16 if storage == "bf16" else torch.float32
    torch.manual_seed(0)
    blk = MultiScaleHGNN(scales).to(dev).eval()
    f = torch.randn(B, N, 64, device=dev).to(dtype)
    counts = [N - 1] * B
    held = ops.agent_counts(counts, B, N, dev)
    g_ragged = GraphedMultiScale(blk, B, N, seed=SEED, dtype=dtype, ragged=True)
    g_full = GraphedMultiScale(blk, B, N, seed=SEED, dtype=dtype)
    g_ragged(f, n_agents=counts)
    g_full(f)

    def eager():
        blk(f, n_agents=held)

    sides = {"eager": eager, "replay": lambda: g_ragged(), "reset": lambda: g_ragged(n_agents=counts),
             "full": lambda: g_full()}
    G.set_noise_mode("device", seed=SEED, offset=0)
    try:
        n_launch = {"eager": launches_of(eager), "replay": launches_of(g_ragged._step), "full": launches_of(g_full._step)}
        n_launch["reset"] = n_launch["replay"]
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
        print(json.dumps(dict(B=B, N=N, scales=scales, storage=storage, per_forward_ms=res)))
        rows.append(f"| B = {B}, N = {N}, scales {{{', '.join(map(str, scales))}}}, {storage} storage | {cell(res['eager'])} | "
                    f"{cell(res['replay'])} | {cell(res['reset'])} | {cell(res['full'])} |")
    print("| shape | eager ragged forward | ragged replay, counts set once | ragged replay, counts set every time | "
          "full-batch replay |\n|---|---|---|---|---|")
    print("\n".join(rows))


if __name__ == "__main__":
    main(sys.argv[1:])
