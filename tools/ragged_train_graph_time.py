"""What a ragged training step costs eagerly and replayed ("Ragged training from a captured graph").

Times, in ONE process and in alternating windows, one training step (forward, MSE loss over the valid rows, backward, SGD;
device Philox noise) of one MultiScaleHGNN block with scales {2, 5, 11} at B = 512, N = 11, counts uniform in 1..11:
  eager_ragged   the eager ragged step behind `set_ragged_training(True)`: `block(f, n_agents=held)`, the holder made once;
  graph_full     `GraphedTrainStep()` on the full batch (no counts);
  graph_ragged   `GraphedTrainStep(ragged=True)`, the counts set once;
  graph_reset    the same graph, the counts set again before every replay;
  graph_det      `GraphedTrainStep(ragged=True)` captured with `set_deterministic(True)`.
Protocol of DESIGN.md §4 "Ragged training": host clock around a synchronise, WINDOWS alternating windows of STEPS steps
after a warm-up window of each side; median (min-max) per step in ms, and the figures per REAL agent.

    python tools/ragged_train_graph_time.py
"""
import copy
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # repo root
import groupnet_amd as G  # noqa: E402
from groupnet_amd import ops  # noqa: E402
from groupnet_amd.graphs import GraphedTrainStep  # noqa: E402
from groupnet_amd.multiscale import MultiScaleHGNN  # noqa: E402

B, N, SCALES, SEED = 512, 11, [2, 5, 11], 7
WINDOWS, STEPS, LR = 7, 100, 1e-3


def masked_mse(out, H, target, valid=None):
    if valid is None:
        return ((out - target) ** 2).mean()
    d = torch.where(valid[..., None], out - target, torch.zeros((), device=out.device))
    return (d * d).sum() / (valid.sum().clamp(min=1) * d.shape[-1])


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    base = MultiScaleHGNN(SCALES).to(dev).train()
    f = torch.randn(B, N, 64, device=dev)
    tgt = torch.randn(B, N, base.out_features, device=dev)
    counts = torch.randint(1, N + 1, (B,), generator=torch.Generator().manual_seed(1)).tolist()
    valid = (torch.arange(N)[None, :] < torch.tensor(counts)[:, None]).to(dev)
    real = sum(counts)

    def graphed(ragged, det=False):
        blk = copy.deepcopy(base)
        G.set_deterministic(True if det else None)
        try:
            step = GraphedTrainStep(blk, torch.optim.SGD(blk.parameters(), lr=LR), masked_mse, B, N, [tuple(tgt.shape)],
                                    seed=SEED, ragged=ragged)
        finally:
            G.set_deterministic(None)
        step(f, tgt, **(dict(n_agents=counts) if ragged else {}))
        return step

    g_full, g_ragged, g_det = graphed(False), graphed(True), graphed(True, det=True)
    e_blk = copy.deepcopy(base)
    e_opt = torch.optim.SGD(e_blk.parameters(), lr=LR)
    held = ops.agent_counts(counts, B, N, dev)

    def eager_ragged():
        G.set_ragged_training(True)
        G.set_noise_mode("device", seed=SEED, offset=0)
        try:
            e_opt.zero_grad(set_to_none=True)
            out, H = e_blk(f, n_agents=held)
            masked_mse(out, H, tgt, valid).backward()
            e_opt.step()
        finally:
            G.set_noise_mode("host", seed=0, offset=0)
            G.set_ragged_training(None)

    sides = {"eager_ragged": eager_ragged, "graph_full": lambda: g_full(), "graph_ragged": lambda: g_ragged(),
             "graph_reset": lambda: g_ragged(n_agents=counts), "graph_det": lambda: g_det()}

    def window(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    for fn in sides.values():
        window(fn, STEPS // 4)
    times = {k: [] for k in sides}
    for _ in range(WINDOWS):
        for name, fn in sides.items():
            times[name].append(window(fn, STEPS))
    res = {k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()}
    agents = {k: (B * N if k == "graph_full" else real) for k in sides}
    print(json.dumps(dict(B=B, N=N, scales=SCALES, mean_count=real / B, windows=WINDOWS, steps=STEPS, per_step_ms=res,
                          ns_per_real_agent={k: res[k]["median"] * 1e6 / agents[k] for k in sides})))
    print("| side | ms per step, median (min–max) | ns per real agent |\n|---|---|---|")
    for k, r in res.items():
        print(f"| {k} | {r['median']:.3f} ({r['min']:.3f}–{r['max']:.3f}) | {r['median'] * 1e6 / agents[k]:.0f} |")


if __name__ == "__main__":
    main()
