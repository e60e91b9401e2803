"""Test helper: the cases, inputs and per-scene oracle of the ragged-batch tests (tests/test_ragged_cpu.py checks the
cases and the oracle's plumbing, tests/test_ragged_gpu.py runs them).  Pure torch on the CPU; the library is never loaded.

The contract ("Ragged batches").  `n_agents` gives every scene of a call its own agent count n_b <= N;
the first n_b agent rows are real, the rest is padding.  Every value at a valid position — node rows n < n_b, pairwise
edges (i, j) with i, j < n_b, hyperedge rows e < n_b or the single row of a scale-N module — equals what the module
computes for scene b ALONE as an n_b-agent scene.  So the oracle is the existing CPU oracle run on h[b:b+1, :n_b]:
  * pairwise: `ms_hgnn_pairwise_forward`, the scene's noise gathered at the padded indices i*N + j, i, j < n_b;
  * hyper: `_message_passing` on the incidence of the contract: scale < N — zeros(1, n_b, n_b).scatter(2,
    corr.topk(min(s, n_b)).indices, 1); scale == N (the padded size) — ones(1, 1, n_b).
The incidence is ranked on the fp32 affinity of the scene's own rows (of their bf16 roundings for bf16 storage); the
cases' seeds keep every k-th / (k+1)-th affinity gap of a valid row at 2e-5 or more — ten times the affinity gate of
2e-6 of tests/test_parity_gpu.py — so that no rounding of the affinity can change a selection (asserted on the CPU).
"""
from __future__ import annotations

import functools
from typing import Dict, List, Tuple

import torch

from launch_forms import state64
from oracle import ms_hgnn_oracle as O

K_PAIR, K_HYPER = 6, 10
MIN_GAP = 2e-5          # smallest admissible gap between the k-th and (k+1)-th affinity of a valid row
TOL_CORR = 2e-6         # the affinity gate of tests/test_parity_gpu.py
TOL = 1e-5              # the project's absolute gate of fp32 storage (default-init outputs are of order 0.2)


def _case(id, N, counts, scales, seed, what):
    return dict(id=id, N=N, counts=list(counts), B=len(counts), scales=list(scales), seed=seed, what=what)


CASES = [
    _case("n7", 7, [1, 2, 3, 5, 6, 7], [2, 5, 7], 0,
          "fused-gather side; several scenes per workgroup; the n_b = 1 and 2 edges of the max rule"),
    _case("n17", 17, [17, 3, 16, 9, 1], [2, 5, 17], 3, "stand-alone gather side"),
    _case("n50", 50, [50, 23, 5], [2, 4, 8, 16], 5, "fp32 and bf16 storage"),
    _case("n113", 113, [113, 40], [2, 8, 113], 5, "incidence and node->edge only; the banded top-k"),
]
BY_ID = {c["id"]: c for c in CASES}
BLOCK_CASES = [c for c in CASES if c["N"] <= 50]      # the cases that run whole modules


def n_edges(N: int, s: int) -> int:
    return 1 if s == N else N


def noise_shapes(case: Dict) -> List[Tuple[int, int, int]]:
    B, N = case["B"], case["N"]
    return [(B, N * N, K_PAIR)] + [(B, n_edges(N, s), K_HYPER) for s in case["scales"]]


def inputs(case: Dict, nmp: int = 1, bf16: bool = False):
    """(h (B, N, 64) N(0,1), U: per module, pairwise first, its `nmp` uniform tensors of the PADDED shapes).  bf16: h
    rounded to bf16 (as fp32 values)."""
    gen = torch.Generator().manual_seed(1000 + case["seed"])
    h = torch.randn(case["B"], case["N"], 64, generator=gen)
    if bf16:
        h = h.bfloat16().float()
    U = [[torch.rand(shp, generator=gen) for _ in range(nmp)] for shp in noise_shapes(case)]
    return h, U


def with_garbage(case: Dict, h: torch.Tensor, scale: float = 100.0, seed: int = 77) -> torch.Tensor:
    """h with every padded row replaced by finite garbage, N(0,1) x 100."""
    gen = torch.Generator().manual_seed(seed + case["seed"])
    g = torch.randn(h.shape, generator=gen) * scale
    out = h.clone()
    for b, n in enumerate(case["counts"]):
        out[b, n:] = g[b, n:]
    return out


def garbage_corr(case: Dict, corr: torch.Tensor, seed: int = 78) -> torch.Tensor:
    """corr (B, N, N) with every entry that has a padded end replaced by N(0,1) x 100."""
    gen = torch.Generator().manual_seed(seed + case["seed"])
    g = torch.randn(corr.shape, generator=gen) * 100.0
    out = g.clone()
    for b, n in enumerate(case["counts"]):
        out[b, :n, :n] = corr[b, :n, :n]
    return out


def cpu_block(case: Dict, nmp: int = 1):
    """(the case's MultiScaleHGNN on the CPU with its seeded default init, the pairwise state, the hyper states)."""
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(case["seed"])
    blk = MultiScaleHGNN(case["scales"], nmp_layers=nmp)
    sp = {k: v.detach().clone() for k, v in blk.interaction.state_dict().items()}
    shs = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in blk.interaction_hyper]
    return blk, sp, shs


# ---------------------------------------------------------------------------------------------------------------------
# the contract's incidence
# ---------------------------------------------------------------------------------------------------------------------
def scene_corr(h: torch.Tensor, b: int, n: int) -> torch.Tensor:
    """The fp32 affinity (1, n, n) of scene b alone."""
    return O.affinity(h[b:b + 1, :n].float())


def scene_incidence(corr: torch.Tensor, s: int, N: int) -> torch.Tensor:
    """The incidence of a scale-s module (of padded size N) on a scene of n agents with affinity corr (1, n, n):
    (1, 1, n) of ones for s == N, else (1, n, n) with the top-min(s, n) of every row."""
    n = corr.shape[1]
    if s == N:
        return torch.ones(1, 1, n)
    k = min(max(int(s), 1), n)
    return torch.zeros(1, n, n).scatter(2, corr.topk(k, dim=2).indices, 1)


def padded_incidence(case: Dict, h: torch.Tensor, s: int) -> torch.Tensor:
    """(B, E, N): every scene's contract incidence embedded in zeros."""
    N = case["N"]
    out = torch.zeros(case["B"], n_edges(N, s), N)
    for b, n in enumerate(case["counts"]):
        Hb = scene_incidence(scene_corr(h, b, n), s, N)
        out[b, :Hb.shape[1], :n] = Hb[0]
    return out


def padded_corr(case: Dict, h: torch.Tensor) -> torch.Tensor:
    """(B, N, N): every scene's own affinity in its valid block, zeros elsewhere."""
    out = torch.zeros(case["B"], case["N"], case["N"])
    for b, n in enumerate(case["counts"]):
        out[b, :n, :n] = scene_corr(h, b, n)[0]
    return out


def min_gap(case: Dict, h: torch.Tensor) -> float:
    """The smallest gap between the k-th and (k+1)-th affinity over every valid row and top-k scale (k = min(s, n_b) <
    n_b: a row that takes every valid column has no gap to keep)."""
    N, worst = case["N"], float("inf")
    for b, n in enumerate(case["counts"]):
        v = torch.sort(scene_corr(h, b, n), dim=-1, descending=True).values
        for s in case["scales"]:
            k = min(max(s, 1), n)
            if s != N and k < n:
                worst = min(worst, float((v[..., k - 1] - v[..., k]).min()))
    return worst


# ---------------------------------------------------------------------------------------------------------------------
# the per-scene oracle
# ---------------------------------------------------------------------------------------------------------------------
def pair_index(N: int, n: int) -> torch.Tensor:
    """The padded ordered-edge indices i*N + j of the n x n valid pairs, row-major."""
    i = torch.arange(n)
    return (i[:, None] * N + i[None, :]).reshape(-1)


def scene_noise(U_mod: List[torch.Tensor], b: int, N: int, n: int, pairwise: bool) -> List[torch.Tensor]:
    """Scene b's draws of one module at its valid edges: the pairs (i, j < n) at their padded indices, the hyperedge
    rows e < n, or the single row of a scale-N module."""
    out = []
    for u in U_mod:
        ub = u[b:b + 1]
        if pairwise:
            out.append(ub[:, pair_index(N, n)])
        else:
            out.append(ub if ub.shape[1] == 1 else ub[:, :n])
    return out


def scene_oracle(sp, shs, case: Dict, h: torch.Tensor, U, b: int, nmp: int = 1):
    """Scene b alone as an n_b-agent scene, in float64 (the incidence is ranked on the fp32 affinity) -> (node features
    per module (n_b, 64), factors per module, incidences per scale (1, e, n_b))."""
    N, n = case["N"], case["counts"][b]
    hb = h[b:b + 1, :n].double()
    noise = lambda Um, pairwise: [u.double() for u in scene_noise(Um, b, N, n, pairwise)]
    with torch.no_grad():
        nf, fac = O.ms_hgnn_pairwise_forward(state64(sp), hb, noise(U[0], True), nmp, decomposed=True)
        feats, facs, Hs = [nf[0]], [fac[0]], []
        corr = scene_corr(h, b, n)
        for sh, s, Um in zip(shs, case["scales"], U[1:]):
            H = scene_incidence(corr, s, N)
            nf, fac = O._message_passing(state64(sh), hb, H.double(), noise(Um, False), nmp, True, None)
            feats.append(nf[0])
            facs.append(fac[0])
            Hs.append(H)
    return feats, facs, Hs


@functools.lru_cache(maxsize=None)
def block_oracle(case_id: str, nmp: int = 1, bf16: bool = False):
    """The float64 per-scene oracle of every scene of a case, computed once and shared (never written to): a list, per
    scene, of `scene_oracle`'s tuple; with the case's inputs (h, U) and states."""
    case = BY_ID[case_id]
    _, sp, shs = cpu_block(case, nmp)
    h, U = inputs(case, nmp, bf16)
    return h, U, sp, shs, [scene_oracle(sp, shs, case, h, U, b, nmp) for b in range(case["B"])]


def node2edge64(state, hb: torch.Tensor, H: torch.Tensor, slab: int = 2048) -> torch.Tensor:
    """`O.node2edge` of one scene in float64, hyperedges in slabs (they are independent): (E, 64)."""
    s64 = state64(state)
    with torch.no_grad():
        return torch.cat([O.node2edge(s64, hb.double(), H[:, e0:e0 + slab].double(), 0, True)[0][0]
                          for e0 in range(0, H.shape[1], slab)])
