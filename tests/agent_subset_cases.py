"""Test helper: the rule, the cases and the torch-indexing references of the subset tests ("Agents missing
anywhere"; tests/test_agent_subset_cpu.py checks them, tests/test_agent_subset_gpu.py runs them).  numpy and torch on
the CPU; the library is never loaded.

The rule.  Scene b has a validity row over its N agent slots (non-zero byte = valid); V_b = its valid slots in increasing
order, n_b = |V_b|.  `subset_rule` states n_valid, order and slot in numpy.  The contract of a forward with
``n_agents=ops.agent_subset(mask)``: at valid positions what the existing ragged forward (``n_agents=n_valid``) returns
for the COMPACTED batch — valid rows first, in order, zeros behind them — moved back to the original slots, zeros at every
other position.  `compact_*` / `expand_*` state the two moves with torch indexing.

A case is a `ragged_cases` case whose counts are the mask's n_valid — so `ragged_cases.min_gap`, `scene_oracle` and the
rest read the compacted batch as the ragged batch it is — plus the mask.  The seeds keep every top-k selection of the
compacted scenes `ragged_cases.MIN_GAP` apart (asserted on the CPU).
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np
import torch

import ragged_cases as C

EMPTY = 2          # GN_COUNTS_EMPTY


def subset_rule(valid) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """(n_valid (B,), order (B,N), slot (B,N), status) of a (B,N) mask, all int32: order[b,r] = the slot of the r-th valid
    agent (r < n_b), -1 behind; slot[b,n] = the rank of slot n among the valid ones, -1 where invalid; status = EMPTY
    where some scene has no valid agent, else 0."""
    v = np.asarray(valid) != 0
    B, N = v.shape
    n_valid = v.sum(axis=1).astype(np.int32)
    order = np.full((B, N), -1, dtype=np.int32)
    slot = np.full((B, N), -1, dtype=np.int32)
    for b in range(B):
        r = 0
        for n in range(N):
            if v[b, n]:
                order[b, r], slot[b, n] = n, r
                r += 1
    return n_valid, order, slot, (EMPTY if (n_valid == 0).any() else 0)


# ---------------------------------------------------------------------------------------------------------------------
# the two moves, by torch indexing
# ---------------------------------------------------------------------------------------------------------------------
def _valid_slots(mask: torch.Tensor, b: int) -> torch.Tensor:
    return torch.nonzero(mask[b] != 0).reshape(-1)


def compact_nodes(x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """(B,N,w): scene b's valid rows first, in order, zeros behind them."""
    out = torch.zeros_like(x)
    for b in range(x.shape[0]):
        V = _valid_slots(mask, b)
        out[b, :len(V)] = x[b, V]
    return out


def expand_nodes(xc: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """(B,N,w): compacted row r back at the slot of the r-th valid agent, zeros at invalid slots."""
    out = torch.zeros_like(xc)
    for b in range(xc.shape[0]):
        V = _valid_slots(mask, b)
        out[b, V] = xc[b, :len(V)]
    return out


def compact_matrix(x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """(B,N,N,...): the valid block x[b][V][:, V] in the leading corner, zeros elsewhere."""
    out = torch.zeros_like(x)
    for b in range(x.shape[0]):
        V = _valid_slots(mask, b)
        out[b, :len(V), :len(V)] = x[b][V][:, V]
    return out


def expand_matrix(xc: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    out = torch.zeros_like(xc)
    for b in range(xc.shape[0]):
        V = _valid_slots(mask, b)
        out[b][V[:, None], V[None, :]] = xc[b, :len(V), :len(V)]
    return out


def compact_pairs(x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """(B,N*N,w) ordered pair rows i*N + j."""
    B, NN, w = x.shape
    N = mask.shape[1]
    return compact_matrix(x.reshape(B, N, N, w), mask).reshape(B, NN, w)


def expand_pairs(xc: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    B, NN, w = xc.shape
    N = mask.shape[1]
    return expand_matrix(xc.reshape(B, N, N, w), mask).reshape(B, NN, w)


def compact_edges(x: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """(B,E,w) rows of a hyper module: node-like for a top-k module (E = N), the single row of a scale-N module stays."""
    return x.clone() if x.shape[1] == 1 and mask.shape[1] != 1 else compact_nodes(x, mask)


def expand_edges(xc: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    return xc.clone() if xc.shape[1] == 1 and mask.shape[1] != 1 else expand_nodes(xc, mask)


def expand_incidence(Hc: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """(B,E,N) of one module: rows and columns of a top-k H, the columns of a scale-N module's single row."""
    if Hc.shape[1] == 1 and mask.shape[1] != 1:
        return expand_nodes(Hc.transpose(1, 2), mask).transpose(1, 2).contiguous()
    return expand_matrix(Hc, mask)


def expand_new_H(Hc: torch.Tensor, mask: torch.Tensor, scales) -> torch.Tensor:
    """cat(H_s, dim=1), scale block by scale block."""
    N, out, e0 = mask.shape[1], [], 0
    for s in scales:
        E = C.n_edges(N, s)
        out.append(expand_incidence(Hc[:, e0:e0 + E], mask))
        e0 += E
    return torch.cat(out, dim=1)


def compact_noise(U, mask: torch.Tensor):
    """The block's noise — per module, pairwise first, its rounds' tensors — compacted like every other input."""
    return [[compact_pairs(u, mask) if i == 0 else compact_edges(u, mask) for u in us] for i, us in enumerate(U)]


# ---------------------------------------------------------------------------------------------------------------------
# the cases: those of ragged_cases.CASES, the smallest sizes that cross each form edge.  Every table holds one all-valid
# scene, one scene whose slot 0 is invalid and slot N - 1 valid, and one single-agent scene.
# ---------------------------------------------------------------------------------------------------------------------
def _rows(N: int, specs, seed: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(9000 + seed)
    rows = []
    for spec in specs:
        r = torch.zeros(N, dtype=torch.uint8)
        if spec == "all":
            r[:] = 1
        elif spec == "last":                      # a single agent, in the last slot
            r[N - 1] = 1
        elif isinstance(spec, tuple) and spec[0] == "only":
            r[spec[1]] = 1
        elif isinstance(spec, tuple) and spec[0] == "alt":
            r[spec[1]::2] = 1
        elif isinstance(spec, tuple) and spec[0] == "prefix":
            r[:spec[1]] = 1
        else:                                     # ("rand", p): holes anywhere, slot 0 invalid, slot N - 1 valid
            r = (torch.rand(N, generator=gen) < spec[1]).to(torch.uint8)
            r[0], r[N - 1] = 0, 1
        rows.append(r)
    return torch.stack(rows)


def _case(id, N, scales, specs, seed, storage, what):
    mask = _rows(N, specs, seed)
    c = C._case(id, N, [int(v) for v in mask.sum(dim=1)], scales, seed, what)
    c.update(mask=mask, storage=storage)
    return c


CASES = [
    _case("n7", 7, [2, 5, 7], ["all", ("rand", 0.6), ("only", 3), ("alt", 0), ("alt", 1), ("rand", 0.8)], 0, "fp32",
          "the N <= 16 forms; several scenes per workgroup"),
    _case("n17", 17, [2, 5, 17], ["all", ("rand", 0.6), ("only", 5), ("rand", 0.5), ("prefix", 9)], 0, "fp32",
          "stand-alone gather side"),
    _case("n50", 50, [2, 4, 8, 16], ["all", ("rand", 0.5), ("only", 17)], 1, "bf16", "the twins"),
    _case("n113", 113, [2, 8, 113], ["all", "last"], 2, "fp32", "the banded graph stage beyond the fused tile"),
    # beyond the issue's table (whose two scenes at N = 113 leave no room for holes among many agents)
    _case("n113h", 113, [2, 8, 113], [("rand", 0.7), "all"], 1, "fp32", "... with holes among many agents"),
]
BY_ID = {c["id"]: c for c in CASES}


def inputs(case: Dict, nmp: int = 1):
    """(h, U) of `ragged_cases.inputs` in the ORIGINAL layout, bf16-rounded for a bf16 case."""
    return C.inputs(case, nmp, bf16=case["storage"] == "bf16")


def compacted_inputs(case: Dict, nmp: int = 1):
    """(h, U) moved to the compacted layout by torch indexing: the ragged batch whose counts are the case's."""
    h, U = inputs(case, nmp)
    return compact_nodes(h, case["mask"]), compact_noise(U, case["mask"])


def with_nan(case: Dict, h: torch.Tensor) -> torch.Tensor:
    """h with NaN in every invalid row."""
    out = h.clone()
    out[case["mask"] == 0] = float("nan")
    return out


def nan_noise(case: Dict, U) -> List[List[torch.Tensor]]:
    """The noise with NaN at every position that has an invalid end."""
    mask, out = case["mask"], []
    for i, us in enumerate(U):
        mod = []
        for u in us:
            keep = (expand_pairs(compact_pairs(torch.ones_like(u), mask), mask) if i == 0 else
                    expand_edges(compact_edges(torch.ones_like(u), mask), mask))
            mod.append(torch.where(keep != 0, u, torch.full_like(u, float("nan"))))
        out.append(mod)
    return out
