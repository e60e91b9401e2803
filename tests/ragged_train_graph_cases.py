"""Test helper of the ragged train-graph tests (tests/test_ragged_train_graph_cpu.py, tests/test_ragged_train_graph_gpu.py):
the shapes, the count vectors and masks of the replays, and the losses both sides of a comparison share.  Pure torch; the
library is never loaded.

Shapes: the smallest that reach every route of the step — a top-k module beside a scale-N module (N = 7), the
stand-alone gather beyond 16 agents (N = 17), two message-passing rounds (N = 6).  Count vectors of a shape: a ragged
one, None (the replay sets nothing: the previous counts stay), all N, another ragged one — three different vectors, one
of them all N, and one replay that sets nothing."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import torch

D = 64


@dataclass(frozen=True)
class Shape:
    id: str
    B: int
    N: int
    scales: Tuple[int, ...]
    nmp: int
    replays: Tuple[Optional[Tuple[int, ...]], ...]
    seed: int


SHAPES = [
    Shape("n7", 5, 7, (3, 7), 1, ((7, 4, 3, 2, 1), None, (7,) * 5, (1, 7, 2, 5, 3)), 7),
    Shape("n17", 3, 17, (5,), 1, ((17, 6, 3), None, (17,) * 3, (1, 16, 9)), 17),
    Shape("n6_nmp2", 4, 6, (3,), 2, ((6, 4, 2, 1), None, (6,) * 4, (3, 1, 6, 5)), 6),
]
BY_ID = {s.id: s for s in SHAPES}
EMPTY_COUNTS = (7, 0, 3, 0, 1)          # shape n7: two empty slots among three live scenes


def counts_in_force(replays: Sequence[Optional[Sequence[int]]]) -> List[Tuple[int, ...]]:
    """The counts each replay runs with: its own, or those of the last replay that set any."""
    out, cur = [], None
    for c in replays:
        cur = cur if c is None else tuple(c)
        assert cur is not None, "the first replay must set counts"
        out.append(cur)
    return out


def prefix_valid(counts: Sequence[int], N: int) -> torch.Tensor:
    """(B,N) bool: arange(N) < counts[:, None]."""
    return torch.arange(N)[None, :] < torch.tensor(list(counts))[:, None]


def features(shape: Shape, width: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(f (B,N,64), target (B,N,width)) of a shape, N(0,1), seeded."""
    g = torch.Generator().manual_seed(4000 + shape.seed)
    return torch.randn(shape.B, shape.N, D, generator=g), torch.randn(shape.B, shape.N, width, generator=g)


def subset_masks(mask: torch.Tensor) -> List[torch.Tensor]:
    """Three different (B,N) masks with holes from a case's own: itself, its columns reversed, and one with the first
    valid agent of every scene that has two taken out.  Every scene keeps a valid agent."""
    m0 = mask != 0
    m2 = m0.clone()
    for b in range(m2.shape[0]):
        idx = torch.nonzero(m2[b]).reshape(-1)
        if len(idx) >= 2:
            m2[b, idx[0]] = False
    out = [m0, m0.flip(1), m2]
    assert all(bool(m.any(dim=1).all()) for m in out)
    assert not torch.equal(out[0], out[1]) and not torch.equal(out[0], out[2]) and not torch.equal(out[1], out[2])
    return out


class MaskedMSE:
    """Mean squared error of the module columns of ``final`` over the real agents; keeps what it was last called with
    (``seen`` = (final, new_H, valid)): for a captured step these are the graph's static tensors.  ``final`` is kept
    detached: a reference to the autograd graph would keep the warm-up's AccumulateGrad nodes alive into the capture."""

    def __init__(self):
        self.seen = None

    def __call__(self, final, new_H, target, valid):
        self.seen = (final.detach(), new_H, valid)
        d = torch.where(valid[..., None], final[..., D:] - target, torch.zeros((), device=final.device))
        return (d * d).sum() / (valid.sum().clamp(min=1) * d.shape[-1])


class PaddedDot:
    """<module columns of final, target> over EVERY position: the linear loss whose parameter gradients the per-scene
    float64 oracle states module by module (`ragged_backward_cases.module_oracle` with R1 = the module's columns of
    the target and R2 = 0).  ``valid`` is kept and not used: the module columns are zeros at invalid positions by
    contract, so the value is the sum over the real agents — and the gradient this loss puts at the invalid positions
    (the target, non-zero) is what the backward must drop."""

    def __init__(self):
        self.seen = None

    def __call__(self, final, new_H, target, valid):
        self.seen = (final.detach(), new_H, valid)
        return (final[..., D:] * target).sum()
