"""Packed weight images of the MS-HGNN modules: their layouts and the caches that keep them current.

A layout is a builder ``(plan, layers) -> packed dict`` over one `ops.PackPlan`.  Matrices are virtual matrices made
of placed parts ``[(W, place_r, place_c)]``; `pair` emits a layer pair in `ops.pipeline_order`.  Each module keeps its
`WeightCache`s in one registry (`cache`), which `MS_HGNN_batch.invalidate_weight_caches` walks.
"""
from __future__ import annotations

import math
from typing import Callable, Iterable, Sequence, Tuple

import torch
import torch.nn as nn

from . import ops

Tensor = torch.Tensor
T = ops.PackPlan.TILE
Parts = Sequence[Tuple[Tensor, int, int]]     # [(W, place_r, place_c)]: a virtual matrix
_HID = 128           # hidden width of the typed aggregation MLPs (model/MS_HGNN_batch.py:253-255)
_LGF_LD = 32         # leading dimension of the backward's (logits | factor pre-activation) layer


# ---------------------------------------------------------------------------------------------
# cache policy
# ---------------------------------------------------------------------------------------------
def _param_key(params: Iterable[nn.Parameter]):
    """Cheap fingerprint of a parameter set: storage address + in-place version counter."""
    return tuple((p.data_ptr(), p._version) for p in params)


def _volatile(params: Iterable[nn.Parameter]) -> bool:
    """Whether the packed-image cache must not be trusted for this call.  The fingerprint above misses writes
    made through ``p.data`` / raw pointers (they do not bump ``_version``) — the idiom of hand-written
    optimizers, EMA updates, weight clamping and the reference's own ``m.bias.data.fill_`` re-initialisation.
    While autograd is recording for these parameters (a training step) every call therefore re-runs the one
    refresh launch of its pack plan; only inference (no-grad / frozen parameters) trusts the cache, and code
    that rewrites weights there behind autograd's back calls `invalidate_weight_caches`."""
    return _TRAINING_CALL[0] or (torch.is_grad_enabled() and any(p.requires_grad for p in params))


_TRAINING_CALL = [False]


class training_call:
    """Context of a forward that belongs to a training step (`backward.MSHGNNFunction.forward` runs under
    no_grad, so `_volatile` cannot see it from the grad mode)."""

    def __enter__(self):
        self.prev, _TRAINING_CALL[0] = _TRAINING_CALL[0], True

    def __exit__(self, *exc):
        _TRAINING_CALL[0] = self.prev
        return False


class WeightCache:
    """One packed dict derived from one parameter set by one `ops.PackPlan`.  The plan (arena and segment table)
    is rebuilt when the parameters' storage moves; its one refresh launch runs when their versions moved or
    `_volatile` says so — or on every call with ``always`` (the backward's concatenations: a backward is part of a
    training step by definition)."""

    def __init__(self, always: bool = False):
        self.always = always
        self.ptrs = self.plan = self.pk = self.key = None

    def get(self, params: Sequence[nn.Parameter], build: Callable[[ops.PackPlan], dict]) -> dict:
        ptrs = tuple(p.data_ptr() for p in params)
        if ptrs != self.ptrs:
            self.plan = ops.PackPlan(params[0].device)
            self.pk = build(self.plan)
            self.ptrs, self.key = ptrs, None
        if self.always:
            self.plan.refresh()
            return self.pk
        key = _param_key(params)
        if key != self.key or _volatile(params):
            self.plan.refresh()
            self.pk["xi"].bump()
            self.key = key
        return self.pk

    def invalidate(self) -> None:
        """Distrust the packed images: the next `get` refreshes them (the plan itself stays)."""
        self.key = None


def cache(owner: nn.Module, name, always: bool = False) -> WeightCache:
    """The weight cache `name` of `owner`, registered on first use in the owner's one registry."""
    reg = owner.__dict__.get("_gn_weights")
    if reg is None:
        reg = owner.__dict__["_gn_weights"] = {}
    c = reg.get(name)
    if c is None:
        c = reg[name] = WeightCache(always)
    return c


def caches(owner: nn.Module) -> Iterable[WeightCache]:
    return owner.__dict__.get("_gn_weights", {}).values()


# ---------------------------------------------------------------------------------------------
# emitter
# ---------------------------------------------------------------------------------------------
def _extent(parts: Parts) -> Tuple[int, int]:
    """Tiles (rows, columns) of the virtual matrix made of `parts`."""
    return (max(pr + W.shape[0] for W, pr, _ in parts) + 31) // 32, (max(pc + W.shape[1] for W, _, pc in parts) + 31) // 32


def _window(plan: ops.PackPlan, off: int, parts: Parts, IT: int, r: int, c: int, nr: int, nc: int) -> None:
    """Rows [r, r+nr) x columns [c, c+nc) of the virtual matrix made of `parts` -> the packed image (IT tiles per
    packed row) at arena offset `off`."""
    for W, pr, pc in parts:
        r0, r1 = max(r, pr), min(r + nr, pr + W.shape[0])
        c0, c1 = max(c, pc), min(c + nc, pc + W.shape[1])
        if r0 < r1 and c0 < c1:
            plan.block(off, W, IT, r0=r0 - pr, c0=c0 - pc, rows=r1 - r0, cols=c1 - c0, place_r=r0 - r, place_c=c0 - c)


def _second(plan: ops.PackPlan, off: int, second: Parts, t: int) -> int:
    """B_t: the tiles of the second layer consuming hidden tile t, one per output tile; returns the next offset."""
    for o in range(_extent(second)[0]):
        _window(plan, off, second, 1, 32 * o, 32 * t, 32, 32)
        off += T
    return off


def pair(plan: ops.PackPlan, first: Parts, second: Parts) -> int:
    """A layer pair in pipeline order (A_t = the first-layer rows producing hidden tile t, B_t = the second-layer
    columns consuming it; a ragged last output tile is zero-padded); returns its arena offset."""
    HT, IT = _extent(first)
    off = start = plan.alloc(HT * (IT + _extent(second)[0]) * T)
    for kind, t in ops.pipeline_order(HT):
        if kind == "A":
            _window(plan, off, first, IT, 32 * t, 0, 32, 32 * IT)
            off += IT * T
        else:
            off = _second(plan, off, second, t)
    return start


def matrix(plan: ops.PackPlan, parts: Parts) -> int:
    """The whole virtual matrix made of `parts` as one packed image; returns its arena offset."""
    OT, IT = _extent(parts)
    off = plan.alloc(OT * IT * T)
    _window(plan, off, parts, IT, 0, 0, 32 * OT, 32 * IT)
    return off


def _one(l: nn.Linear) -> Parts:
    return [(l.weight, 0, 0)]


# ---------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------
def node_chain(plan: ops.PackPlan, start: Tuple[nn.Linear, nn.Linear], att: Tuple[nn.Linear, nn.Linear]) -> dict:
    """Node stage: node2edge_start_mlp and the node half of attention_mlp.  Attention layer 0 acts on
    cat(x'_n, e0_e): it is split into the node half (with the bias) and the edge half, which by linearity is applied
    to x' before the H-pooling: Wpq = [W[:, :D]; W[:, D:]].  W = the fp32-core stream (matrix by matrix), "chain" =
    the same chain in pipeline order followed by Wpq."""
    (s0, s1), (a0, a1) = start, att
    D = a0.in_features // 2
    wpq = [(a0.weight[:, :D], 0, 0), (a0.weight[:, D:], a0.out_features, 0)]
    w0 = matrix(plan, _one(s0))
    matrix(plan, _one(s1))
    matrix(plan, wpq)
    w_len = plan.size - w0
    wc = pair(plan, _one(s0), _one(s1))
    matrix(plan, wpq)
    wc_len = plan.size - wc
    bo = plan.alloc(256 + 64 + 64)
    plan.vector(bo, s0.bias)
    plan.vector(bo + 256, s1.bias)
    plan.vector(bo + 320, a0.bias)
    plan.finish()
    return dict(W=plan.view(w0, w_len), bias=plan.view(bo, 384), xi=ops.XImages(chain=plan.view(wc, wc_len)),
                w2=a1.weight.detach()[0], b2=a1.bias.detach())    # views of the parameters: no host sync


def edge_mlp(plan: ops.PackPlan, init: Tuple[nn.Linear, nn.Linear], dist: Tuple[nn.Linear, nn.Linear],
             fac: Tuple[nn.Linear, nn.Linear]) -> dict:
    """Edge MLP: pair A = init_MLP; pair B = MLP_distribution's hidden layer over MLP_factor's (rows 128..255) and the
    (logits | factor) head over them, d1 in rows 0..K-1 and f1 in row K over hidden columns 128..255.  The 40 tiles
    of both pairs are the source of the bf16-core image; W (fp32 cores) is the same tiles plus two zero tiles, which
    the kernel's ring reads ahead of the last one it uses."""
    (i0, i1), (d0, d1), (f0, f1) = init, dist, fac
    K, H = d1.out_features, d0.out_features
    w0 = pair(plan, _one(i0), _one(i1))
    pair(plan, [(d0.weight, 0, 0), (f0.weight, H, 0)], [(d1.weight, 0, 0), (f1.weight, K, H)])
    n_img = plan.size - w0
    plan.alloc(2 * T)
    w_len = plan.size - w0
    bo = plan.alloc(128 + 64 + 256 + 32)
    plan.vector(bo, i0.bias)
    plan.vector(bo + 128, i1.bias)
    plan.vector(bo + 192, d0.bias)
    plan.vector(bo + 320, f0.bias)
    plan.vector(bo + 448, d1.bias)
    plan.vector(bo + 448, f1.bias, place=K)
    plan.finish()
    return dict(W=plan.view(w0, w_len), bias=plan.view(bo, 480), xi=ops.XImages(edge=plan.view(w0, n_img)))


def typed_agg(plan: ops.PackPlan, l0: Sequence[nn.Linear], l1: Sequence[nn.Linear]) -> dict:
    """The K typed aggregation MLPs: W (both layers, type by type), b1 / b2, and for the pairwise form layer 1 of
    all types as one (K*128 x 64) matrix applied per node (half the bias rides with each of the two nodes of a pair)
    and layer 2 per hidden tile; W12 = both layers of each type in pipeline order (two-layer form)."""
    K = len(l0)
    w0 = plan.alloc(0)
    for a, b in zip(l0, l1):
        matrix(plan, _one(a))
        matrix(plan, _one(b))
    w_len = plan.size - w0
    b1o, b2o, bho = plan.alloc(K * 128), plan.alloc(K * 64), plan.alloc(K * 128)
    w1c, w2t = plan.alloc(K * 8 * T), plan.alloc(K * 8 * T)
    w12 = plan.size
    for k in range(K):
        pair(plan, _one(l0[k]), _one(l1[k]))
        plan.vector(b1o + 128 * k, l0[k].bias)
        plan.vector(b2o + 64 * k, l1[k].bias)
        plan.vector(bho + 128 * k, l0[k].bias, scale=0.5)
        plan.block(w1c + k * 8 * T, l0[k].weight, 2)
        off = w2t + k * 8 * T
        for t in range(4):
            off = _second(plan, off, _one(l1[k]), t)
    w12_len = plan.size - w12
    plan.finish()
    pk = dict(W=plan.view(w0, w_len), b1=plan.view(b1o, K * 128).view(K, 128), b2=plan.view(b2o, K * 64).view(K, 64),
              W1cat=plan.view(w1c, K * 8 * T), b1half=plan.view(bho, K * 128), W2t=plan.view(w2t, K * 8 * T))
    pk["xi"] = ops.XImages(W2t=pk["W2t"],                         # layer 2 per hidden tile (pair form)
                           W12=plan.view(w12, w12_len),             # both layers, hidden-tile-major (two-layer form)
                           W1cat=pk["W1cat"])                       # layer 1 of all types per node (node stage)
    return pk


def closing_mlp(plan: ops.PackPlan, l0: nn.Linear, l1: nn.Linear) -> dict:
    """A two-layer MLP of the node rows (the rounds' closing MLPs): W (matrix by matrix), and in pipeline order the
    source of the bf16-core image where the kernels take one (dout <= 64, din and dh multiples of 32)."""
    w0 = matrix(plan, _one(l0))
    matrix(plan, _one(l1))
    w_len = plan.size - w0
    pad = lambda n: (n + 31) // 32 * 32
    din, dh, dout = l0.in_features, l0.out_features, l1.out_features
    wh = None
    if dout <= 64 and din % 32 == 0 and dh % 32 == 0:
        wh = pair(plan, _one(l0), _one(l1))
        wh_len = plan.size - wh
    bo = plan.alloc(pad(dh) + pad(dout))
    plan.vector(bo, l0.bias)
    plan.vector(bo + pad(dh), l1.bias)
    plan.finish()
    xi = ops.XImages() if wh is None else ops.XImages(mlp2=plan.view(wh, wh_len))
    return dict(W=plan.view(w0, w_len), bias=plan.view(bo, pad(dh) + pad(dout)), xi=xi, din=din, dh=dh, dout=dout)


def backward_cat(plan: ops.PackPlan, a0: nn.Linear, dist: Tuple[nn.Linear, nn.Linear], fac: Tuple[nn.Linear, nn.Linear],
                 l0: Sequence[nn.Linear], l1: Sequence[nn.Linear]) -> dict:
    """The concatenated weight matrices a round's backward GEMMs read — the K typed MLPs as one wide layer,
    MLP_distribution | MLP_factor side by side, the split attention layer 0 — as plain row-major matrices."""
    (d0, d1), (f0, f1) = dist, fac
    K, D = len(l0), ops.FEAT
    shapes = dict(W1cat=(K * _HID, D), b1cat=(K * _HID,), W2cat=(D, K * _HID), b2mat=(K, D), Wd0=(256, D), bd0=(256,),
                  Wd1=(_LGF_LD, 256), bd1=(_LGF_LD,), Wpq=(D, D), bpq=(D,))
    off = {n: plan.alloc(math.prod(shp)) for n, shp in shapes.items()}
    for k in range(K):
        plan.place(off["W1cat"], D, l0[k].weight, place_r=k * _HID)           # (K*128, 64)
        plan.place(off["b1cat"], 0, l0[k].bias, place_c=k * _HID)
        plan.place(off["W2cat"], K * _HID, l1[k].weight, place_c=k * _HID)     # (64, K*128)
        plan.place(off["b2mat"], 0, l1[k].bias, place_c=k * D)                 # (K, 64)
    plan.place(off["Wd0"], D, d0.weight)                                       # hidden layers side by side
    plan.place(off["Wd0"], D, f0.weight, place_r=128)
    plan.place(off["bd0"], 0, d0.bias)
    plan.place(off["bd0"], 0, f0.bias, place_c=128)
    plan.place(off["Wd1"], 256, d1.weight)                                     # rows 0..K-1: logits over hidden[:128]
    plan.place(off["Wd1"], 256, f1.weight, place_r=K, place_c=128)             # row K: factor over hidden[128:]
    plan.place(off["bd1"], 0, d1.bias)
    plan.place(off["bd1"], 0, f1.bias, place_c=K)
    plan.place(off["Wpq"], D, a0.weight[:, :D])                                # P = W[:, :64] x' + b
    plan.place(off["Wpq"], D, a0.weight[:, D:], place_r=32)                    # Qn = W[:, 64:] x'
    plan.place(off["bpq"], 0, a0.bias)
    plan.finish()
    return {n: plan.view(off[n], math.prod(shp)).view(*shp) for n, shp in shapes.items()}
