"""Packed weight images of the MS-HGNN modules: how they are packed, their layouts and the caches that keep them current.

`PackPlan` packs every image of one module into one arena refreshed by one launch; `XImages` splits its tile streams
into the 16-bit-core images; `repack_scope` turns a training step's refreshes into two launches.  A layout is a builder
``(plan, layers) -> packed dict`` over one `PackPlan`.  Matrices are virtual matrices made of placed parts
``[(W, place_r, place_c)]``; `pair` emits a layer pair in `pipeline_order`.  Each module keeps its `WeightCache`s in one
registry (`cache`), which `MS_HGNN_batch.invalidate_weight_caches` walks.
"""
from __future__ import annotations

import math
from typing import Callable, Iterable, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import addr, check, load, stream_handle
from .ops import _req

Tensor = torch.Tensor
Parts = Sequence[Tuple[Tensor, int, int]]     # [(W, place_r, place_c)]: a virtual matrix
_HID = 128           # hidden width of the typed aggregation MLPs (model/MS_HGNN_batch.py:253-255)
_LGF_LD = 32         # leading dimension of the backward's (logits | factor pre-activation) layer


# ---------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------
def pack_linear(W: Tensor, col_offset: int = 0, in_features: Optional[int] = None) -> Tensor:
    """Packed image of an nn.Linear weight (out x in), or of the column block
    [col_offset, col_offset + in_features) of it."""
    _req(W, "W", (None, None))
    out_f, ld = W.shape
    in_f = ld - col_offset if in_features is None else in_features
    lib = load()
    Wp = torch.empty(lib.gn_packed_elems(out_f, in_f), dtype=W.dtype, device=W.device)
    with torch.cuda.device(W.device):
        check(lib.gn_pack_linear_f32(addr(W), addr(Wp), out_f, in_f, ld, col_offset, stream_handle()),
              "gn_pack_linear_f32")
    return Wp


def pack_stream(weights: Sequence[Tensor]) -> Tensor:
    """One weight stream: the packed images of `weights` (nn.Linear layout, out x in) back to back, in
    the order a kernel consumes them."""
    return torch.cat([pack_linear(w.detach().contiguous()) for w in weights])


def edge_stream(Wi0: Tensor, Wi1: Tensor, Wd0: Tensor, Wd1: Tensor) -> Tensor:
    """Weight stream of the edge-MLP kernel: the packed images of its four layers cut into hidden tiles
    (T, 8 steps) and second-layer slices (S) and laid out in the order the kernel consumes them —
    pair A: T0 T1 S0 T2 S1 T3 S2 S3 (S = both output tiles over one hidden tile, 8 steps);
    pair B: T0 T1 S0 T2 S1 ... T7 S6 S7 (S = 4 steps).  One step = 256 floats."""
    a0 = pack_linear(Wi0.detach().contiguous()).view(4, 8, 256)          # (128 x 64): 4 tiles x 8 steps
    a1 = pack_linear(Wi1.detach().contiguous()).view(2, 4, 4, 256)       # (64 x 128): (o, t) x 4 steps
    b0 = pack_linear(Wd0.detach().contiguous()).view(8, 8, 256)          # (256 x 64): 8 tiles x 8 steps
    b1 = pack_linear(Wd1.detach().contiguous()).view(1, 8, 4, 256)       # (32 x 256): (0, t) x 4 steps
    sa = lambda t: a1[:, t].reshape(8, 256)                               # slices (0,t), (1,t)
    sb = lambda t: b1[0, t]
    parts = [a0[0], a0[1], sa(0), a0[2], sa(1), a0[3], sa(2), sa(3)]
    parts += [b0[0], b0[1]]
    for t in range(8):
        parts.append(sb(t))
        if t < 6:
            parts.append(b0[t + 2])
    parts.append(a0.new_zeros(8, 256))      # the kernel's ring reads 8 steps ahead of the last one it uses
    return torch.cat([p.reshape(-1) for p in parts]).contiguous()


def bias_stream(biases: Sequence[Tensor]) -> Tensor:
    """Biases back to back, each zero-padded to a multiple of 32 (one 32-float tile per output tile)."""
    parts = []
    for b in biases:
        b = b.detach().reshape(-1)
        pad = (-b.numel()) % 32
        parts.append(torch.cat((b, b.new_zeros(pad))) if pad else b)
    return torch.cat(parts).contiguous()


def pipeline_order(HT: int) -> List[Tuple[str, int]]:
    """Order in which the bf16-core kernels consume the tiles of one layer pair with HT hidden tiles
    (gn_mlp_bf16.hpp, layer_pair): A_t = the first-layer tiles producing hidden tile t, B_t = the second-layer
    tiles consuming it;  A0 A1 B0 A2 B1 ... A(HT-1) B(HT-2) B(HT-1)."""
    out = [("A", 0)]
    for t in range(HT):
        if t + 1 < HT:
            out.append(("A", t + 1))
        out.append(("B", t))
    return out


def split_bf16(packed: Tensor, out: Optional[Tensor] = None, parts: int = 3) -> Tensor:
    """bf16-core image (16-bit words, as int16) of packed fp32 32x32 weight tiles: `gn_split_bf16_f32`
    (parts = 3: x = p1 + p2 + p3, the fp32-accurate path; parts = 1: x rounded to bf16, the twins; parts = 2: two fp16
    parts x = hi + lo — the f16x3 path — followed by the 16-byte range flag)."""
    _req(packed, "packed")
    n_tiles = packed.numel() // 1024
    if out is None:
        n = n_tiles * 2 * parts * 64 * 8
        out = (torch.zeros(n + 8, dtype=torch.int16, device=packed.device) if parts == 2 else     # (+ the flag word)
               torch.empty(n, dtype=torch.int16, device=packed.device))
    if _REPACK["rec"] is not None:
        _REPACK["rec"][1].append((packed, out, int(parts)))
    elif _REPACK["done_splits"] is not None and (packed.data_ptr(), out.data_ptr(), int(parts)) in _REPACK["done_splits"]:
        return out      # this step's RepackBatch built it already
    with torch.cuda.device(packed.device):
        check(load().gn_split_bf16_f32(addr(packed), addr(out), n_tiles, int(parts), stream_handle()),
              "gn_split_bf16_f32")
    return out


class XImages:
    """bf16-core weight images of one packed-weight set (`gn_split_bf16_f32`), built on demand per number of
    parts (3: the fp32-accurate path of the fp32 entry points, 1: the bf16 twins) from hidden-tile-major fp32
    tile streams of a `PackPlan` arena, and rebuilt whenever the owner bumps `version` after a refresh."""

    def __init__(self, **src: Tensor):
        self.src = src
        self.img = {}
        self.version = 0

    def bump(self) -> None:
        self.version += 1

    def get(self, name: str, parts: int) -> Tensor:
        hit = self.img.get((name, parts))
        src = self.src[name]
        if hit is None:
            n = src.numel() // 1024 * 2 * parts * 64 * 8
            # (two fp16 parts: + the 16-byte flag word behind the image; every split clears it before it may raise it)
            buf = (torch.zeros(n + 8, dtype=torch.int16, device=src.device) if parts == 2 else
                   torch.empty(n, dtype=torch.int16, device=src.device))
            hit = self.img[(name, parts)] = [buf, -1]
        if hit[1] != self.version:
            split_bf16(src, hit[0], parts)
            hit[1] = self.version
        return hit[0]


class PackPlan:
    """All packed weight images of one module as ONE arena refreshed by ONE launch.

    Built once (per module and parameter addresses): `block` / `place` / `vector` record segments of
    `gn_pack_segments_f32` and hand out arena offsets; `finish()` uploads the segment table to the device.
    `refresh()` = one kernel launch, reading the parameters in place — what has to happen after every
    optimizer step, capturable in a hipGraph."""

    TILE = 1024

    def __init__(self, device: torch.device):
        self.device = device
        self.size = 0
        self._segs: List[Tuple[int, dict]] = []      # (arena offset of the destination, the other gn_pack_seg_t fields)
        self._keep: List[Tensor] = []
        self.arena: Optional[Tensor] = None
        self.table: Optional[Tensor] = None
        self.max_elems = 1

    def alloc(self, numel: int) -> int:
        off = self.size
        self.size += (numel + 63) // 64 * 64          # keeps every image 256-byte aligned
        return off

    def _seg(self, dst_off: int, W: Tensor, **seg) -> None:
        self._keep.append(W)
        self._segs.append((dst_off, seg))
        self.max_elems = max(self.max_elems, seg["rows"] * seg["cols"])

    def block(self, dst_off: int, W: Tensor, IT: int, r0=0, c0=0, rows=None, cols=None, place_r=0, place_c=0,
              scale=1.0) -> None:
        """W[r0:r0+rows, c0:c0+cols] -> the packed image at arena offset dst_off (IT tiles per packed row),
        at (place_r, place_c) of its virtual matrix."""
        W = W.detach()
        if W.dim() != 2 or W.stride(1) != 1 or W.dtype != torch.float32 or W.device != self.device:
            raise ValueError("PackPlan.block: 2-D fp32 row-major matrix on the plan's device")
        rows = W.shape[0] - r0 if rows is None else rows
        cols = W.shape[1] - c0 if cols is None else cols
        self._seg(dst_off, W, src=W.data_ptr() + 4 * (r0 * W.stride(0) + c0), ld=W.stride(0), rows=rows, cols=cols,
                  place_r=place_r, place_c=place_c, IT=IT, scale=float(scale))

    def place(self, dst_off: int, dst_ld: int, W: Tensor, place_r=0, place_c=0, scale=1.0) -> None:
        """W (2-D, or a vector as one row) -> rows [place_r, ...) x columns [place_c, ...) of the plain row-major
        (.., dst_ld) matrix at arena offset dst_off: concatenations without torch.cat."""
        W = W.detach()
        W = W.reshape(1, -1) if W.dim() == 1 else W
        if W.dim() != 2 or W.stride(1) != 1 or W.dtype != torch.float32 or W.device != self.device:
            raise ValueError("PackPlan.place: fp32 row-major matrix or vector on the plan's device")
        self._seg(dst_off, W, src=W.data_ptr(), ld=W.stride(0), rows=W.shape[0], cols=W.shape[1], place_r=place_r,
                  place_c=place_c, scale=float(scale), dst_ld=dst_ld)

    def vector(self, dst_off: int, v: Tensor, place=0, scale=1.0) -> None:
        v = v.detach().reshape(1, -1)
        if v.stride(1) != 1 or v.dtype != torch.float32 or v.device != self.device:
            raise ValueError("PackPlan.vector: contiguous fp32 vector on the plan's device")
        self._seg(dst_off, v, src=v.data_ptr(), ld=v.shape[1], rows=1, cols=v.shape[1], place_c=place,
                  scale=float(scale))

    def finish(self) -> "PackPlan":
        self.arena = torch.zeros(max(self.size, 64), dtype=torch.float32, device=self.device)
        base = self.arena.data_ptr()
        arr = (_lib.PackSeg * len(self._segs))(*[_lib.PackSeg(dst=base + 4 * off, **seg) for off, seg in self._segs])
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.table = raw.to(self.device)
        return self

    def view(self, off: int, numel: int) -> Tensor:
        return self.arena[off:off + numel]

    def refresh(self) -> None:
        # (segments always write the same positions: the padding zeroed in finish() stays zero)
        if _REPACK["rec"] is not None:
            _REPACK["rec"][0].append(self)
        elif _REPACK["done_plans"] is not None and id(self) in _REPACK["done_plans"]:
            return      # this step's RepackBatch refreshed it already
        with torch.cuda.device(self.device):
            check(load().gn_pack_segments_f32(addr(self.table), len(self._segs), self.max_elems, stream_handle()),
                  "gn_pack_segments_f32")


T = PackPlan.TILE


# ---- one re-pack per training step -----------------------------------------------------------------------------
# A training step re-derives every packed weight image from the parameters (the optimizer just rewrote them): one
# `refresh` launch per pack plan and one `split_bf16` launch per bf16-core image — 21 + 17 launches of ~4.6 us per step
# of the multiscale block, 9 % of the graphed step.  All of them read only the parameters, so they can run first and
# together: `repack_scope` RECORDS which plans / images one step touches (first use), then runs them as TWO launches —
# `gn_pack_segments_f32` over the concatenated segment tables, `gn_split_bf16_batch_f32` over all images — at the head
# of every later step and turns the recorded per-plan / per-image launches of that step into no-ops.  A plan or image
# that is not in the batch (rebuilt because parameter storage moved) simply takes its own launch as before.
_REPACK = {"rec": None, "done_plans": None, "done_splits": None}


class RepackBatch:
    def __init__(self, plans: Sequence["PackPlan"], splits: Sequence[Tuple[Tensor, Tensor, int]]):
        self.plans, self.splits = list(plans), list(splits)          # (keeps arenas, tables and images alive)
        dev = self.plans[0].device
        self.device = dev
        self.table = torch.cat([p.table for p in self.plans])
        self.n_segs = sum(len(p._segs) for p in self.plans)
        self.max_elems = max(p.max_elems for p in self.plans)
        if self.n_segs > 65535:
            raise ValueError("RepackBatch: too many segments for one launch")
        self.parts = sorted({pt for _, _, pt in self.splits})
        self.jobs = {}
        for pt in self.parts:
            js = [(a, b) for a, b, q in self.splits if q == pt]
            arr = (_lib.SplitJob * len(js))(*[_lib.SplitJob(packed=a.data_ptr(), out=b.data_ptr(),
                                                            n_tiles=a.numel() // 1024) for a, b in js])
            raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
            self.jobs[pt] = (raw, len(js), max(a.numel() // 1024 for a, _ in js))
        self.plan_ids = {id(p) for p in self.plans}
        self.split_keys = {(a.data_ptr(), b.data_ptr(), q) for a, b, q in self.splits}

    def run(self) -> None:
        with torch.cuda.device(self.device):
            check(load().gn_pack_segments_f32(addr(self.table), self.n_segs, self.max_elems, stream_handle()),
                  "gn_pack_segments_f32")
            for pt, (raw, n, mx) in self.jobs.items():
                check(load().gn_split_bf16_batch_f32(addr(raw), n, mx, pt, stream_handle()), "gn_split_bf16_batch_f32")


class repack_scope:
    """``with repack_scope(holder):`` around ONE whole training step (forward and backward).  `holder` is a dict owned by
    the caller; its first use records, later uses replay the batch (see above).  Not re-entrant."""

    def __init__(self, holder: dict):
        self.h = holder

    def __enter__(self):
        if _REPACK["rec"] is not None or _REPACK["done_plans"] is not None:
            raise RuntimeError("repack_scope is not re-entrant")
        batch = self.h.get("batch")
        if batch is None:
            _REPACK["rec"] = ([], [])
        else:
            batch.run()
            _REPACK["done_plans"], _REPACK["done_splits"] = batch.plan_ids, batch.split_keys
        return self

    def __exit__(self, et, ev, tb):
        rec = _REPACK["rec"]
        _REPACK["rec"] = _REPACK["done_plans"] = _REPACK["done_splits"] = None
        if rec is not None and et is None:
            plans, seen = [], set()
            for p in rec[0]:
                if id(p) not in seen:
                    seen.add(id(p))
                    plans.append(p)
            splits, seen2 = [], set()
            for a, b, q in rec[1]:
                k = (a.data_ptr(), b.data_ptr(), q)
                if k not in seen2:
                    seen2.add(k)
                    splits.append((a, b, q))
            self.h["batch"] = RepackBatch(plans, splits) if plans else None
        return False


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
    """One packed dict derived from one parameter set by one `PackPlan`.  The plan (arena and segment table)
    is rebuilt when the parameters' storage moves; its one refresh launch runs when their versions moved or
    `_volatile` says so — or on every call with ``always`` (the backward's concatenations: a backward is part of a
    training step by definition)."""

    def __init__(self, always: bool = False):
        self.always = always
        self.ptrs = self.plan = self.pk = self.key = None

    def get(self, params: Sequence[nn.Parameter], build: Callable[[PackPlan], dict]) -> dict:
        ptrs = tuple(p.data_ptr() for p in params)
        if ptrs != self.ptrs:
            self.plan = PackPlan(params[0].device)
            self.pk = build(self.plan)
            self.ptrs, self.key = ptrs, None
        if _SEEN[0] is not None:
            _SEEN[0].append((self, tuple(params)))
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
        _EPOCH[0] += 1


# ---- what a captured inference forward reads --------------------------------------------------------------------
# Under no_grad `WeightCache.get` trusts the packed images, so a forward captured after its warm-up contains no pack or
# split launch: the graph reads the arenas and the split images where they lie.  `seen_caches` records which caches
# (with their parameters) a warm-up step asked; `CapturedWeights` keeps their plans and images alive and re-derives all
# of them in place.  `_EPOCH` counts invalidations (`WeightCache.invalidate`, `note_invalidation`): ONE integer compare
# tells a replay whether anything was distrusted since its images were last derived.
_SEEN: list = [None]
_EPOCH = [0]


def note_invalidation() -> None:
    """Something derived from parameters that is not a `WeightCache` (the encoders' composed embedding) was distrusted."""
    _EPOCH[0] += 1


class seen_caches:
    """``with seen_caches() as seen:`` — every `WeightCache.get` inside appends (cache, parameters).  Not re-entrant."""

    def __enter__(self) -> list:
        if _SEEN[0] is not None:
            raise RuntimeError("seen_caches is not re-entrant")
        _SEEN[0] = []
        return _SEEN[0]

    def __exit__(self, *exc):
        _SEEN[0] = None
        return False


def moved_storage(what: str) -> RuntimeError:
    return RuntimeError(f"{what}: a parameter's storage moved since the capture; the graph reads the packed images "
                        "derived from the old storage and cannot follow — capture the graph again")


class CapturedWeights:
    """The pack plans and split images a captured forward reads, as `seen_caches` recorded them right after the
    capture.  `refresh()` re-derives every one from the live parameters at the captured addresses, on the current
    stream; `check()` refuses, before anything is launched, where a parameter's storage has moved since."""

    def __init__(self, seen: Sequence[Tuple["WeightCache", tuple]]):
        self.entries, ids = [], set()
        for c, params in seen:
            if id(c) not in ids:
                ids.add(id(c))
                self.entries.append((c, params, c.ptrs, c.plan, c.pk))       # (keeps arenas, tables and images alive)
        self.epoch = _EPOCH[0]

    def check(self, what: str) -> None:
        for _, params, ptrs, _, _ in self.entries:
            if tuple(p.data_ptr() for p in params) != ptrs:
                raise moved_storage(what)

    def refresh(self, what: str) -> None:
        self.check(what)
        for c, params, _, plan, pk in self.entries:
            plan.refresh()
            xi = pk.get("xi")
            if xi is not None:
                xi.bump()
                for name, parts in list(xi.img):       # every image that exists: the captured forward's are among them
                    xi.get(name, parts)
            if c.plan is plan:
                c.key = _param_key(params)             # what the eager path now may trust as well
        self.epoch = _EPOCH[0]


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


def _window(plan: PackPlan, off: int, parts: Parts, IT: int, r: int, c: int, nr: int, nc: int) -> None:
    """Rows [r, r+nr) x columns [c, c+nc) of the virtual matrix made of `parts` -> the packed image (IT tiles per
    packed row) at arena offset `off`."""
    for W, pr, pc in parts:
        r0, r1 = max(r, pr), min(r + nr, pr + W.shape[0])
        c0, c1 = max(c, pc), min(c + nc, pc + W.shape[1])
        if r0 < r1 and c0 < c1:
            plan.block(off, W, IT, r0=r0 - pr, c0=c0 - pc, rows=r1 - r0, cols=c1 - c0, place_r=r0 - r, place_c=c0 - c)


def _second(plan: PackPlan, off: int, second: Parts, t: int) -> int:
    """B_t: the tiles of the second layer consuming hidden tile t, one per output tile; returns the next offset."""
    for o in range(_extent(second)[0]):
        _window(plan, off, second, 1, 32 * o, 32 * t, 32, 32)
        off += T
    return off


def pair(plan: PackPlan, first: Parts, second: Parts) -> int:
    """A layer pair in pipeline order (A_t = the first-layer rows producing hidden tile t, B_t = the second-layer
    columns consuming it; a ragged last output tile is zero-padded); returns its arena offset."""
    HT, IT = _extent(first)
    off = start = plan.alloc(HT * (IT + _extent(second)[0]) * T)
    for kind, t in pipeline_order(HT):
        if kind == "A":
            _window(plan, off, first, IT, 32 * t, 0, 32, 32 * IT)
            off += IT * T
        else:
            off = _second(plan, off, second, t)
    return start


def matrix(plan: PackPlan, parts: Parts) -> int:
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
def node_chain(plan: PackPlan, start: Tuple[nn.Linear, nn.Linear], att: Tuple[nn.Linear, nn.Linear]) -> dict:
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
    return dict(W=plan.view(w0, w_len), bias=plan.view(bo, 384), xi=XImages(chain=plan.view(wc, wc_len)),
                w2=a1.weight.detach()[0], b2=a1.bias.detach())    # views of the parameters: no host sync


def edge_mlp(plan: PackPlan, init: Tuple[nn.Linear, nn.Linear], dist: Tuple[nn.Linear, nn.Linear],
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
    return dict(W=plan.view(w0, w_len), bias=plan.view(bo, 480), xi=XImages(edge=plan.view(w0, n_img)))


def typed_agg(plan: PackPlan, l0: Sequence[nn.Linear], l1: Sequence[nn.Linear]) -> dict:
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
    pk["xi"] = XImages(W2t=pk["W2t"],                         # layer 2 per hidden tile (pair form)
                           W12=plan.view(w12, w12_len),             # both layers, hidden-tile-major (two-layer form)
                           W1cat=pk["W1cat"])                       # layer 1 of all types per node (node stage)
    return pk


def closing_mlp(plan: PackPlan, l0: nn.Linear, l1: nn.Linear) -> dict:
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
    xi = XImages() if wh is None else XImages(mlp2=plan.view(wh, wh_len))
    return dict(W=plan.view(w0, w_len), bias=plan.view(bo, pad(dh) + pad(dout)), xi=xi, din=din, dh=dh, dout=dout)


def backward_cat(plan: PackPlan, a0: nn.Linear, dist: Tuple[nn.Linear, nn.Linear], fac: Tuple[nn.Linear, nn.Linear],
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
