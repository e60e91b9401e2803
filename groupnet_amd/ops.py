"""Python faces of the HIP kernels: argument checking, output allocation, launch.

One function per C-ABI entry point of include/groupnet_hip.h.  Tensors must be fp32,
contiguous and on a HIP device; anything else raises ValueError (the reference would
instead crash on device tensors, SURVEY.md §8b "Errors").  Nothing here touches the
CPU oracle or falls back to torch math.
"""
from __future__ import annotations

import ctypes
import functools
import math
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import _P, addr, check, load, stream_handle
# the kernel limits live beside the forward's route, which reads them without loading torch or the library
from .route import MASK_MAX_N, NODE_FORM_MAX_K, NODE_FORM_MAX_N, POOL_KERNEL_MAX_N, SCENE_FORM_MAX_N  # noqa: F401

Tensor = torch.Tensor
FEAT = 64


_ACT_DTYPES = (torch.float32, torch.bfloat16)   # storage types of activations: the *_f32 kernels and their *_bf16 twins


def _req(t: Tensor, name: str, shape: Optional[Sequence[Optional[int]]] = None, dtype=torch.float32) -> Tensor:
    """`dtype`: the required dtype, or a tuple of admissible ones (activations: fp32 or the bf16 twins)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise ValueError(f"{name}: must live on the GPU (got device {t.device}); groupnet_amd has no CPU path")
    if (t.dtype not in dtype) if isinstance(dtype, tuple) else (t.dtype != dtype):
        want = " or ".join(str(d) for d in dtype) if isinstance(dtype, tuple) else str(dtype)
        raise ValueError(f"{name}: must be {want} (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None:
        if t.dim() != len(shape) or any(s is not None and int(d) != int(s) for d, s in zip(t.shape, shape)):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _counter_arg(counter: Optional[Tensor], name: str = "counter") -> Optional[Tensor]:
    """A Philox counter as the kernels take it — a 1-element int64 GPU tensor — or None, passed through."""
    if counter is not None and not (counter.is_cuda and counter.dtype == torch.int64 and counter.numel() == 1):
        raise ValueError(f"{name}: a 1-element int64 GPU tensor")
    return counter


def _same_device(*ts: Tensor) -> None:
    dev = ts[0].device
    for t in ts[1:]:
        if t is not None and t.device != dev:
            raise ValueError(f"tensors on different devices: {dev} vs {t.device}")


# ---- optional instrumentation ----------------------------------------------------------------------
# bench.py brackets the launches of the matrix-core kernels with HIP events on the stream they are
# launched on (the roofline leg of the bench contract).  `launch_probe(name, flops, before)` is None in
# normal use and costs one comparison per launch.
launch_probe = None


# Matrix path of the fp32 entry points, chosen at import by GN_PRECISION (set_precision changes it later):
#   f16x3 (default): two fp16 parts per operand, three part-products per product, bf16x6 as the in-kernel fallback for
#                    operands beyond the fp16 range;
#   bf16x6: fp32-accurate products on the bf16 cores (three parts, six products);
#   fp32: the fp32 matrix cores.
_PRECISION = os.environ.get("GN_PRECISION", "f16x3").lower()
BF16X6 = _PRECISION != "fp32"      # fp32-accurate products on the 16-bit cores ...
F16X3 = _PRECISION not in ("bf16x6", "fp32")      # ... from fp16 parts


# the fused affinity + top-k launch as the tail workgroups of the first node stage (GN_AFFINITY_TAIL = 0: its own launch)
_AFFINITY_TAIL = os.environ.get("GN_AFFINITY_TAIL", "1") != "0"


# Form in which the stand-alone gather / scatter launches of the engine read a hyperedge incidence: "dense" (default) — the
# fp32 H (B,E,N) — or "mask" — 64-bit member words (`IncidenceMasks`), inference, 16 < N <= 64.  None: not set by
# `set_incidence_form`, the environment decides per call (GN_INC_MASKS=1: mask).
_INCIDENCE_FORM: Optional[str] = None


def incidence_form() -> str:
    """'dense' or 'mask': what `set_incidence_form` chose, else GN_INC_MASKS=1 selects 'mask' (A/B switch, read per
    call).  Results are bit-identical either way."""
    if _INCIDENCE_FORM is not None:
        return _INCIDENCE_FORM
    return "mask" if os.environ.get("GN_INC_MASKS", "0") == "1" else "dense"


def set_incidence_form(form: Optional[str]) -> None:
    """'dense' | 'mask' for launches issued from now on (captured graphs keep the form they were captured with); None
    hands the choice back to the environment."""
    global _INCIDENCE_FORM
    if form is not None:
        form = form.lower()
        if form not in ("dense", "mask"):
            raise ValueError("incidence form: 'dense' or 'mask'")
    _INCIDENCE_FORM = form


def precision() -> str:
    """Matrix path of the fp32 entry points: 'f16x3' (default), 'bf16x6' or 'fp32' (the fp32 matrix cores)."""
    return "f16x3" if (BF16X6 and F16X3) else ("bf16x6" if BF16X6 else "fp32")


def set_precision(mode: str) -> None:
    """Select the matrix path of the fp32 entry points for launches issued from now on: 'f16x3' | 'bf16x6' | 'fp32'.
    (Captured graphs keep the path they were captured with.)"""
    global BF16X6, F16X3
    mode = mode.lower()
    if mode not in ("f16x3", "bf16x6", "fp32"):
        raise ValueError("precision: 'f16x3', 'bf16x6' or 'fp32'")
    BF16X6 = mode != "fp32"
    F16X3 = mode == "f16x3"


def _twin(dtype: torch.dtype) -> bool:
    return dtype == torch.bfloat16


def _fn(stem: str, dtype: torch.dtype):
    """The C entry point of a stage for a storage type: `<stem>_f32` or its `<stem>_bf16` twin."""
    return getattr(load(), stem + ("_bf16" if _twin(dtype) else "_f32"))


def _ximg(pk: dict, name: str, dtype: torch.dtype) -> int:
    """Device address of image `name` for a launch on `dtype` activations, or 0 (fp32 entry point with the
    bf16-core path switched off: the launch then uses the plain packed stream on the fp32 matrix cores)."""
    xi = pk.get("xi")
    if _twin(dtype):
        if xi is None or name not in xi.src:
            raise ValueError(f"no bf16 image '{name}' for this weight set")
        return xi.get(name, 1).data_ptr()
    if not BF16X6 or xi is None or name not in xi.src:
        return 0
    return xi.get(name, 3).data_ptr()


def _himg(pk: dict, name: str, dtype: torch.dtype) -> int:
    """Device address of the two-part fp16 image `name` (f16x3 path of the fp32 entry points), or 0."""
    xi = pk.get("xi")
    if _twin(dtype) or not (BF16X6 and F16X3) or xi is None or name not in xi.src:
        return 0
    return xi.get(name, 2).data_ptr()


class _Probed:
    """flops: the EXECUTED fp32-equivalent count of the launch, or (executed, reference form) where a stage runs an
    algebraically reduced form (typed aggregation: the reference form is every ordered edge through both layers,
    SURVEY.md 8d)."""
    __slots__ = ("name", "flops", "probe")

    def __init__(self, name: str, flops):
        self.name, self.flops, self.probe = name, flops, launch_probe

    def __enter__(self):
        if self.probe is not None:
            self.probe(self.name, self.flops, True)

    def __exit__(self, *exc):
        if self.probe is not None:
            self.probe(self.name, self.flops, False)
        return False


# ---- ragged batches ----------------------------------------------------------------------------
class AgentCounts:
    """The per-scene agent counts of a ragged batch ("Ragged batches"), validated: ``counts`` — the B
    ints on the host, ``N`` — the padded size, ``dev`` — the counts as a (B,) int32 tensor on ``device``, uploaded once,
    when the first launch asks for it (a forward that refuses the call has then copied nothing).  Made by
    `agent_counts`; every ``n_agents=`` argument of this module takes one (or what `agent_counts` takes)."""
    __slots__ = ("counts", "N", "device", "_dev")
    admits_empty = False        # every count is >= 1 (`StaticAgentCounts`: a count of 0, an empty slot, may occur)

    def __init__(self, counts: Tuple[int, ...], N: int, device):
        self.counts, self.N, self.device, self._dev = counts, N, torch.device(device), None

    @property
    def B(self) -> int:
        return len(self.counts)

    @property
    def dev(self) -> Tensor:
        if self._dev is None:
            self._dev = torch.tensor(self.counts, dtype=torch.int32).to(self.device, non_blocking=True)
        return self._dev


def count_values(n_agents, B: int, N: int, lowest: int = 1) -> List[int]:
    """The host validation of ``n_agents`` — a sequence of ints or a CPU integer tensor, one count per scene,
    ``lowest`` <= n_b <= N — as a list of B ints, or ValueError.  Pure: no device is asked.  ``lowest`` is 1 for a
    call's ``n_agents=`` and 0 for `StaticAgentCounts.set`, whose batches may hold empty slots."""
    if isinstance(n_agents, torch.Tensor):
        if n_agents.is_cuda:
            raise ValueError("n_agents: a sequence of ints or a CPU integer tensor (a GPU tensor would have to be read "
                             "back: a hidden synchronisation)")
        if n_agents.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or n_agents.dim() != 1:
            raise ValueError("n_agents: a 1-D integer tensor")
        vals = n_agents.tolist()
    else:
        try:
            vals = list(n_agents)
        except TypeError:
            raise ValueError("n_agents: a sequence of ints or a CPU integer tensor") from None
        if any(isinstance(v, bool) or not isinstance(v, int) for v in vals):
            raise ValueError("n_agents: every count must be an int")
    if len(vals) != B:
        raise ValueError(f"n_agents: {B} counts needed (one per scene), got {len(vals)}")
    if any(not lowest <= v <= N for v in vals):
        raise ValueError(f"n_agents: every count must lie in {lowest}..{N} (the padded size)")
    return vals


def agent_counts(n_agents, B: int, N: int, device) -> Optional[AgentCounts]:
    """``n_agents`` — a sequence of ints or a CPU integer tensor, one count per scene, 1 <= n_b <= N — as an
    `AgentCounts` on ``device``, or None when no scene is padded (every count equals N, or ``n_agents`` is None): the
    caller then takes the full-batch path and gets its bits.  A GPU tensor is refused: reading it would synchronise.
    An `AgentCounts` (a `StaticAgentCounts` included) passes through and keeps the ragged route whatever it holds."""
    if n_agents is None:
        return None
    if isinstance(n_agents, AgentCounts):
        if n_agents.B != B or n_agents.N != N:
            raise ValueError(f"n_agents: counts of {n_agents.B} scenes padded to {n_agents.N}, "
                             f"the call has {B} scenes padded to {N}")
        return n_agents
    vals = count_values(n_agents, B, N)
    if all(v == N for v in vals):
        return None
    if torch.device(device).type != "cuda":
        raise ValueError("n_agents: the counts go with GPU tensors; groupnet_amd has no CPU path")
    return AgentCounts(tuple(vals), N, device)


class StaticAgentCounts(AgentCounts):
    """Counts that live in ONE (B,) int32 device buffer for the holder's whole life, with replaceable values: what a
    captured graph needs (`graphs.GraphedMultiScale(ragged=True)`), since a hipGraph captures the buffer's address.
    Accepted wherever an `AgentCounts` is, and — as every `AgentCounts` instance — it keeps the ragged route even when
    every count is N.  A count of 0 is admitted: an EMPTY SLOT, whose outputs are all zeros.  The buffer
    starts filled with N.

    ``set(counts)`` validates on the host (`count_values`, 0..N) and copies into the buffer asynchronously, ordered on
    the current stream.  No host synchronisation in steady state: the values are staged in a RING of ``slots`` pinned
    rows, each with an event recorded behind its copy.  A `set` takes the next row and first waits for that row's
    event — the copy issued ``slots`` calls ago, which has long run when a replay follows every `set`; the wait returns
    at once then and blocks only a host that runs more than ``slots`` copies ahead of the GPU.  Two `set`s in a row use
    two rows, so the second cannot overwrite what the first copy has yet to read.

    ``set_from_mask(valid)`` counts a (B,N) bool / uint8 GPU mask on the device (`counts_from_mask`) straight into the
    buffer and reads nothing back; what it finds is ORed into ``status`` (one sticky device word, `_lib.COUNTS_*`).

    The host does not know the values after `set_from_mask`, so ``counts`` raises: nothing on the ragged route may depend
    on the values (it needs ``B`` and ``N`` only)."""
    __slots__ = ("_B", "status", "_stage", "_events", "_next")
    admits_empty = True

    def __init__(self, B: int, N: int, device, slots: int = 4):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("n_agents: the counts go with GPU tensors; groupnet_amd has no CPU path")
        if B < 1 or N < 1 or slots < 1:
            raise ValueError("StaticAgentCounts: B, N and slots must be positive")
        self._B, self.N, self.device = int(B), int(N), device
        self._dev = torch.full((self._B,), self.N, dtype=torch.int32, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self._stage = torch.empty((slots, self._B), dtype=torch.int32).pin_memory()
        self._events = [None] * slots
        self._next = 0

    @property
    def B(self) -> int:
        return self._B

    @property
    def counts(self):
        raise RuntimeError("StaticAgentCounts.counts: the values live on the device only (use B and N)")

    @property
    def dev(self) -> Tensor:
        return self._dev

    def set(self, counts) -> None:
        vals = count_values(counts, self._B, self.N, lowest=0)
        i = self._next
        self._next = (i + 1) % len(self._events)
        if self._events[i] is not None:
            self._events[i].synchronize()       # the copy that last read this row: done long ago in steady state
        self._stage[i].copy_(torch.tensor(vals, dtype=torch.int32))
        with torch.cuda.device(self.device):
            self._dev.copy_(self._stage[i], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self.device))
        self._events[i] = ev

    def set_from_mask(self, valid: Tensor) -> None:
        counts_from_mask(_mask_arg(valid, self._B, self.N, self.device), out=self._dev, status=self.status)


def _mask_arg(valid, B: Optional[int], N: Optional[int], device=None) -> Tensor:
    """A validity mask as the counts kernel takes it: a contiguous (B,N) bool or uint8 GPU tensor (checked on the host,
    before anything is launched)."""
    if not isinstance(valid, torch.Tensor) or not valid.is_cuda:
        raise ValueError("agent_mask: a (B,N) torch.bool or torch.uint8 tensor on the GPU")
    if valid.dtype not in (torch.bool, torch.uint8) or valid.dim() != 2 or not valid.is_contiguous():
        raise ValueError(f"agent_mask: a contiguous (B,N) torch.bool or torch.uint8 tensor (got {valid.dtype}, "
                         f"{tuple(valid.shape)})")
    if (B is not None and valid.shape[0] != B) or (N is not None and valid.shape[1] != N) or valid.numel() == 0:
        raise ValueError(f"agent_mask: expected shape ({B}, {N}), got {tuple(valid.shape)}")
    if device is not None and valid.device != torch.device(device):
        raise ValueError(f"tensors on different devices: {device} vs {valid.device}")
    return valid


def counts_from_mask(valid: Tensor, out: Optional[Tensor] = None, status: Optional[Tensor] = None
                     ) -> Tuple[Tensor, Tensor]:
    """Agent counts of a (B,N) bool / uint8 GPU validity mask, on the device (gn_agent_counts_u8): out[b] = the length
    of the LEADING run of valid agents of scene b -> (out (B,) int32, status (1,) int32).  ``status`` is sticky — the
    launch only ORs into it: `_lib.COUNTS_NOT_PREFIX` when some scene has a valid agent behind an invalid one (those are
    not counted), `_lib.COUNTS_EMPTY` when some scene has none.  Nothing is read back; given ``out`` / ``status`` are
    written in place (a fresh ``status`` starts at 0)."""
    _mask_arg(valid, None, None)
    B, N = valid.shape
    if out is None:
        out = torch.empty((B,), dtype=torch.int32, device=valid.device)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=valid.device)
    _req(out, "out", (B,), torch.int32)
    _req(status, "status", (1,), torch.int32)
    _same_device(valid, out, status)
    with torch.cuda.device(valid.device):
        check(load().gn_agent_counts_u8(addr(valid), B, N, addr(out), addr(status), stream_handle()), "gn_agent_counts_u8")
    return out, status


ZERO_NODE_ROWS, ZERO_EDGE_ROWS, ZERO_PAIR_ROWS = _lib.ZERO_NODE_ROWS, _lib.ZERO_EDGE_ROWS, _lib.ZERO_PAIR_ROWS
ZERO_SYM_PAIR_ROWS = _lib.ZERO_SYM_PAIR_ROWS


def _zero_launch(who: str, hint: str, items, n_agents, rows: Optional[int], layout) -> None:
    """What `zero_padding` and `zero_empty_scenes` (``who``: the caller, and gn_<who> its launcher) do alike: check
    ``items`` = [(tensor, kind)], build their `_lib.ZeroItem` array and launch it, unless nothing is left to zero.  The
    admissible shapes are (B, ``rows``, width); ``rows`` None: any row count, and the launcher takes N as well.
    ``layout(t, kind)`` is the caller's rows-per-scene rule: (pitch, width) of a row in elements, None for a tensor to
    skip, ValueError for one it refuses."""
    if not isinstance(n_agents, AgentCounts):
        raise ValueError(f"{who}: n_agents must be an ops.AgentCounts{hint}")
    arr = []
    for t, kind in items:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 3 and t.shape[0] == n_agents.B
                and rows in (None, t.shape[1])):
            raise ValueError(f"{who}: (B, {'rows' if rows is None else rows}, width) GPU tensors")
        if t.dtype not in _ACT_DTYPES:
            raise ValueError(f"{who}: fp32 or bf16 tensors (got {t.dtype})")
        row = layout(t, kind)
        if row is None:
            continue
        _same_device(n_agents.dev, t)
        arr.append(_lib.ZeroItem(ptr=t.data_ptr(), pitch=row[0] * t.element_size(), width=row[1] * t.element_size(),
                                 kind=kind))
    if not arr:
        return
    if len(arr) > _lib.MAX_ZERO_ITEMS:
        raise ValueError(f"{who}: at most {_lib.MAX_ZERO_ITEMS} tensors per launch")
    dims = (n_agents.B, n_agents.N) if rows is None else (n_agents.B,)
    with torch.cuda.device(n_agents.dev.device):
        check(getattr(load(), "gn_" + who)((_lib.ZeroItem * len(arr))(*arr), len(arr), *dims, addr(n_agents.dev),
                                           stream_handle()), "gn_" + who)


def zero_padding(items: Sequence[Tuple[Tensor, int]], n_agents) -> None:
    """Zero the padded positions of several tensors of a ragged batch in ONE launch (gn_zero_padding).  items =
    [(tensor, kind)]: ZERO_NODE_ROWS — (B,N,w), rows n >= n_b; ZERO_EDGE_ROWS — the (B,N,w) hyperedge rows of a top-k
    module, rows e >= n_b (the (B,1,w) rows of a scale-N module are valid: they are skipped here); ZERO_PAIR_ROWS —
    (B,N*N,w) ordered pair rows with an end >= n_b, or a contiguous (B,N,N) matrix per scene (corr, H, new_H);
    ZERO_SYM_PAIR_ROWS — (B,N(N+1)/2,w) unordered pair rows (`pair_count`, row-major over i <= j) with an end >= n_b.  A
    tensor may be a last-dim slice of a wider contiguous one; fp32 or bf16 (rows of an even number of bytes)."""
    def layout(t, kind):
        N, R, w = n_agents.N, t.shape[1], t.shape[2]
        if kind == ZERO_PAIR_ROWS and (R, w) == (N, N) and t.is_contiguous():
            R, w, pitch = N * N, 1, 1          # a matrix per scene: one element per ordered pair
        else:
            if t.stride(2) != 1 or t.stride(0) != R * t.stride(1):
                raise ValueError("zero_padding: a contiguous tensor or a last-dim slice of one")
            pitch = t.stride(1)
        if kind == ZERO_EDGE_ROWS and R == 1:
            return None
        rows = {ZERO_NODE_ROWS: N, ZERO_EDGE_ROWS: N, ZERO_PAIR_ROWS: N * N, ZERO_SYM_PAIR_ROWS: pair_count(N)}
        if R != rows.get(kind):
            raise ValueError(f"zero_padding: kind {kind} does not go with {R} rows per scene at N = {N}")
        return pitch, w

    _zero_launch("zero_padding", " (ops.agent_counts)", items, n_agents, None, layout)


def zero_empty_scenes(items: Sequence[Tensor], n_agents) -> None:
    """Zero, in ONE launch, every scene with count 0 of the single-row tensors that `zero_padding` skips — the (B,1,w)
    factor rows of scale-N modules, which reach an empty slot's row through row-wise stages (gn_zero_empty_scenes).  For
    holders that admit a count of 0 (`StaticAgentCounts`); scenes with a count >= 1 keep their bits.  fp32 or bf16,
    contiguous or a last-dim slice of a contiguous tensor."""
    def layout(t, kind):
        if t.stride(2) != 1 or t.stride(0) < t.shape[2]:
            raise ValueError("zero_empty_scenes: a contiguous tensor or a last-dim slice of one")
        return t.stride(0), t.shape[2]

    _zero_launch("zero_empty_scenes", "", [(t, ZERO_EDGE_ROWS) for t in items], n_agents, 1, layout)


# ---- agents missing anywhere: the subset of a mask with holes ------------------------------------------------------
REMAP_NODE_ROWS, REMAP_PAIR_ROWS = _lib.REMAP_NODE_ROWS, _lib.REMAP_PAIR_ROWS


class _CompactedCounts(AgentCounts):
    """The counts of an `AgentSubset` as plain counts: what a forward hands to the ragged route once it has compacted
    its inputs (the route then runs exactly as with ``n_agents=<counts>``)."""
    __slots__ = ("_of",)

    def __init__(self, of: "AgentSubset"):
        self._of, self.N, self.device, self._dev = of, of.N, of.device, None

    admits_empty = property(lambda self: self._of.admits_empty)
    counts = property(lambda self: self._of.counts)
    B = property(lambda self: self._of.B)
    dev = property(lambda self: self._of.dev)


class AgentSubset(AgentCounts):
    """The valid agents of a batch whose scenes have agents missing ANYWHERE ("Agents missing
    anywhere"), made by `agent_subset`.  As an `AgentCounts` its counts are those of the COMPACTED tensors — valid rows
    first, in order — so every stage of this module takes it as the counts it is; the three forwards read the two maps
    besides: ``order`` (B,N) int32 — the slot of the r-th valid agent, -1 behind the last — and ``slot`` (B,N) int32 — the
    rank of a slot among the valid ones, -1 where it is invalid.  Both come from the device kernel
    (gn_agent_subset_u8), launched when the first launch asks for them: a forward that refuses the call has uploaded
    and launched nothing.  ``compacted``: the counts alone (what the ragged route is handed behind the compaction).
    Built from a GPU mask the values live on the device only: ``counts`` raises, ``admits_empty`` holds and ``status``
    is the sticky word of the kernel (`_lib.COUNTS_EMPTY` only)."""
    __slots__ = ("_B", "_counts", "_host", "_order", "_slot", "status", "_plain")

    def __init__(self, B: int, N: int, device, counts: Optional[Tuple[int, ...]] = None, host_mask: Optional[Tensor] = None):
        self._B, self.N, self.device = int(B), int(N), torch.device(device)
        self._counts, self._host = counts, host_mask
        self._dev = self._order = self._slot = self.status = self._plain = None

    @property
    def admits_empty(self) -> bool:
        return self._counts is None

    @property
    def B(self) -> int:
        return self._B

    @property
    def counts(self):
        if self._counts is None:
            raise RuntimeError("AgentSubset.counts: built from a GPU mask, the values live on the device only")
        return self._counts

    def _alloc(self, device) -> None:
        self._dev = torch.empty((self._B,), dtype=torch.int32, device=device)
        self._order = torch.empty((self._B, self.N), dtype=torch.int32, device=device)
        self._slot = torch.empty((self._B, self.N), dtype=torch.int32, device=device)
        if self.status is None:
            self.status = torch.zeros(1, dtype=torch.int32, device=device)

    def _launch(self, valid: Tensor) -> None:
        """gn_agent_subset_u8 of a (B,N) GPU mask into the holder's buffers."""
        with torch.cuda.device(valid.device):
            check(load().gn_agent_subset_u8(addr(valid), self._B, self.N, addr(self._dev), addr(self._order),
                                            addr(self._slot), addr(self.status), stream_handle()), "gn_agent_subset_u8")

    def _built(self) -> "AgentSubset":
        if self._dev is None:      # a host mask: its bytes are uploaded now, the device kernel builds the maps
            valid = self._host.to(self.device, non_blocking=True)
            self._alloc(valid.device)
            self._launch(valid)
        return self

    @property
    def dev(self) -> Tensor:
        return self._built()._dev

    @property
    def order(self) -> Tensor:
        return self._built()._order

    @property
    def slot(self) -> Tensor:
        return self._built()._slot

    @property
    def compacted(self) -> AgentCounts:
        if self._plain is None:
            self._plain = _CompactedCounts(self)
        return self._plain


def _host_mask(valid) -> Tensor:
    """A host validity mask — a CPU bool / uint8 tensor, a numpy array of those types or a nested sequence of bools /
    ints — as a contiguous (B,N) uint8 CPU tensor of 0 / 1, or ValueError."""
    if isinstance(valid, torch.Tensor):
        t = valid
    else:
        try:
            t = torch.as_tensor(valid)
        except Exception:
            raise ValueError("agent_subset: a (B,N) bool / uint8 mask (tensor, numpy array or nested sequence)") from None
        if not isinstance(valid, (list, tuple)) and t.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"agent_subset: a bool or uint8 mask (got {t.dtype})")
        if t.dtype in (torch.int8, torch.int16, torch.int32, torch.int64):      # a nested sequence of ints
            t = t != 0
    if t.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"agent_subset: a bool or uint8 mask (got {t.dtype})")
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"agent_subset: a (B,N) mask with B, N >= 1 (got shape {tuple(t.shape)})")
    return (t != 0).to(torch.uint8).contiguous()


def agent_subset(valid, device=None) -> Optional[AgentCounts]:
    """The valid agents of a batch from a (B,N) validity mask (non-zero = valid) with zeros ANYWHERE, as what the
    forwards' ``n_agents=`` takes.
    A HOST mask (CPU bool / uint8 tensor, numpy array, nested sequence) is validated here — every scene needs a valid
    agent, else ValueError — and gives None when everything is valid (the call takes the full-batch path), a plain
    `AgentCounts` when every scene's mask is a prefix (the ``n_agents=`` call and its bits), else an `AgentSubset` with
    host-known counts on ``device`` (default: the current GPU).  Nothing is uploaded or launched yet.
    A GPU mask (contiguous bool / uint8) gives an `AgentSubset` whose values live on the device only: the kernel is
    launched here, nothing is read back, empty scenes are admitted (their outputs are zeros, ``status`` says so) and the
    holder is inference-only."""
    if isinstance(valid, torch.Tensor) and valid.is_cuda:
        _mask_arg(valid, None, None, device)
        sub = AgentSubset(valid.shape[0], valid.shape[1], valid.device)
        sub._alloc(valid.device)
        sub._launch(valid)
        return sub
    m = _host_mask(valid)
    B, N = m.shape
    counts = tuple(int(c) for c in m.sum(dim=1).tolist())
    if min(counts) < 1:
        raise ValueError("agent_subset: every scene needs at least one valid agent")
    if all(c == N for c in counts):
        return None
    device = torch.device("cuda" if device is None else device)
    if device.type != "cuda":
        raise ValueError("agent_subset: the subset goes with GPU tensors; groupnet_amd has no CPU path")
    if all(bool(m[b, :c].all()) for b, c in enumerate(counts)):
        return AgentCounts(counts, N, device)
    return AgentSubset(B, N, device, counts=counts, host_mask=m)


class StaticAgentSubset(AgentSubset):
    """An `AgentSubset` whose counts, ``order`` and ``slot`` live at FIXED device addresses for the holder's whole life,
    with replaceable values: what `graphs.GraphedMultiScale(ragged="subset")` captures.  It starts with every agent
    valid.  ``set_from_mask(valid)`` runs gn_agent_subset_u8 of a (B,N) bool / uint8 GPU mask into the buffers — holes
    are honoured, nothing is read back, an empty scene is ORed into ``status``.  ``set(counts)`` sets prefix counts
    (0..N, validated on the host) through the staging ring of `StaticAgentCounts`, and the prefix order with them."""
    __slots__ = ("_ring",)

    def __init__(self, B: int, N: int, device, slots: int = 4):
        super().__init__(B, N, device)
        self._ring = StaticAgentCounts(B, N, device, slots)
        self._alloc(self._ring.device)
        self._dev = self._ring.dev
        self._prefix_maps()

    def _prefix_maps(self) -> None:
        ar = torch.arange(self.N, dtype=torch.int32, device=self._dev.device).expand(self._B, self.N)
        pref = torch.where(ar < self._dev[:, None], ar, torch.full_like(ar, -1))
        self._order.copy_(pref)
        self._slot.copy_(pref)

    def set(self, counts) -> None:
        self._ring.set(counts)
        with torch.cuda.device(self._dev.device):
            self._prefix_maps()

    def set_from_mask(self, valid: Tensor) -> None:
        self._launch(_mask_arg(valid, self._B, self.N, self._dev.device))


def _remap_layout(t: Tensor, kind: int, B: int, N: int):
    """(scene stride, row pitch, row width) in elements of a tensor of `remap_rows`, or ValueError."""
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 3 and t.shape[0] == B):
        raise ValueError("remap_rows: (B, rows, width) GPU tensors")
    if t.dtype not in _ACT_DTYPES:
        raise ValueError(f"remap_rows: fp32 or bf16 tensors (got {t.dtype})")
    R, w = t.shape[1], t.shape[2]
    if any(s < 0 for s in t.stride()) or (w > 1 and t.stride(2) != 1):
        raise ValueError("remap_rows: a contiguous tensor, a last-dim slice or a row block of one")
    if kind == REMAP_PAIR_ROWS and (R, w) == (N, N) and (N == 1 or t.stride(1) == N):
        return t.stride(0), 1, 1             # a matrix per scene: one element per ordered pair
    if R != (N * N if kind == REMAP_PAIR_ROWS else N) or kind not in (REMAP_NODE_ROWS, REMAP_PAIR_ROWS):
        raise ValueError(f"remap_rows: kind {kind} does not go with {R} rows per scene at N = {N}")
    if R > 1 and t.stride(1) < w:
        raise ValueError("remap_rows: a contiguous tensor, a last-dim slice or a row block of one")
    return t.stride(0), max(t.stride(1), w), w


def remap_rows(items: Sequence[Tuple[Tensor, Tensor, int]], map: Tensor) -> None:
    """Move the rows of several tensors through a per-scene index map in ONE launch (gn_remap_rows): items =
    [(src, dst, kind)], ``map`` (B,N) int32 — `AgentSubset.order` compacts (valid rows first, zeros behind), `.slot`
    expands (results back at their slots, zeros elsewhere).  REMAP_NODE_ROWS — (B,N,w), destination row r from source
    row map[b,r]; REMAP_PAIR_ROWS — (B,N*N,w) ordered pair rows, or a (B,N,N) matrix per scene (corr, H, a scale block of
    new_H).  ``src`` and ``dst`` have one shape and dtype (fp32 or bf16) and must not overlap; each is contiguous, a
    last-dim slice or a row block of a contiguous tensor (the (B,1,N) row of a scale-N module's H goes as the node kind
    on its (B,N,1) view).  Every destination position is written: unmapped ones as zeros.  A launch takes
    `_lib.MAX_ZERO_ITEMS` tensors; a longer list goes in further launches."""
    _req(map, "map", (None, None), torch.int32)
    B, N = map.shape
    arr = []
    for src, dst, kind in items:
        ls, ld = _remap_layout(src, kind, B, N), _remap_layout(dst, kind, B, N)
        if src.shape != dst.shape or src.dtype != dst.dtype or ls[2] != ld[2]:
            raise ValueError("remap_rows: source and destination of one shape and dtype")
        _same_device(map, src, dst)
        es = src.element_size()
        arr.append(_lib.RemapItem(src=src.data_ptr(), dst=dst.data_ptr(), src_scene=ls[0] * es, dst_scene=ld[0] * es,
                                  src_pitch=ls[1] * es, dst_pitch=ld[1] * es, width=ls[2] * es, kind=kind))
    if not arr or B == 0 or N == 0:
        return
    with torch.cuda.device(map.device):
        for i in range(0, len(arr), _lib.MAX_ZERO_ITEMS):      # (more tensors than a launch's table holds: further launches)
            part = arr[i:i + _lib.MAX_ZERO_ITEMS]
            check(load().gn_remap_rows((_lib.RemapItem * len(part))(*part), len(part), B, N, addr(map), stream_handle()),
                  "gn_remap_rows")


# ---- A0 / A1 -----------------------------------------------------------------------------------
def affinity(f: Tensor) -> Tensor:
    """corr = normalize(f) @ normalize(f)^T   (model/GroupNet_nba.py:284-286)."""
    _req(f, "f", (None, None, None))
    B, N, D = f.shape
    corr = torch.empty((B, N, N), dtype=f.dtype, device=f.device)
    with torch.cuda.device(f.device):
        check(load().gn_affinity_f32(addr(f), addr(corr), B, N, D, stream_handle()), "gn_affinity_f32")
    return corr


def _alloc_incidence(B: int, N: int, scales: Sequence[int], device) -> List[Tensor]:
    out = []
    for s in scales:
        s = int(s)
        if s > N:
            raise RuntimeError("selected index k out of range")  # what torch.topk raises (MS_HGNN_batch.py:382)
        E = 1 if s == N else N
        out.append(torch.empty((B, E, N), dtype=torch.float32, device=device))
    return out


def _scale_args(Hs: List[Tensor], scales: Sequence[int]):
    n = len(Hs)
    Hl = (_P * n)(*[h.data_ptr() for h in Hs])
    kl = (ctypes.c_int * n)(*[int(s) for s in scales])
    return Hl, kl, n


def topk_incidence(corr: Tensor, scales: Sequence[int], n_agents=None) -> List[Tensor]:
    """H per scale from corr (MS_HGNN_hyper.init_adj_attention, model/MS_HGNN_batch.py:372-388).  ``n_agents`` (ragged
    batch, `agent_counts`): row i < n_b holds the top-min(scale, n_b) of corr[b, i, :n_b], everything else is zeros and a
    scale-N hyperedge holds the n_b valid agents (gn_topk_incidence_ragged_f32)."""
    _req(corr, "corr", (None, None, None))
    B, N, N2 = corr.shape
    if N != N2:
        raise ValueError(f"corr: expected (B,N,N), got {tuple(corr.shape)}")
    if not 1 <= len(scales) <= 8:
        raise ValueError("between 1 and 8 scales per call")
    counts = agent_counts(n_agents, B, N, corr.device)
    Hs = _alloc_incidence(B, N, scales, corr.device)
    Hl, kl, n = _scale_args(Hs, scales)
    with torch.cuda.device(corr.device):
        if counts is not None:
            _same_device(corr, counts.dev)
            check(load().gn_topk_incidence_ragged_f32(addr(corr), Hl, kl, n, B, N, addr(counts.dev), stream_handle()),
                  "gn_topk_incidence_ragged_f32")
        else:
            check(load().gn_topk_incidence_f32(addr(corr), Hl, kl, n, B, N, stream_handle()), "gn_topk_incidence_f32")
    return Hs


def listall_incidence(corr: Tensor, scale: int) -> Tensor:
    """H of MS_HGNN_hyper.init_adj_attention_listall (model/MS_HGNN_batch.py:390-414): (B,1,N) of ones when
    scale == N, else (B,N,N) with row i = the best group of max(scale,1) agents containing i (exhaustive
    search over C(N-1, scale-1) candidates, first maximum in torch.combinations order)."""
    _req(corr, "corr", (None, None, None))
    B, N, N2 = corr.shape
    if N != N2:
        raise ValueError("corr must be (B, N, N)")
    scale = int(scale)
    if scale > N:
        raise RuntimeError("group size larger than the number of agents")   # the reference cannot build its table either
    H = torch.empty((B, 1 if scale == N else N, N), dtype=corr.dtype, device=corr.device)
    if B == 0:
        return H
    with torch.cuda.device(corr.device):
        check(load().gn_listall_incidence_f32(addr(corr), addr(H), B, N, scale, stream_handle()),
              "gn_listall_incidence_f32")
    return H


class IncidenceMasks:
    """Bit-mask form of a 0/1 incidence H (B,E,N), N <= 64 (hence E <= 64), as int64 tensors: bit n of ``row[b,e]`` and bit
    e of ``col[b,n]`` are set iff H[b,e,n] != 0 (include/groupnet_hip.h).  Made by `incidence_masks`,
    `affinity_topk(want_masks=True)` or `AffinityTail(want_masks=True)`; consumed by `agg_gather*` (row) and
    `agg_scatter*` (col)."""
    __slots__ = ("row", "col")

    def __init__(self, row: Tensor, col: Tensor):
        _req(row, "row", (None, None), torch.int64)
        _req(col, "col", (row.shape[0], None), torch.int64)
        _same_device(row, col)
        if row.shape[1] > MASK_MAX_N or col.shape[1] > MASK_MAX_N:
            raise ValueError(f"IncidenceMasks: at most {MASK_MAX_N} hyperedges and nodes")
        self.row, self.col = row, col


class Incidence:
    """The graph a hyper module passes messages on, in both forms: the dense ``H`` (B,E,N) and, optionally, the
    `IncidenceMasks` of that same H.  An entry of `run_message_passing`'s ``Hs`` (a plain tensor there is an `Incidence`
    without masks, None the implicit pairwise graph)."""
    __slots__ = ("H", "masks")

    def __init__(self, H: Tensor, masks: Optional[IncidenceMasks] = None):
        if not isinstance(H, torch.Tensor) or H.dim() != 3:
            raise ValueError("H: expected a (B,E,N) tensor")
        if masks is not None:
            if not isinstance(masks, IncidenceMasks):
                raise ValueError("masks: expected an ops.IncidenceMasks")
            B, E, N = H.shape
            _req(masks.row, "masks.row", (B, E), torch.int64)
            _req(masks.col, "masks.col", (B, N), torch.int64)
            _same_device(H, masks.row)
        self.H, self.masks = H, masks


def _alloc_masks(B: int, E: int, N: int, device) -> IncidenceMasks:
    if N > MASK_MAX_N or E > MASK_MAX_N:
        raise ValueError(f"the bit-mask form of an incidence needs N <= {MASK_MAX_N} and E <= {MASK_MAX_N}")
    return IncidenceMasks(torch.empty((B, E), dtype=torch.int64, device=device),
                          torch.empty((B, N), dtype=torch.int64, device=device))


def incidence_masks(H: Tensor, assume_binary: bool = False) -> IncidenceMasks:
    """The bit-mask form of a dense fp32 H (B,E,N), E, N <= 64 (gn_incidence_masks_f32).  Without ``assume_binary`` the
    launch also checks that H holds only 0 and 1 and the flag is read back — ONE HOST SYNCHRONISATION, not capturable in
    a graph — raising ValueError otherwise (such an H keeps the dense form).  Pass ``assume_binary=True`` for an H the
    library built itself."""
    _req(H, "H", (None, None, None))
    B, E, N = H.shape
    m = _alloc_masks(B, E, N, H.device)
    if B == 0:
        return m
    flag = None if assume_binary else torch.empty((1,), dtype=torch.int32, device=H.device)
    with torch.cuda.device(H.device):
        check(load().gn_incidence_masks_f32(addr(H), B, E, N, addr(m.row), addr(m.col), addr(flag), stream_handle()),
              "gn_incidence_masks_f32")
    if flag is not None and int(flag.item()) != 0:
        raise ValueError("incidence_masks: H holds entries other than 0 and 1; it has no bit-mask form")
    return m


@functools.lru_cache(maxsize=None)
def graph_form(N: int, D: int, x_dim: int = 0, mask_scales: int = 0) -> str:
    """Which launches build the graph of scenes of N agents with D features (``x_dim`` raw inputs per agent with the
    embedding front-end; ``mask_scales`` > 0: the launch also emits the bit-mask form of that many scales):
      "tail"   — the fused affinity + top-k job rides as tail workgroups of the first node-stage launch,
      "fused"  — it is a launch of its own (gn_affinity_topk_*),
      "banded" — its scene tile does not fit: gn_affinity_f32 (banded there) + gn_topk_incidence_f32.
    The library alone answers, from two plan queries with placeholder addresses (nothing is launched, no GPU is asked):
    the tile rule and both budgets are stated in C only.  Memoised: an eager forward asks once per shape."""
    P = _PLACEHOLDER      # a plan query tests addresses, it never reads through them
    n = max(1, mask_scales)
    Hl, kl = (_P * n)(*[P] * n), (ctypes.c_int * n)(*[1] * n)
    ex = _lib.BlockExtras(x_raw=P, x_dim=x_dim, M=P, c=P, f_contig=P) if x_dim else _lib.BlockExtras()
    words = (_P * n)(*[P] * n) if mask_scales else None
    plan = _lib.LaunchPlan()
    rc = load().gn_affinity_topk_plan_f32(P, None, Hl, kl, n, 1, N, D, ctypes.byref(ex), words, words, ctypes.byref(plan))
    if rc == _lib.GN_ERR_LDS:
        return "banded"
    check(rc, "gn_affinity_topk_plan")
    if mask_scales:
        return "fused"        # only the stand-alone launch emits masks
    g = (_lib.NodeGroup * 1)(_lib.NodeGroup(x=P, Wx=P, bias=P, xp=P, pq=P))
    job = _lib.AffinityJob(f=P, H_list=Hl, k_list=kl, n_scales=n, B=1, N=N, D=D, extras=ctypes.pointer(ex))
    rc = load().gn_node_mlp_plan_f32(g, 1, N, ctypes.byref(job), ctypes.byref(plan))
    return "tail" if rc == _lib.GN_OK else "fused"


def affinity_topk(f: Optional[Tensor], scales: Sequence[int], want_corr: bool = True, f_out: Optional[Tensor] = None,
                  want_H_cat: bool = False, counter: Optional[Tensor] = None, counter_add: int = 0,
                  embed: Optional[Tuple[Tensor, Tensor, Tensor]] = None, want_masks: bool = False, n_agents=None):
    """Fused A0+A1: f -> (corr, [H_s], H_cat) in one launch.  ``want_masks`` (N <= 64): the launch also writes the
    bit-mask form of every H_s; the LAST return value then is the list of `IncidenceMasks`, one per scale.

    Extras for the multiscale block (no copy kernels after this launch): ``f_out`` — a last-dim slice
    (B, N, D) of a wider contiguous tensor that also receives f; ``want_H_cat`` — also build
    cat(H_s, dim=1); ``counter``/``counter_add`` — advance the device Philox position.
    ``embed`` = (x_raw (B,N,xd), M (D,xd), c (N,D)): f itself is computed in the launch as M x + c[n]
    (pass f=None, fp32 only); a fourth return value then carries f (B,N,D).
    ``n_agents`` (ragged batch, `agent_counts`): the incidences and corr of scenes with n_b <= N agents each
    (gn_affinity_topk_ragged_*: valid blocks as each scene alone, zeros elsewhere); not with ``embed`` or ``want_masks``."""
    job = AffinityTail(f, scales, want_corr, f_out, want_H_cat, counter, counter_add, embed, want_masks, n_agents)
    job.launch()
    return (job.corr, job.Hs, job.H_cat) + ((job.f,) if embed is not None else ()) + ((job.masks,) if want_masks else ())


class AffinityTail:
    """The fused affinity + top-k launch of a forward, DEFERRED: outputs are allocated now, the work is issued as the tail
    workgroups of the first node-stage launch (`node_stage_grouped(..., affinity=job)` -> gn_node_mlp_affinity_*), or —
    when nothing picks it up — by `launch()` as the stand-alone launch.  Same arguments as `affinity_topk`; the results
    are the attributes ``f``, ``corr``, ``Hs``, ``H_cat``, ``masks`` and ``incidences`` (one `Incidence` per scale: H_s with
    its masks, what `run_message_passing` takes after the pairwise module's None).
    ``want_masks``: also emit the bit-mask form of every H_s (``masks``: one `IncidenceMasks` per scale).  Only the
    stand-alone launch emits masks, so the job then declines the tail (`fits_tail()` is False).
    ``n_agents`` (ragged batch): the ragged launch, which is never the tail either and takes neither ``embed`` nor
    ``want_masks``."""

    def __init__(self, f: Optional[Tensor], scales: Sequence[int], want_corr: bool = False,
                 f_out: Optional[Tensor] = None, want_H_cat: bool = False, counter: Optional[Tensor] = None,
                 counter_add: int = 0, embed: Optional[Tuple[Tensor, Tensor, Tensor]] = None, want_masks: bool = False,
                 n_agents=None):
        ex = {}
        if n_agents is not None and (embed is not None or want_masks):
            raise ValueError("n_agents: the ragged launch has no embedding front-end and emits no masks")
        if embed is not None:
            x_raw, M, c = embed
            _req(x_raw, "x_raw", (None, None, None))
            B, N, xd = x_raw.shape
            _req(M, "M", (None, xd))
            D = M.shape[0]
            _req(c, "c", (N, D))
            _same_device(x_raw, M, c)
            f = torch.empty((B, N, D), dtype=x_raw.dtype, device=x_raw.device)   # the launch writes it (f_contig)
            ex.update(x_raw=x_raw.data_ptr(), x_dim=xd, M=M.data_ptr(), c=c.data_ptr(), f_contig=f.data_ptr())
        _req(f, "f", (None, None, None), _ACT_DTYPES)
        self.f, self.scales = f, [int(s) for s in scales]
        B, N, D = f.shape
        self.counts = agent_counts(n_agents, B, N, f.device)
        self.corr = torch.empty((B, N, N), dtype=torch.float32, device=f.device) if want_corr else None
        self.Hs = _alloc_incidence(B, N, self.scales, f.device)
        self._Hl, self._kl, n = _scale_args(self.Hs, self.scales)
        self.masks: Optional[List[IncidenceMasks]] = None
        self._rl = self._cl = None
        if want_masks:
            self.masks = [_alloc_masks(B, h.shape[1], N, f.device) for h in self.Hs]
            self._rl = (_P * n)(*[m.row.data_ptr() for m in self.masks])
            self._cl = (_P * n)(*[m.col.data_ptr() for m in self.masks])
        self.incidences = [Incidence(H, m) for H, m in zip(self.Hs, self.masks or [None] * n)]
        self.H_cat = None
        if f_out is not None:
            if not (f_out.is_cuda and f_out.dtype == f.dtype and tuple(f_out.shape) == (B, N, D)
                    and f_out.stride(2) == 1 and f_out.stride(0) == N * f_out.stride(1)):
                raise ValueError("f_out: a (B,N,D) last-dim slice of a contiguous GPU tensor of f's dtype")
            ex.update(f_out=f_out.data_ptr(), f_out_ld=f_out.stride(1))
        if want_H_cat:
            self.H_cat = torch.empty((B, sum(h.shape[1] for h in self.Hs), N), dtype=f.dtype, device=f.device)
            ex.update(H_cat=self.H_cat.data_ptr())
        if _counter_arg(counter) is not None:
            ex.update(counter=counter.data_ptr(), counter_add=int(counter_add) & (2**64 - 1))
        self._ex = _lib.BlockExtras(**ex)
        self._keep = (f_out, counter)
        self.job = _lib.AffinityJob(f=f.data_ptr(), corr=addr(self.corr), H_list=self._Hl, k_list=self._kl, n_scales=n,
                                    B=B, N=N, D=D, extras=ctypes.pointer(self._ex))
        self.done = False

    def fits_tail(self) -> bool:
        B, N, D = self.f.shape
        return self.masks is None and self.counts is None and graph_form(N, D, int(self._ex.x_dim)) == "tail"

    def launch(self) -> None:
        """The stand-alone launch (nothing took the job along)."""
        if self.done:
            return
        B, N, D = self.f.shape
        with torch.cuda.device(self.f.device):
            if self.counts is not None:
                _same_device(self.f, self.counts.dev)
                check(_fn("gn_affinity_topk_ragged", self.f.dtype)(
                    addr(self.f), addr(self.corr), self._Hl, self._kl, len(self.Hs), B, N, D, ctypes.byref(self._ex),
                    addr(self.counts.dev), stream_handle()), "gn_affinity_topk_ragged")
            else:
                check(_fn("gn_affinity_topk", self.f.dtype)(addr(self.f), addr(self.corr), self._Hl, self._kl, len(self.Hs), B, N, D,
                                                            ctypes.byref(self._ex), self._rl, self._cl, stream_handle()),
                      "gn_affinity_topk")
        self.done = True


# ---- A3 ------------------------------------------------------------------------------------------
def _groups(n: int) -> None:
    if not 1 <= n <= _lib.MAX_GROUPS:
        raise ValueError(f"1..{_lib.MAX_GROUPS} groups per launch, got {n}")


def node_stage_grouped(items: Sequence[Tuple[Tensor, dict]], keep: Optional[List[dict]] = None,
                       a_specs: Optional[Sequence[Optional[Tuple[dict, int]]]] = None,
                       affinity: Optional["AffinityTail"] = None
                       ) -> Tuple[List[Tuple[Tensor, Tensor]], List[Optional[Tensor]]]:
    """One launch for the node rows of several modules: items = [(x (B,N,64), pk{"W","bias","xi"})] with equal
    shapes -> [(x', pq)].  ``keep`` (training) receives per group {"hid": relu(W0 x + b0) (rows, 256)}.
    ``a_specs[g]`` = (agg_pk, K) asks for the per-node first layer of the typed aggregation MLP of the pairwise
    graph, A = W1cat x + b1/2 (B,N,K*128), from the SAME launch (bf16-core path of the fp32 entry point; with
    that path switched off it is a `node_linear` launch of its own); returned as the second list."""
    _groups(len(items))
    x0 = _req(items[0][0], "x", (None, None, FEAT), _ACT_DTYPES)
    dt = x0.dtype
    rows = x0.shape[0] * x0.shape[1]
    arr = (_lib.NodeGroup * len(items))()
    outs, As, late = [], [], []
    for g, (x, pk) in enumerate(items):
        _req(x, "x", tuple(x0.shape), dt)
        _same_device(x0, x)
        xp, pq = torch.empty_like(x), torch.empty_like(x)
        hid = None
        if keep is not None:
            if _twin(dt):
                raise ValueError("the bf16 twins are forward-only")
            hid = torch.empty((rows, 256), dtype=x.dtype, device=x.device)
            keep.append(dict(hid=hid))
        wx = _ximg(pk, "chain", dt)
        A, a_fields = None, {}
        spec = a_specs[g] if a_specs is not None else None
        if spec is not None:
            if _twin(dt):
                raise ValueError("the per-node first layer (pair form) belongs to the fp32 entry points")
            apk, K = spec
            if wx:
                A = torch.empty(tuple(x.shape[:-1]) + (K * 128,), dtype=x.dtype, device=x.device)
                a_fields = dict(WAx=_ximg(apk, "W1cat", dt), bA=apk["b1half"].data_ptr(), A=A.data_ptr(), KA=K,
                                WAh=_himg(apk, "W1cat", dt))
            else:
                late.append((g, x, apk, K))
        As.append(A)
        arr[g] = _lib.NodeGroup(x=x.data_ptr(), W=pk["W"].data_ptr(), bias=pk["bias"].data_ptr(), xp=xp.data_ptr(),
                                pq=pq.data_ptr(), hid_out=addr(hid), Wx=wx, Wh=_himg(pk, "chain", dt) if wx else 0,
                                **a_fields)
        outs.append((xp, pq))
    flops = sum(rows * 2 * (64 * 256 + 256 * 64 + 64 * 64 + (64 * 128 * int(a.KA) if a.A else 0)) for a in arr)
    # ``affinity``: a deferred fused affinity + top-k launch rides as this launch's tail workgroups (bf16-/fp16-core
    # kernels, a scene tile within the tail's LDS limit); otherwise it is issued on its own right here
    ride = (affinity is not None and not affinity.done and all(bool(a.Wx) for a in arr) and affinity.fits_tail()
            and affinity.f.dtype == dt and affinity.f.device == x0.device and _AFFINITY_TAIL)
    if affinity is not None and not ride:
        affinity.launch()
    with torch.cuda.device(x0.device), _Probed("node_stage_kernel", flops):
        if ride:
            check(_fn("gn_node_mlp_affinity", dt)(arr, len(items), rows, ctypes.byref(affinity.job), stream_handle()),
                  "gn_node_mlp_affinity")
            affinity.done = True
        else:
            check(_fn("gn_node_mlp", dt)(arr, len(items), rows, stream_handle()), "gn_node_mlp")
    for g, x, apk, K in late:
        As[g] = node_linear(x, apk["W1cat"], apk["b1half"], K * 128)
    return outs, As


def node_mlp(x: Tensor, pk: dict) -> Tuple[Tensor, Tensor]:
    """x (B,N,64) -> x' = MLP_{64->256->64}(x), pq = x' Wpq^T + bpq.  pk: {"W": stream, "bias": stream}."""
    return node_stage_grouped([(x, pk)])[0][0]


def pair_count(N: int) -> int:
    """Unordered pairs (i <= j) of N nodes — rows per scene of the symmetric pairwise form."""
    return N * (N + 1) // 2


def node2edge_grouped(items: Sequence[tuple], n_agents=None) -> List[Tensor]:
    """items = [(xp, pq, H or None, w2 (32,), b2 (1,)[, sym[, masks]])] over the same (B, N); returns [edges (B,E,64)].
    w2 / b2 = weight row and bias of attention layer 1, device tensors (the parameters themselves).
    H=None selects the implicit pairwise graph: E = N*N ordered edges, or with sym=True the
    N(N+1)/2 unordered pairs (edges (i,j) and (j,i) carry the same feature).
    ``masks`` (an `IncidenceMasks` of a 0/1 H, N <= 64; every hyper group of a call or none): where the launch takes its
    row form it reads the row words instead of H (gn_node2edge_masks_*); H stays in the item, the rows are the same.
    ``n_agents`` (ragged batch, `agent_counts`): every scene pools over its own n_b nodes (gn_node2edge_ragged_*): an H
    must have zero columns >= n_b (the ragged incidences do), pairwise edges with an end >= n_b come out as zeros; no
    masks."""
    _groups(len(items))
    xp0 = _req(items[0][0], "xp", (None, None, FEAT), _ACT_DTYPES)
    dt = xp0.dtype
    B, N, _ = xp0.shape
    counts = agent_counts(n_agents, B, N, xp0.device)
    arr = (_lib.N2EGroup * len(items))()
    outs, words = [], []
    for g, item in enumerate(items):
        xp, pq, H, w2, b2 = item[:5]
        sym = bool(item[5]) if len(item) > 5 else False
        masks = item[6] if len(item) > 6 else None
        _req(xp, "xp", (B, N, FEAT), dt)
        _req(pq, "pq", (B, N, FEAT), dt)
        if H is None:
            E = pair_count(N) if sym else N * N
        else:
            if sym:
                raise ValueError("sym applies to the pairwise graph (H=None) only")
            _req(H, "H", (B, None, N))
            E = H.shape[1]
        if masks is not None:
            if H is None:
                raise ValueError("masks apply to a hyper group (an explicit H) only")
            if not isinstance(masks, IncidenceMasks):
                raise ValueError("masks: expected an ops.IncidenceMasks")
            if counts is not None:
                raise ValueError("n_agents: the ragged node->edge launch reads the dense H, not masks")
            _req(masks.row, "masks.row", (B, E), torch.int64)
            words.append(masks.row)
        else:
            words.append(None)
        _req(w2, "w2", (32,))
        _req(b2, "b2", (1,))
        _same_device(xp0, xp, pq, H, w2, b2, words[-1])
        edges = torch.empty((B, E, FEAT), dtype=xp.dtype, device=xp.device)
        arr[g] = _lib.N2EGroup(xp=xp.data_ptr(), pq=pq.data_ptr(), H=addr(H), w2=w2.data_ptr(), edges=edges.data_ptr(),
                               b2=b2.data_ptr(), E=E, sym=int(sym))
        outs.append(edges)
    with torch.cuda.device(xp0.device):
        if counts is not None:
            _same_device(xp0, counts.dev)
            check(_fn("gn_node2edge_ragged", dt)(arr, len(items), B, N, addr(counts.dev), stream_handle()),
                  "gn_node2edge_ragged")
        elif any(w is not None for w in words):
            rows = (ctypes.c_void_p * len(items))(*[None if w is None else w.data_ptr() for w in words])
            check(_fn("gn_node2edge_masks", dt)(arr, rows, len(items), B, N, stream_handle()), "gn_node2edge_masks")
        else:
            check(_fn("gn_node2edge", dt)(arr, len(items), B, N, stream_handle()), "gn_node2edge")
    return outs


def node2edge(xp: Tensor, pq: Tensor, H: Optional[Tensor], w2: Tensor, b2: Tensor, sym: bool = False,
              masks: Optional["IncidenceMasks"] = None, n_agents=None) -> Tensor:
    return node2edge_grouped([(xp, pq, H, w2, b2, sym, masks)], n_agents)[0]


# ---- A4 ------------------------------------------------------------------------------------------
class PhiloxNoise:
    """Uniforms generated inside the edge kernel: element (row, k) of a (B,E,K) draw is element
    offset (+ device counter) + row*K + k of the Philox4x32-10 stream `seed`."""
    __slots__ = ("seed", "offset", "counter")

    def __init__(self, seed: int, offset: int = 0, counter: Optional[Tensor] = None):
        _counter_arg(counter)
        self.seed, self.offset, self.counter = int(seed) & (2**64 - 1), int(offset), counter


class PoolSpec:
    """Rows of the edge MLP to be formed inside its kernel instead of read from an `edges` tensor: the
    attention-weighted node -> edge pooling of `node2edge` (xp, pq (B,N,64) from the node stage; H (B,E,N) or None =
    the implicit pairwise graph, sym -> unordered pairs; w2 (32,), b2 (1,)).  bf16-core kernels only; H needs N <= 16
    (run_message_passing uses the hyper form only up to POOL_MAX_N)."""
    __slots__ = ("xp", "pq", "H", "w2", "b2", "sym")

    def __init__(self, xp: Tensor, pq: Tensor, H: Optional[Tensor], w2: Tensor, b2: Tensor, sym: bool = False):
        self.xp, self.pq, self.H, self.w2, self.b2, self.sym = xp, pq, H, w2, b2, bool(sym)


# Hyper modules: POOL_KERNEL_MAX_N is the largest N whose pooling the edge kernel may form itself (the kernel's bound is
# 16: a row's incidence stays in registers), so that an inference forward at N <= 16 has no node2edge launch.  The edge
# kernel stages a workgroup's scenes in LDS (pq, then x', through one buffer); groups that fit no stage (scale = N: one
# hyperedge per scene) pool from global memory with one live row block per workgroup ("Edge-kernel
# prologue").  POOL_MAX_N is the hyper modules' limit the engine hands to its route per call: all the kernel covers (the
# parity tests lower it to 0 to compare against the node2edge launch)
POOL_MAX_N = POOL_KERNEL_MAX_N


def edge_mlp_gumbel_grouped(items: Sequence[tuple], tau: float = 0.5, keep: Optional[List[dict]] = None
                            ) -> List[Tuple[Tensor, Optional[Tensor]]]:
    """items = [(edges (B,E,64) or PoolSpec, U tensor (B,E,K) or PhiloxNoise, pk, K[, sym_N[, want_dist]])];
    returns [(edge_feat, dist)].  All PhiloxNoise entries of one call must share seed and counter.

    sym_N = N > 0: `edges` holds the (B, N(N+1)/2, 64) unordered-pair rows of the pairwise graph; U /
    the Philox positions and `dist` are those of the ORDERED (B, N*N, K) tensor; edge_feat is
    (B, N(N+1)/2, K) = fac * (dist_ij + dist_ji).  want_dist=False skips the ordered dist output.
    ``keep`` (training) receives per group the activations the kernel otherwise holds in registers:
    {"z1" (rows,128), "z" (rows,64), "dh1" (rows,256), "lgf" (rows,32)}."""
    _groups(len(items))
    first = items[0][0]
    e0 = _req(first.xp if isinstance(first, PoolSpec) else first, "edges", (None, None, FEAT), _ACT_DTYPES)
    dt = e0.dtype
    arr = (_lib.EdgeGroup * len(items))()
    outs = []
    seed, ctr = None, None
    for g, item in enumerate(items):
        edges, U, pk, K = item[:4]
        sym_N = int(item[4]) if len(item) > 4 else 0
        want_dist = bool(item[5]) if len(item) > 5 else True
        pool = edges if isinstance(edges, PoolSpec) else None
        if pool is not None:
            if keep is not None or not BF16X6 and not _twin(dt):
                raise ValueError("PoolSpec: forward-only, bf16-core kernels only")
            _req(pool.xp, "xp", (None, None, FEAT), dt)
            B, Np, _ = pool.xp.shape
            _req(pool.pq, "pq", (B, Np, FEAT), dt)
            _req(pool.w2, "w2", (32,))
            _req(pool.b2, "b2", (1,))
            if pool.H is None:
                if bool(sym_N) != pool.sym or (sym_N and sym_N != Np):
                    raise ValueError("PoolSpec: sym must agree with sym_N = N")
                E = pair_count(Np) if pool.sym else Np * Np
            else:
                _req(pool.H, "H", (B, None, Np))
                if sym_N or Np > POOL_KERNEL_MAX_N:
                    raise ValueError(f"PoolSpec with H: a hyper module with N <= {POOL_KERNEL_MAX_N}")
                E = pool.H.shape[1]
            _same_device(e0, pool.xp, pool.pq, pool.H, pool.w2, pool.b2)
            edges = pool.xp              # (device / dtype of the outputs)
        else:
            _req(edges, "edges", (None, None, FEAT), dt)
            _same_device(e0, edges)
            B, E, _ = edges.shape
        if sym_N and E != pair_count(sym_N):
            raise ValueError(f"edges: symmetric form needs {pair_count(sym_N)} pair rows per scene, got {E}")
        Eo = sym_N * sym_N if sym_N else E          # ordered edges per scene (noise / dist layout)
        if isinstance(U, PhiloxNoise):
            if seed is None:
                seed, ctr = U.seed, U.counter
            elif (seed, ctr) != (U.seed, U.counter) and not (seed == U.seed and ctr is U.counter):
                raise ValueError("all PhiloxNoise groups of one launch must share seed and counter")
            u_ptr, off = 0, U.offset
        else:
            _req(U, "noise_u", (B, Eo, K))
            _same_device(edges, U)
            u_ptr, off = U.data_ptr(), 0
        edge_feat = torch.empty((B, E, K), dtype=torch.float32, device=edges.device)    # always fp32: a VALU scale
        dist = torch.empty((B, Eo, K), dtype=dt, device=edges.device) if (want_dist or not sym_N) else None
        opt = {}        # the training outputs keep_*, or the fused pooling's fields
        if keep is not None:
            if _twin(dt):
                raise ValueError("the bf16 twins are forward-only")
            mk = lambda w: torch.empty((B * E, w), dtype=edges.dtype, device=edges.device)
            keep.append(dict(z1=mk(128), z=mk(64), dh1=mk(256), lgf=mk(32)))
            opt = {"keep_" + n: t.data_ptr() for n, t in keep[-1].items()}
        if pool is not None:
            opt.update(xp=pool.xp.data_ptr(), pq=pool.pq.data_ptr(), pool_H=addr(pool.H), w2=pool.w2.data_ptr(),
                       b2=pool.b2.data_ptr(), pool_N=pool.xp.shape[1], pool_E=0 if pool.H is None else pool.H.shape[1])
        arr[g] = _lib.EdgeGroup(edges=0 if pool is not None else edges.data_ptr(), U=u_ptr, W=pk["W"].data_ptr(),
                                bias=pk["bias"].data_ptr(), edge_feat=edge_feat.data_ptr(), dist=addr(dist),
                                philox_offset=off, rows=B * E, K=K, sym_N=sym_N, Wx=_ximg(pk, "edge", dt),
                                Wh=_himg(pk, "edge", dt), **opt)
        outs.append((edge_feat, dist))
    flops = sum(int(a.rows) for a in arr) * 2 * (64 * 128 + 128 * 64 + 64 * 256 + 256 * 32)
    with torch.cuda.device(e0.device), _Probed("edge_mlp_gumbel_kernel", flops):
        check(_fn("gn_edge_mlp_gumbel", dt)(arr, len(items), float(tau), seed or 0, addr(ctr), stream_handle()),
              "gn_edge_mlp_gumbel")
    return outs


def edge_mlp_gumbel(edges: Tensor, U, pk: dict, K: int, tau: float = 0.5) -> Tuple[Tensor, Tensor]:
    """(edge_feat, dist) of MLP_dict_softmax.  `U`: a (B,E,K) tensor of uniforms, or a PhiloxNoise."""
    return edge_mlp_gumbel_grouped([(edges, U, pk, K)], tau)[0]


# ---- A5 ------------------------------------------------------------------------------------------
def _edge_count(H: Optional[Tensor], B: int, N: int, sym: bool = False, masks: Optional[IncidenceMasks] = None) -> int:
    if masks is not None:
        if sym:
            raise ValueError("sym applies to the pairwise graph (H=None) only")
        if not isinstance(masks, IncidenceMasks):
            raise ValueError("masks: expected an ops.IncidenceMasks")
        _req(masks.row, "masks.row", (B, None), torch.int64)
        _req(masks.col, "masks.col", (B, N), torch.int64)
        if H is not None:
            _req(H, "H", (B, masks.row.shape[1], N))
        return masks.row.shape[1]
    if H is None:
        return pair_count(N) if sym else N * N
    if sym:
        raise ValueError("sym applies to the pairwise graph (H=None) only")
    _req(H, "H", (B, None, N))
    return H.shape[1]


def agg_gather_grouped(items: Sequence[tuple]) -> List[Tensor]:
    """items = [(ori (B,N,64), H (B,E,N) or None[, sym[, masks]])] -> [eo (B,E,64)].  ``masks`` (an `IncidenceMasks`,
    N <= 64): the group is gathered from its row words instead of H (which may then be None); every hyper group of a call
    in the same form."""
    _groups(len(items))
    o0 = _req(items[0][0], "ori", (None, None, FEAT), _ACT_DTYPES)
    dt = o0.dtype
    B, N, _ = o0.shape
    arr = (_lib.GatherGroup * len(items))()
    outs = []
    for g, item in enumerate(items):
        ori, H = item[:2]
        sym = bool(item[2]) if len(item) > 2 else False
        masks = item[3] if len(item) > 3 else None
        _req(ori, "ori", (B, N, FEAT), dt)
        E = _edge_count(H, B, N, sym, masks)
        _same_device(o0, ori, H, None if masks is None else masks.row)
        eo = torch.empty((B, E, FEAT), dtype=ori.dtype, device=ori.device)
        arr[g] = _lib.GatherGroup(ori=ori.data_ptr(), H=addr(H), eo=eo.data_ptr(), E=E, sym=int(sym),
                                  rowmask=0 if masks is None else masks.row.data_ptr())
        outs.append(eo)
    with torch.cuda.device(o0.device):
        check(_fn("gn_agg_gather", dt)(arr, len(items), B, N, stream_handle()), "gn_agg_gather")
    return outs


def agg_gather(ori: Tensor, H: Optional[Tensor], sym: bool = False, masks: Optional[IncidenceMasks] = None) -> Tensor:
    return agg_gather_grouped([(ori, H, sym, masks)])[0]


class GatherSpec:
    """Input rows of the typed MLP to be formed inside the kernel instead of read from an `eo` tensor:
    eo = H @ ori (H (B,E,N)), or the pairwise rows ori_i + ori_j (H=None; sym -> unordered pairs).
    ``node=True`` (bf16 twins, pairwise graph, unordered pairs, N <= SCENE_FORM_MAX_N): the NODE form with one scene per
    workgroup — both layers run once per node (layer 1 is linear in the two nodes, layer 2 and the type weighting commute
    with H^T, see PairSpec); the result is H^T feat (B,N,64) for a ``NodeAggSpec``."""
    __slots__ = ("ori", "H", "sym", "node")

    def __init__(self, ori: Tensor, H: Optional[Tensor], sym: bool = False, node: bool = False):
        self.ori, self.H, self.sym, self.node = ori, H, bool(sym), bool(node)


class PairSpec:
    """Pair form of the typed MLP for the pairwise graph: A (B,N,K*128) = node_linear(ori) holds the first
    layer per node; rows are the N(N+1)/2 unordered pairs.  Uses pk["W2t"] instead of pk["W"].
    ``node=True`` (N <= NODE_FORM_MAX_N, bf16-core images): the NODE form — the per-pair feature is consumed only as
    H^T feat (model/MS_HGNN_batch.py:267) and type weighting + layer 2 are linear, so layer 2 runs once per node on
    S[n,k] = sum_j ef[p(n,j),k] relu(A[n,k] + A[j,k]); the result is H^T feat (B,N,64), to be fed to the closing MLP
    through a ``NodeAggSpec``."""
    __slots__ = ("A", "node")

    def __init__(self, A: Tensor, node: bool = False):
        self.A, self.node = A, bool(node)


def node_form_enabled() -> bool:
    """GN_NODE_FORM=0 keeps the per-pair form (A/B switch, read per call)."""
    return os.environ.get("GN_NODE_FORM", "1") != "0"


def _closing_askable(items, pks2: Sequence[dict]) -> bool:
    """What a descriptor of the aggregation launch cannot say about its closing stage: the A/B switches, the closing MLP
    being 128 -> 128 -> dout with its bf16-core image, and every group naming its nodes (an `eo` tensor does not)."""
    return (BF16X6 and closing_fusion_enabled()
            and all((pk2["din"], pk2["dh"]) == (2 * FEAT, 128) and _ximg(pk2, "mlp2", torch.float32) != 0 for pk2 in pks2)
            and all(isinstance(src, (PairSpec, GatherSpec)) for src, _, _, _ in items))


def _plan_takes_closing(arr, n: int, dt: torch.dtype) -> bool:
    plan = _lib.LaunchPlan()
    return _fn("gn_agg_mlp_plan", dt)(arr, n, ctypes.byref(plan)) == _lib.GN_OK and bool(plan.closing)


def closing_fusable(items: Sequence[Tuple[object, Tensor, dict, int]], pks2: Sequence[dict]) -> bool:
    """Can gn_agg_mlp_f32 apply the closing MLPs itself (gn_agg_group_t.y)?  Asks the launcher's plan
    (gn_agg_mlp_plan_*) with the descriptors of that launch, outputs as placeholders: every launch rule is the library's
    (`_closing_askable`: what a descriptor cannot say).  `agg_mlp_closing` asks and launches with one descriptor array."""
    if not _closing_askable(items, pks2):
        return False
    arr, _, _, _, dt = _agg_descriptors(items, [(pk2, None, None) for pk2 in pks2], allocate=False)
    return _plan_takes_closing(arr, len(items), dt)


def closing_fusion_enabled() -> bool:
    """GN_FUSE_CLOSING=0: the closing MLP as a launch of its own (read per call)."""
    return os.environ.get("GN_FUSE_CLOSING", "1") != "0"


_PLACEHOLDER = 16      # an aligned non-NULL "address" of a tensor not allocated yet: a plan query never dereferences it


def _agg_descriptors(items, closing=None, allocate: bool = True):
    """The gn_agg_group_t array of a typed-aggregation launch (arguments of `agg_mlp_grouped`) -> (array, outputs, (flops,
    reference flops), device, storage type).  allocate=False (a plan query): outputs, and an `ori` of the closing stage
    that is not known yet (None), are placeholders."""
    _groups(len(items))
    arr = (_lib.AggGroup * len(items))()
    outs = []
    flops = ref_flops = flops2 = 0
    dev0 = dt = None
    for g, (eo, edge_feat, pk, K) in enumerate(items):
        wkey = "W"
        if isinstance(eo, PairSpec):
            A = eo.A
            _req(A, "A", (None, None, K * 128))
            B, N = A.shape[0], A.shape[1]
            E = pair_count(N)
            _same_device(A, edge_feat)
            like, wkey = A, "W2t"
            fields = dict(E=E, N=N, sym=1, A=A.data_ptr(), W2x=_ximg(pk, "W2t", A.dtype), W2h=_himg(pk, "W2t", A.dtype),
                          node_form=int(eo.node))
            if eo.node and (N > NODE_FORM_MAX_N or K > NODE_FORM_MAX_K or not fields["W2x"]):
                raise ValueError("PairSpec(node=True): needs N <= 16, K <= 12 and the bf16-core weight images")
        elif isinstance(eo, GatherSpec):
            ori, H = eo.ori, eo.H
            _req(ori, "ori", (None, None, FEAT), _ACT_DTYPES)
            B, N, _ = ori.shape
            E = _edge_count(H, B, N, eo.sym)
            _same_device(ori, H, edge_feat)
            like = ori
            if eo.node and not (_twin(ori.dtype) and H is None and eo.sym and N <= SCENE_FORM_MAX_N):
                raise ValueError("GatherSpec(node=True): bf16 storage, the pairwise graph's unordered pairs and N <= 64")
            fields = dict(ori=ori.data_ptr(), H=addr(H), E=E, N=N, sym=int(eo.sym), W12x=_ximg(pk, "W12", ori.dtype),
                          W12h=_himg(pk, "W12", ori.dtype), node_form=int(eo.node))
        else:
            _req(eo, "eo", (None, None, FEAT), _ACT_DTYPES)
            B, E, _ = eo.shape
            _same_device(eo, edge_feat)
            like = eo
            fields = dict(eo=eo.data_ptr(), W12x=_ximg(pk, "W12", eo.dtype), W12h=_himg(pk, "W12", eo.dtype))
        dev0, dt = dev0 or like.device, dt or like.dtype
        if like.device != dev0 or like.dtype != dt:
            raise ValueError("grouped launch: every group must be on the same device and of the same storage type")
        _req(edge_feat, "edge_feat", (B, E, K))
        node = isinstance(eo, (PairSpec, GatherSpec)) and eo.node
        if closing is not None:
            pk2, out2, ori2 = closing[g]
            if ori2 is not None:
                _req(ori2, "ori", (B, N, FEAT))
            y, ldy = _mlp2_out((B, N), pk2["dout"], out2, ori2) if allocate else (None, pk2["dout"])
            # (ori: the pairwise group's node form does not read it — the fused stage reads it from there)
            fields.update(ori=fields.get("ori", _PLACEHOLDER) if ori2 is None else ori2.data_ptr(), m2x=_ximg(pk2, "mlp2", like.dtype), m2h=_himg(pk2, "mlp2", like.dtype),
                          m2bias=pk2["bias"].data_ptr(), y=y.data_ptr() if allocate else _PLACEHOLDER, ldy=ldy, dout=pk2["dout"], divisor=float(N))
            outs.append(y)
            flops2 += B * N * 2 * (128 * 128 + 128 * (((pk2["dout"] + 31) // 32) * 32))
        else:
            feat = torch.empty((B, N if node else E, FEAT), dtype=like.dtype, device=like.device) if allocate else None
            fields.update(feat=feat.data_ptr() if allocate else _PLACEHOLDER)
            outs.append(feat)
        arr[g] = _lib.AggGroup(edge_feat=edge_feat.data_ptr(), W=pk[wkey].data_ptr(), b1=pk["b1"].data_ptr(),
                               b2=pk["b2"].data_ptr(), rows=B * E, K=K, **fields)
        # executed FLOPs: both layers, or the second layer only in the pair form; node form: layer 2 per node plus the
        # 3 flops (add, max, fma) per pair-member and hidden value that form S
        if node:
            flops += (B * N * K * ((2 * 128 * 64 + 2 * 64) + (0 if wkey == "W2t" else 2 * 64 * 128))
                      + B * N * N * K * 128 * 3)
        else:
            flops += B * E * K * ((2 * 128 * 64 + 2 * 64) + (0 if wkey == "W2t" else 2 * 64 * 128))
        # the reference's form of the stage (model/MS_HGNN_batch.py:262-265): every edge row — all N*N ordered edges of
        # the pairwise graph — through both layers of every type
        pairwise = isinstance(eo, PairSpec) or (isinstance(eo, GatherSpec) and eo.H is None)
        ref_flops += B * (N * N if pairwise else E) * K * (2 * 64 * 128 + 2 * 128 * 64 + 2 * 64)
    return arr, outs, (flops + flops2, ref_flops + flops2), dev0, dt


def agg_mlp_grouped(items: Sequence[Tuple[object, Tensor, dict, int]],
                    closing: Optional[Sequence[Tuple[dict, Optional[Tensor], Tensor]]] = None) -> List[Tensor]:
    """items = [(eo (B,E,64) | GatherSpec | PairSpec, edge_feat (B,E,K) fp32, pk{"W","b1","b2","xi"[,"W2t"]}, K)]
    -> [feat (B,E,64)] in the storage type of the inputs (bf16 twin: eo / GatherSpec only).
    ``closing`` (see `closing_fusable`): per item (pk of the closing MLP, out or None, ori (B,N,64)) — the launch then also
    applies y = MLP(cat(H^T feat, ori) / N) and returns [y (B,N,dout)] instead of the features."""
    arr, outs, flops, dev0, dt = _agg_descriptors(items, closing)
    return _agg_launch(arr, outs, flops, dev0, dt)


def agg_mlp_closing(items, closing: Sequence[Tuple[dict, Optional[Tensor], Tensor]]) -> Optional[List[Tensor]]:
    """`agg_mlp_grouped(items, closing)` where the launcher's plan takes the closing stage (`closing_fusable`), else None
    and nothing is launched.  One descriptor array serves the question and the launch: it is built with placeholder
    outputs, and the outputs are allocated once the plan has accepted."""
    if not _closing_askable(items, [pk2 for pk2, _, _ in closing]):
        return None
    arr, outs, flops, dev0, dt = _agg_descriptors(items, closing, allocate=False)
    if not _plan_takes_closing(arr, len(items), dt):
        return None
    for g, (pk2, out2, ori2) in enumerate(closing):
        outs[g], arr[g].ldy = _mlp2_out(tuple(ori2.shape[:2]), pk2["dout"], out2, ori2)
        arr[g].y = outs[g].data_ptr()
    return _agg_launch(arr, outs, flops, dev0, dt)


def _agg_launch(arr, outs, flops, dev0, dt) -> List[Tensor]:
    # (the scene-form groups of the twins run in their own kernel ahead of the others' launch, on the same stream: forked
    # onto a side stream beside it they were measured at config 4 — single-stream 0.791 -> 0.784 ms, but 4-stream
    # throughput 1.445 -> 1.338 M scenes/s — and the fork was not kept)
    with torch.cuda.device(dev0), _Probed("agg_mlp_kernel", flops):
        check(_fn("gn_agg_mlp", dt)(arr, len(arr), stream_handle()), "gn_agg_mlp")
    return outs


def agg_mlp(eo: Tensor, edge_feat: Tensor, pk: dict, K: int) -> Tensor:
    return agg_mlp_grouped([(eo, edge_feat, pk, K)])[0]


def node_linear(x: Tensor, W: Tensor, bias: Tensor, dout: int) -> Tensor:
    """y = W x + bias for x (..., 64): W = packed (dout x 64) image, dout a multiple of 128."""
    _req(x, "x")
    if x.shape[-1] != FEAT:
        raise ValueError("x: last dim must be 64")
    rows = x.numel() // FEAT
    y = torch.empty(tuple(x.shape[:-1]) + (dout,), dtype=x.dtype, device=x.device)
    with torch.cuda.device(x.device), _Probed("node_linear_kernel", rows * 2 * 64 * dout):
        check(load().gn_node_linear_f32(addr(x), addr(W), addr(bias), addr(y), rows, dout, stream_handle()),
              "gn_node_linear_f32")
    return y


def agg_scatter_grouped(items: Sequence[tuple], divisor: Optional[float] = None, n_agents=None) -> List[Tensor]:
    """items = [(feat (B,E,64), H or None, ori (B,N,64)[, sym[, masks]])] -> [cat(H^T feat, ori) / divisor
    (B,N,128)]; divisor defaults to N (edge2node, model/MS_HGNN_batch.py:120,355).  ``masks``: as `agg_gather_grouped`
    (the column words are read).
    ``n_agents`` (ragged batch, `agent_counts`; gn_agg_scatter_ragged_*): node n < n_b adds its hyperedges / its partners
    j < n_b, the divisor defaults to each scene's own n_b, rows n >= n_b are zeros; no masks."""
    _groups(len(items))
    o0 = _req(items[0][2], "ori", (None, None, FEAT), _ACT_DTYPES)
    dt = o0.dtype
    B, N, _ = o0.shape
    counts = agent_counts(n_agents, B, N, o0.device)
    arr = (_lib.ScatterGroup * len(items))()
    outs = []
    for g, item in enumerate(items):
        feat, H, ori = item[:3]
        sym = bool(item[3]) if len(item) > 3 else False
        masks = item[4] if len(item) > 4 else None
        if masks is not None and counts is not None:
            raise ValueError("n_agents: the ragged scatter reads the dense H, not masks")
        _req(ori, "ori", (B, N, FEAT), dt)
        E = _edge_count(H, B, N, sym, masks)
        _req(feat, "feat", (B, E, FEAT), dt)
        _same_device(o0, feat, ori, H, None if masks is None else masks.col)
        out = torch.empty((B, N, 2 * FEAT), dtype=ori.dtype, device=ori.device)
        arr[g] = _lib.ScatterGroup(feat=feat.data_ptr(), H=addr(H), ori=ori.data_ptr(), out=out.data_ptr(), E=E,
                                   sym=int(sym), colmask=0 if masks is None else masks.col.data_ptr())
        outs.append(out)
    with torch.cuda.device(o0.device):
        if counts is not None:
            _same_device(o0, counts.dev)
            if divisor is not None and not divisor > 0:
                raise ValueError("divisor: positive, or None for each scene's own count")
            check(_fn("gn_agg_scatter_ragged", dt)(arr, len(items), B, N, float(0.0 if divisor is None else divisor),
                                                   addr(counts.dev), stream_handle()), "gn_agg_scatter_ragged")
        else:
            check(_fn("gn_agg_scatter", dt)(arr, len(items), B, N, float(N if divisor is None else divisor),
                                            stream_handle()), "gn_agg_scatter")
    return outs


def agg_scatter(feat: Tensor, H: Optional[Tensor], ori: Tensor, divisor: Optional[float] = None,
                sym: bool = False, masks: Optional[IncidenceMasks] = None, n_agents=None) -> Tensor:
    return agg_scatter_grouped([(feat, H, ori, sym, masks)], divisor, n_agents)[0]


# ---- A6 ------------------------------------------------------------------------------------------
def _mlp2_out(lead: Tuple[int, ...], dout: int, out: Optional[Tensor], like: Tensor) -> Tuple[Tensor, int]:
    if out is None:
        return torch.empty(tuple(lead) + (dout,), dtype=like.dtype, device=like.device), dout
    if not (out.is_cuda and out.dtype == like.dtype and out.device == like.device):
        raise ValueError("out: must be a tensor of the input's dtype on the input's device")
    if tuple(out.shape) != tuple(lead) + (dout,) or out.stride(-1) != 1:
        raise ValueError(f"out: expected shape {tuple(lead) + (dout,)} with unit inner stride")
    ldy = out.stride(-2) if out.dim() >= 2 else dout
    for d in range(out.dim() - 2):   # leading dims must be row-contiguous w.r.t. ldy
        if out.stride(d) != out.stride(d + 1) * out.shape[d + 1]:
            raise ValueError("out: leading dimensions must be contiguous")
    return out, ldy


class ScatterSpec:
    """Input rows of a 128-wide MLP to be formed inside the kernel instead of read from a tensor:
    cat(H^T feat, ori) / divisor (divisor defaults to N) — what agg_scatter would have produced."""
    __slots__ = ("feat", "H", "ori", "sym", "divisor")

    def __init__(self, feat: Tensor, H: Optional[Tensor], ori: Tensor, sym: bool = False,
                 divisor: Optional[float] = None):
        self.feat, self.H, self.ori, self.sym, self.divisor = feat, H, ori, bool(sym), divisor


class NodeAggSpec:
    """Input rows of a 128-wide MLP formed inside the kernel from H^T feat per NODE (the node form of the typed
    aggregation, ``PairSpec(node=True)``) and ori: cat(agg, ori) / divisor (divisor defaults to N)."""
    __slots__ = ("agg", "ori", "divisor")

    def __init__(self, agg: Tensor, ori: Tensor, divisor: Optional[float] = None):
        self.agg, self.ori, self.divisor = agg, ori, divisor


def mlp2_grouped(items: Sequence[Tuple[object, dict, Optional[Tensor]]], keep: Optional[List[dict]] = None
                 ) -> List[Tensor]:
    """items = [(x (..., din) or ScatterSpec, pk{"W","bias","din","dh","dout"}, out or None)], same
    shapes and row stride for every group.  ``out`` may be a last-dim slice of a contiguous tensor
    (row stride > dout): the kernel writes the column block in place.  ``keep`` (training): a list that
    receives, per group, {"x": the MLP's input rows as evaluated (rows, din), "hid": relu(W0 x + b0) (rows, dh)}
    — what the backward needs and the fused kernel otherwise never writes."""
    _groups(len(items))
    pk0 = items[0][1]
    din, dh, dout = pk0["din"], pk0["dh"], pk0["dout"]
    arr = (_lib.Mlp2Group * len(items))()
    outs, ld0, shape0, dev0, N, divisor, dt = [], None, None, None, 0, 1.0, None
    for g, (x, pk, out) in enumerate(items):
        if (pk["din"], pk["dh"], pk["dout"]) != (din, dh, dout):
            raise ValueError("grouped mlp2: every group must have the same layer widths")
        if isinstance(x, (NodeAggSpec, ScatterSpec)):      # the input rows cat(., ori) / divisor formed in the kernel
            if din != 2 * FEAT:
                raise ValueError(f"{type(x).__name__} feeds a 128-wide MLP")
            _req(x.ori, "ori", (None, None, FEAT), _ACT_DTYPES)
            B, Nn, _ = x.ori.shape
            if isinstance(x, NodeAggSpec):
                _req(x.agg, "agg", (B, Nn, FEAT), x.ori.dtype)
                _same_device(x.ori, x.agg)
                fields = dict(feat=x.agg.data_ptr(), ori=x.ori.data_ptr())
            else:
                E = _edge_count(x.H, B, Nn, x.sym)
                _req(x.feat, "feat", (B, E, FEAT), x.ori.dtype)
                _same_device(x.ori, x.feat, x.H)
                fields = dict(feat=x.feat.data_ptr(), H=addr(x.H), ori=x.ori.data_ptr(), E=E, sym=int(x.sym))
            d = float(Nn if x.divisor is None else x.divisor)
            if N and (N, divisor) != (Nn, d):
                raise ValueError("grouped mlp2: every fused-scatter group must share N and divisor")
            N, divisor = Nn, d
            lead, like = (B, Nn), x.ori
        else:
            _req(x, "x", None, _ACT_DTYPES)
            if x.shape[-1] != din:
                raise ValueError(f"x: last dim {x.shape[-1]} != {din}")
            lead, like = tuple(x.shape[:-1]), x
            fields = dict(x=x.data_ptr())
        if shape0 is None:
            shape0, dev0, dt = lead, like.device, like.dtype
        elif lead != shape0 or like.device != dev0 or like.dtype != dt:
            raise ValueError("grouped mlp2: every group must have the same leading shape, device and storage type")
        y, ldy = _mlp2_out(lead, dout, out, like)
        if ld0 is None:
            ld0 = ldy
        elif ldy != ld0:
            raise ValueError("grouped mlp2: every group must have the same output row stride")
        if keep is not None:
            if _twin(dt):
                raise ValueError("the bf16 twins are forward-only")
            kd = dict(x=torch.empty((math.prod(lead), din), dtype=like.dtype, device=like.device),
                      hid=torch.empty((math.prod(lead), dh), dtype=like.dtype, device=like.device))
            keep.append(kd)
            fields.update(in_out=kd["x"].data_ptr(), hid_out=kd["hid"].data_ptr())
        arr[g] = _lib.Mlp2Group(W=pk["W"].data_ptr(), bias=pk["bias"].data_ptr(), y=y.data_ptr(),
                                Wx=_ximg(pk, "mlp2", dt) if dout <= 64 else 0, Wh=_himg(pk, "mlp2", dt) if dout <= 64 else 0,
                                **fields)
        outs.append(y)
    rows = math.prod(shape0)
    flops = len(items) * rows * 2 * (din * dh + dh * (((dout + 31) // 32) * 32))
    with torch.cuda.device(dev0), _Probed("mlp2_kernel", flops):
        check(_fn("gn_mlp2", dt)(arr, len(items), rows, din, dh, dout, ld0, N, divisor, stream_handle()),
              "gn_mlp2")
    return outs


def mlp2(x: Tensor, pk: dict, out: Optional[Tensor] = None) -> Tensor:
    """y = W1 relu(W0 x + b0) + b1 over the last dim of x."""
    return mlp2_grouped([(x, pk, out)])[0]


# ---- noise ---------------------------------------------------------------------------------------
def philox_uniform(shape: Sequence[int], seed: int, offset: int, device, offset_dev: Optional[Tensor] = None) -> Tensor:
    """Uniforms in [0,1) from the Philox4x32-10 stream `seed` at element position
    `offset` (+ the int64 device counter `offset_dev`, if given)."""
    U = torch.empty(tuple(shape), dtype=torch.float32, device=device)
    if not U.is_cuda:
        raise ValueError("philox_uniform: device must be a GPU")
    _counter_arg(offset_dev, "offset_dev")
    with torch.cuda.device(U.device):
        check(load().gn_philox_uniform_f32(addr(U), U.numel(), int(seed) & (2**64 - 1), int(offset), addr(offset_dev),
                                           stream_handle()), "gn_philox_uniform_f32")
    return U


def counter_add(counter: Tensor, add: int) -> None:
    """counter += add, in stream order (counter: 1-element int64 GPU tensor)."""
    _counter_arg(counter)
    with torch.cuda.device(counter.device):
        check(load().gn_counter_add_u64(addr(counter), int(add), stream_handle()), "gn_counter_add_u64")




def copy_cols(dst: Tensor, src: Tensor) -> None:
    """dst (contiguous) <- src, where src is a last-dim slice of a wider contiguous tensor (a column block of the
    concatenated features): one pitched copy launch (`gn_copy_2d`) instead of a strided elementwise copy."""
    if not (src.is_cuda and dst.is_cuda and src.dtype == dst.dtype and tuple(src.shape) == tuple(dst.shape)):
        raise ValueError("copy_cols: GPU tensors of equal shape and dtype")
    w = src.shape[-1] * src.element_size()
    rows = src.numel() // src.shape[-1]
    ok = (dst.is_contiguous() and src.stride(-1) == 1 and w % 16 == 0 and src.dim() >= 2
          and (src.stride(-2) * src.element_size()) % 16 == 0 and src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
          and all(src.stride(d) == src.stride(d + 1) * src.shape[d + 1] for d in range(src.dim() - 2)))
    if not ok:
        dst.copy_(src, non_blocking=True)
        return
    with torch.cuda.device(src.device):
        check(load().gn_copy_2d(_P(dst.data_ptr()), w, _P(src.data_ptr()), src.stride(-2) * src.element_size(), w, rows,
                                stream_handle()), "gn_copy_2d")
