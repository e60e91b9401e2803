"""hipGraph capture of the multiscale forward.

One MS-HGNN forward is ~35 short kernel launches on 1+S streams; at B=512 the GPU work is a few
hundred microseconds, less than what the host needs to issue those launches one by one.  The
launchers of libgroupnet_hip.so never synchronise or allocate, so the whole forward (side-stream
fork/join included) is captured once into a hipGraph and replayed with one host call.

Noise inside a graph: the host draw of the reference (torch.rand on the CPU) cannot be captured, so
a graphed forward uses the device Philox stream.  Its position lives in a device counter that the
graph itself advances at the end of every replay — each replay draws fresh, reproducible noise.

Weights inside a graph: an inference forward trusts the packed weight images (`weights.WeightCache`), so the graphs of
`GraphedMultiScale` and `GraphedPastEncoder` contain no pack or split launch — they READ the images (pack-plan arenas,
split images, the encoder's composed embedding) where they lay at capture.  `refresh_weights()` re-derives all of them
from the live parameters in place; a replay does so by itself after `invalidate_weight_caches`; parameter storage that
moved means capturing again.  `GraphedTrainStep` re-packs inside its graph.
"""
from __future__ import annotations

import contextlib
import gc
from typing import Callable, Optional, Sequence, Tuple

import torch

from . import MS_HGNN_batch as _mods
from . import ops, route, weights
from .multiscale import MultiScaleHGNN

Tensor = torch.Tensor


@contextlib.contextmanager
def _noise_state_kept():
    """Puts the process's noise state back on the way out: the steps of a capture switch it to the device stream."""
    prev = (_mods._NoiseState.mode, _mods._NoiseState.seed, _mods._NoiseState.offset, _mods._NoiseState.counter)
    try:
        yield
    finally:
        _mods.set_noise_mode(prev[0], prev[1], prev[2], prev[3])


def _capture(graph, device, step: Callable, counter: Tensor, draws_per_step: int, warmup: int,
             before_capture: Optional[Callable] = None):
    """The capture protocol of the three graphed classes; returns what the captured ``step()`` returned (the graph's
    static outputs).  ``before_capture``: run between the warm-up and the capture."""
    # An autograd graph left over from an eager training step keeps the parameters' AccumulateGrad nodes, which run on the
    # stream they were MADE on: made on the default stream they would pull it into the capture of a training step.  Drop
    # what only a reference cycle keeps alive, so that the warm-up below makes them anew on its own stream.
    gc.collect()
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):      # warm-up off the default stream: packs weights, sizes the pool
        for _ in range(max(1, warmup)):
            step()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize(device)
    # every replay first advances the counter by one step's worth of draws: start one step back
    counter.fill_(-draws_per_step)
    if before_capture is not None:
        before_capture()
    with torch.cuda.graph(graph):
        return step()


def _counts_holder(ragged, B: int, N: int, device, refuse: Callable):
    """The count holder of a capture by its ``ragged=`` argument — False: None, True: an `ops.StaticAgentCounts`,
    "subset": an `ops.StaticAgentSubset` — made, and filled with N, before the capture begins.  ``refuse``: the
    capture's own refusals of a ragged route, run before anything is allocated."""
    if ragged not in (False, True, "subset"):
        raise ValueError("ragged: False, True or 'subset'")
    if not ragged:
        return None
    refuse()
    return (ops.StaticAgentSubset if ragged == "subset" else ops.StaticAgentCounts)(B, N, device)


def _checked_counts(holder, B: int, N: int, device, n_agents, agent_mask):
    """The host validation of a replay's ``n_agents`` / ``agent_mask`` for a graphed class's ``__call__``, before
    anything is copied or launched: at most one of them, on a ragged capture only (``holder``) -> the validated count
    values, or None where no counts were given."""
    if n_agents is None and agent_mask is None:
        return None
    if holder is None:
        raise ValueError("n_agents / agent_mask: the graph was captured without ragged=True")
    if n_agents is not None and agent_mask is not None:
        raise ValueError("n_agents and agent_mask: give at most one of them")
    if n_agents is not None:
        return ops.count_values(n_agents, B, N, lowest=0)
    ops._mask_arg(agent_mask, B, N, device)
    return None


def _set_counts(holder, vals, agent_mask) -> None:
    """What `_checked_counts` admitted, into the holder: the values through its staging ring, or the mask through its
    device kernel; neither synchronises."""
    if vals is not None:
        holder.set(vals)
    elif agent_mask is not None:
        holder.set_from_mask(agent_mask)


def _status(holder) -> int:
    if holder is None:
        raise ValueError("status: the graph was captured without ragged=True")
    return int(holder.status.item()) & 0xFFFFFFFF


class GraphedMultiScale:
    """Static-shape, replayable forward of a ``MultiScaleHGNN`` block.

        g = GraphedMultiScale(block, B, N, seed=1234)
        feats, H = g(f)          # f is copied into the graph's input buffer; outputs are the
                                 # graph's static buffers (overwritten by the next call)

    A RAGGED capture (``ragged=True``; INTEGRATION.md, "Ragged batches") replays batches whose scenes hold different
    numbers of agents, empty slots (count 0) included:

        g = GraphedMultiScale(block, B, N, seed=1234, ragged=True)
        feats, H = g(f, n_agents=[11, 7, 0, ...])     # counts: a sequence of ints or a CPU integer tensor, 0..N
        feats, H = g(f, agent_mask=valid)             # ... or a (B,N) bool / uint8 mask that is already on the GPU
        feats, H = g(f)                               # the previous counts stay
        g.status()                                    # the mask entry's sticky status word (synchronises)

    With ``ragged="subset"`` the mask may have zeros anywhere: agents enter and leave scenes, and every result comes back
    at the agent's own slot (zeros at invalid ones).

    WEIGHTS.  The graph holds no packing launch: it reads the block's packed weight images in place, as they were when it
    was captured.  After the parameters changed IN PLACE — `load_state_dict`, an eager optimizer step, a ``.data`` write —
    call ``g.refresh_weights()``: it re-derives every arena and split image the captured forward reads from the live
    parameters, at the captured addresses, eagerly on the current stream.  After `invalidate_weight_caches(block)` —
    which `GraphedTrainStep.__call__` runs after every replay — the next ``g(...)`` refreshes by itself, so one block
    under a train graph and an eval graph needs no extra call.  A parameter whose STORAGE moved (``p.data = ...``,
    ``block.to(...)``) cannot be followed: `refresh_weights` raises `RuntimeError`; capture again.  Graphs of one block
    that replay on several streams share the images: refresh on one stream and order the others behind it.
    """

    def __init__(self, block: MultiScaleHGNN, B: int, N: int, seed: int = 0, device: Optional[torch.device] = None,
                 warmup: int = 2, dtype: torch.dtype = torch.float32, affinity_tail: Optional[bool] = None,
                 ragged: bool = False):
        """``affinity_tail``: capture with `block.affinity_tail` set to this value (None: as the block has it) — True =
        the latency form (affinity + top-k in the first node stage's tail), False = the throughput form for graphs that
        are replayed side by side on several streams (see `MultiScaleHGNN.affinity_tail`).
        ``ragged``: capture the ragged route with the counts in an `ops.StaticAgentCounts` (``self.counts``), made and
        filled with N before the capture begins: the graph holds the buffer's address, nothing is uploaded inside it, and
        the route is the ragged one whatever the counts of a replay are.  Noise keeps the padded shapes and the same
        ``draws_per_step``; the ragged affinity launch carries the counter bump.
        ``ragged="subset"`` ("Agents missing anywhere"): the counts live in an `ops.StaticAgentSubset`,
        and the graph holds the compaction launch, the ragged route and the expansion launch — ``agent_mask=`` then takes
        masks with holes (the subset kernel runs ahead of the replay, nothing is read back), ``n_agents=`` sets prefix
        counts, and `status` can only ever show `_lib.COUNTS_EMPTY`."""
        p = next(block.parameters())
        self.device = device or p.device
        if self.device.type != "cuda":
            raise ValueError("GraphedMultiScale needs the block on a GPU")
        # (the refusals of the eager ragged forward, before anything is allocated or launched)
        self.counts: Optional[ops.StaticAgentCounts] = _counts_holder(
            ragged, B, N, self.device, lambda: _mods.refuse_ragged(
                training=block.training, listall=any(m.listall for m in block.interaction_hyper)))
        self.block = block
        self.B, self.N = B, N
        self.seed = int(seed)
        self.f_in = torch.zeros((B, N, block.h_dim), dtype=dtype, device=self.device)    # bf16: the twins (config 4)
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.draws_per_step = sum(b * e * k for (b, e, k) in block.noise_shapes(B, N)) * block.interaction.nmp_layers
        self.graph = torch.cuda.CUDAGraph()
        with _noise_state_kept():
            prev_tail = block.affinity_tail
            if affinity_tail is not None:
                block.affinity_tail = bool(affinity_tail)
            try:
                with torch.no_grad(), torch.cuda.device(self.device), weights.seen_caches() as seen:
                    self.out, self.H = _capture(self.graph, self.device, self._step, self.counter, self.draws_per_step,
                                                warmup)
                    self._weights = weights.CapturedWeights(seen)
            finally:
                block.affinity_tail = prev_tail

    def refresh_weights(self) -> None:
        """Re-derive every packed weight image the captured forward reads from the block's live parameters, in place, on
        the current stream (see the class docstring).  `RuntimeError`, before anything is launched, where a parameter's
        storage moved since the capture."""
        with torch.no_grad(), torch.cuda.device(self.device):
            self._weights.refresh("GraphedMultiScale.refresh_weights")

    def _step(self) -> Tuple[Tensor, Optional[Tensor]]:
        # offset 0 + device counter: the position is entirely on the device; the first launch of the
        # forward moves the counter past the previous replay's draws
        _mods.set_noise_mode("device", seed=self.seed, offset=0, counter=self.counter)
        return self.block(self.f_in, advance=(self.counter, self.draws_per_step), n_agents=self.counts)

    def __call__(self, f: Optional[Tensor] = None, n_agents=None, agent_mask: Optional[Tensor] = None
                 ) -> Tuple[Tensor, Optional[Tensor]]:
        """``n_agents`` / ``agent_mask`` (ragged captures only, at most one of them): this replay's counts — see
        `ops.StaticAgentCounts.set` and `set_from_mask`; neither: the previous counts stay.  Both are checked on the host
        before anything is copied or launched; neither path synchronises."""
        vals = _checked_counts(self.counts, self.B, self.N, self.device, n_agents, agent_mask)
        if f is not None:
            self.f_in.copy_(f, non_blocking=True)
        _set_counts(self.counts, vals, agent_mask)
        if self._weights.epoch != weights._EPOCH[0]:      # something was invalidated since the images were derived
            self.refresh_weights()
        self.graph.replay()
        return self.out, self.H

    def status(self) -> int:
        """The sticky status word of the mask entry (`_lib.COUNTS_NOT_PREFIX` | `_lib.COUNTS_EMPTY`, 0: nothing seen) of
        a ragged capture.  THE one call here that synchronises: it reads the device word back."""
        return _status(self.counts)


class GraphedPastEncoder:
    """Static-shape, replayable inference forward of a `PastEncoder` drop-in (embedding front-end, affinity,
    incidences, all modules, concat — `model/GroupNet_nba.py:266-315`) as one hipGraph.

        g = GraphedPastEncoder(enc.eval(), B, N, seed=7)
        feats, new_H = g(inputs)       # inputs (B*N, T, in_dim) copied into the static buffer; outputs static

    WEIGHTS: as `GraphedMultiScale` — the graph reads the modules' packed images and the composed embedding (M, c) in
    place; ``g.refresh_weights()`` after the parameters changed in place, by itself after `invalidate_weight_caches`,
    `RuntimeError` (capture again) where a parameter's storage moved.
    """

    def __init__(self, enc, B: int, N: int, seed: int = 0, warmup: int = 2):
        p = next(enc.parameters())
        self.device = p.device
        if self.device.type != "cuda":
            raise ValueError("GraphedPastEncoder needs the encoder on a GPU")
        if enc.training:
            raise ValueError("GraphedPastEncoder captures the inference path: call enc.eval() first")
        if not enc.fused_front_end_fits(N, enc._length):
            raise ValueError(f"GraphedPastEncoder captures the fused front-end only: the scene tile of N = {N} agents with "
                             f"{enc._length * enc.input_fc.in_features} raw inputs each exceeds the fused affinity launch's "
                             "LDS; call the encoder eagerly")
        self.enc, self.B, self.N, self.seed = enc, B, N, int(seed)
        self.x_in = torch.zeros((B * N, enc._length, enc.input_fc.in_features), dtype=torch.float32, device=self.device)
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        hypers = [getattr(enc, n) for n in enc._hyper_names]
        self.draws_per_step = B * N * N * enc.interaction.edge_types + sum(
            B * (1 if m.scale == N else N) * m.edge_types for m in hypers)
        self.graph = torch.cuda.CUDAGraph()
        with _noise_state_kept():
            try:
                with torch.no_grad(), torch.cuda.device(self.device), weights.seen_caches() as seen:
                    self.out, self.H = _capture(self.graph, self.device, self._step, self.counter, self.draws_per_step,
                                                warmup)
                    self._weights = weights.CapturedWeights(seen)
            finally:
                enc.__dict__.pop("_advance", None)
        # the composed embedding the graph reads (kept alive here) and the parameters it was composed from
        self._affine = enc._compose(enc._length, N)
        self._front = tuple(enc._front_params())
        self._front_ptrs = tuple(p.data_ptr() for p in self._front)

    def refresh_weights(self) -> None:
        """Re-derive, in place and on the current stream, the composed embedding (M, c) and every packed weight image the
        captured forward reads.  `RuntimeError`, before anything is launched, where a parameter's storage moved."""
        what = "GraphedPastEncoder.refresh_weights"
        if tuple(p.data_ptr() for p in self._front) != self._front_ptrs:
            raise weights.moved_storage(what)
        self._weights.check(what)
        with torch.no_grad(), torch.cuda.device(self.device):
            if any(a is not b for a, b in zip(self.enc._compose(self.enc._length, self.N, fresh=True), self._affine)):
                raise weights.moved_storage(what)      # (the encoder's own buffers were replaced)
            self._weights.refresh(what)

    def _step(self):
        _mods.set_noise_mode("device", seed=self.seed, offset=0, counter=self.counter)
        self.enc._advance = (self.counter, self.draws_per_step)
        return self.enc(self.x_in, self.B, self.N)

    def __call__(self, inputs: Optional[Tensor] = None):
        if inputs is not None:
            self.x_in.copy_(inputs, non_blocking=True)
        if self._weights.epoch != weights._EPOCH[0]:
            self.refresh_weights()
        self.graph.replay()
        return self.out, self.H


class GraphedTrainStep:
    """One training step of a ``MultiScaleHGNN`` block — forward, loss, backward and the optimizer update —
    captured in ONE hipGraph (`train_hyper_nba.py:107-118` is this loop).

    Eagerly a step is ~150 launches whose host side (autograd bookkeeping, descriptor tables, allocations)
    takes several times longer than the GPU work; replayed from a graph the step runs at GPU speed.

        step = GraphedTrainStep(block, opt, loss_fn, B, N, target_shapes=[(B, N, 2)], seed=7)
        loss = step(f, target)        # copies into the graph's static inputs, replays, returns the loss tensor

    ``loss_fn(final_feature, new_H, *targets) -> scalar``.  Noise is the device Philox stream, advanced inside
    the graph so every replay draws fresh Gumbel noise.  Everything that depends on parameter values (packed
    weight images) is rebuilt inside the graph; after a replay the eager caches are dropped, so eager calls
    between replays see the updated parameters.  Optimizers must be capturable (SGD is; Adam with
    ``capturable=True``).

    A RAGGED capture (``ragged=True``; INTEGRATION.md, "Ragged batches", Training from a captured graph) trains on
    batches whose scenes hold different numbers of agents, empty slots (count 0) included:

        step = GraphedTrainStep(block, opt, loss_fn, B, N, target_shapes=[(B, N, 2)], seed=7, ragged=True)
        loss = step(f, target, n_agents=[11, 7, 0, ...])   # counts: a sequence of ints or a CPU integer tensor, 0..N
        loss = step(f, target, agent_mask=valid)           # ... or a (B,N) bool / uint8 mask that is already on the GPU
        loss = step(f, target)                             # the previous counts stay
        step.status()                                      # the mask entry's sticky status word (synchronises)

    The loss is then called as ``loss_fn(final_feature, new_H, *targets, valid=valid)`` with ``valid`` a (B,N) bool
    tensor made inside the graph at every replay — true at the real agents — so that it can normalise over them; an
    empty slot adds exactly zero to every parameter gradient.  With ``ragged="subset"`` the mask may have zeros
    anywhere, as in `GraphedMultiScale`.  The capture is its own opt-in: it needs no `set_ragged_training`, and the
    eager refusals stay as they are."""

    def __init__(self, block: MultiScaleHGNN, optimizer: torch.optim.Optimizer, loss_fn: Callable, B: int, N: int,
                 target_shapes: Sequence[Tuple[int, ...]] = (), seed: int = 0, warmup: int = 3, ragged: bool = False):
        """``ragged``: False, True or "subset", as in `GraphedMultiScale`: the counts live in an `ops.StaticAgentCounts` /
        `ops.StaticAgentSubset` (``self.counts``), made and filled with N before the capture; the graph holds its
        address and — for "subset" — the compaction, the ragged training route and the expansion.  What the eager ragged
        training refuses is refused here, before anything is allocated or launched: a ``listall`` module, N beyond the
        per-scene node->edge backward, a scale beyond N."""
        p = next(block.parameters())
        self.device = p.device
        if self.device.type != "cuda":
            raise ValueError("GraphedTrainStep needs the block on a GPU")

        def refuse():
            _mods.refuse_ragged(large=N > route.N2E_BWD_SCENE_MAX_N, listall=any(m.listall for m in block.interaction_hyper))
            if any(s > N for s in block.hyper_scales):
                raise RuntimeError("selected index k out of range")

        self.counts: Optional[ops.StaticAgentCounts] = _counts_holder(ragged, B, N, self.device, refuse)
        self.B, self.N = B, N
        self.block, self.optimizer, self.loss_fn = block, optimizer, loss_fn
        self.seed = int(seed)
        self.f_in = torch.zeros((B, N, block.h_dim), dtype=torch.float32, device=self.device)
        self.targets = [torch.zeros(tuple(s), dtype=torch.float32, device=self.device) for s in target_shapes]
        self.counter = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.draws_per_step = sum(b * e * k for (b, e, k) in block.noise_shapes(B, N)) * block.interaction.nmp_layers
        self.graph = torch.cuda.CUDAGraph()
        self._repack: dict = {}
        def before_capture():
            _mods.invalidate_weight_caches(block)       # every packing kernel must be part of the graph
            optimizer.zero_grad(set_to_none=True)       # gradients are allocated from the graph's pool

        with _noise_state_kept(), torch.cuda.device(self.device):
            self.loss = _capture(self.graph, self.device, self._step, self.counter, self.draws_per_step, warmup,
                                 before_capture)
            _mods.invalidate_weight_caches(block)

    def _step(self) -> Tensor:
        _mods.set_noise_mode("device", seed=self.seed, offset=0, counter=self.counter)
        self.optimizer.zero_grad(set_to_none=True)
        # every packed weight image of the step from TWO launches at its head (weights.repack_scope: the first warm-up step
        # records which plans / images a step touches)
        # (a ragged capture is its own opt-in: the scope admits ``n_agents`` under autograd, and holders with empty slots)
        scope = contextlib.nullcontext() if self.counts is None else _mods.ragged_train_graph_scope()
        with weights.repack_scope(self._repack), scope:
            with torch.enable_grad():
                if self.counts is None:
                    out, H = self.block(self.f_in, advance=(self.counter, self.draws_per_step))
                    loss = self.loss_fn(out, H, *self.targets)
                else:
                    out, H = self.block(self.f_in, advance=(self.counter, self.draws_per_step), n_agents=self.counts)
                    loss = self.loss_fn(out, H, *self.targets, valid=self._valid())
            loss.backward()
        self.optimizer.step()
        return loss.detach()

    def _valid(self) -> Tensor:
        """(B,N) bool, true at the real agents, from the holder's device values (nothing is read back): the slots with a
        rank of a subset, else the first n_b of every scene."""
        if isinstance(self.counts, ops.AgentSubset):
            return self.counts.slot >= 0
        return torch.arange(self.N, dtype=torch.int32, device=self.device)[None, :] < self.counts.dev[:, None]

    def __call__(self, f: Optional[Tensor] = None, *targets: Tensor, n_agents=None, agent_mask: Optional[Tensor] = None
                 ) -> Tensor:
        """``n_agents`` / ``agent_mask`` (ragged captures only, at most one of them): this replay's counts, as in
        `GraphedMultiScale.__call__` — checked on the host before anything is copied or launched; neither: the previous
        counts stay."""
        vals = _checked_counts(self.counts, self.B, self.N, self.device, n_agents, agent_mask)
        if f is not None:
            self.f_in.copy_(f, non_blocking=True)
        for dst, src in zip(self.targets, targets):
            dst.copy_(src, non_blocking=True)
        _set_counts(self.counts, vals, agent_mask)
        self.graph.replay()
        _mods.invalidate_weight_caches(self.block)
        return self.loss

    def status(self) -> int:
        """The sticky status word of the mask entry of a ragged capture, as `GraphedMultiScale.status`.  THE one call
        here that synchronises."""
        return _status(self.counts)
