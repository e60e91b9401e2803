"""The multiscale block around the path: what ``PastEncoder.forward`` does between computing the
agent embedding and concatenating the per-scale features (model/GroupNet_nba.py:284-311).

    corr  = normalize(f) normalize(f)^T                         :284-286
    inter = MS_HGNN_oridinary(f)                                :290
    hyper_s, H_s = MS_HGNN_hyper_s(f, corr)  for each scale     :293-299
    final = cat(f, inter, hyper_1, ...)                         :301-309
    new_H = cat(H_1, H_2, ...) on dim 1                         :296,299

MI355X-first choices: affinity and the incidence of EVERY scale come from one fused launch
(corr never makes a trip through HBM at all); the 1+S modules are independent given (f, H_s), so
each stage of all of them is ONE grouped launch (the hyper modules have only B*N edge rows each
and would leave most of the 256 CUs idle if launched one behind the other).

The graph stage — f to the incidences of every scale — is decided by `route.graph_stage_route` and built by
`build_graphs`, for the block's inference forward, for `multiscale_autograd` and for the trajectory encoders alike.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import contextlib
import torch
import torch.nn as nn

from . import MS_HGNN_batch as _mods
from . import ops, route
from .MS_HGNN_batch import (MS_HGNN_hyper, MS_HGNN_oridinary, _needs_grad, _plist, masks_apply, ragged_counts,
                            ragged_grad_refusals, run_message_passing)

Tensor = torch.Tensor


def noise_shapes(pair: MS_HGNN_oridinary, hypers: Sequence[MS_HGNN_hyper], scales: Sequence[int], B: int, N: int
                 ) -> List[Tuple[int, int, int]]:
    """(B,E,K) of the uniforms each module draws per message-passing round, pairwise first."""
    return [(B, N * N, pair.edge_types)] + [(B, 1 if s == N else N, m.edge_types) for s, m in zip(scales, hypers)]


def draw_noise(shapes: Sequence[Tuple[int, int, int]], rounds: int, device: torch.device) -> List[list]:
    """`rounds` uniforms per shape, drawn as the reference does: module-major — every round of the pairwise module, then
    scale by scale — so that a seeded training forward sees the noise of the seeded inference forward.  Through the
    engine's `_draw_uniform` as it stands at the time of the call, like the engine's own draws."""
    return [[_mods._draw_uniform(shp, device) for _ in range(rounds)] for shp in shapes]


def graph_route(S: int, B: int, N: int, D: int, facts: route.StageFacts, ragged: bool = False, training: bool = False,
                ragged_training: bool = False) -> route.GraphStage:
    """`route.graph_stage_route` for a block without the embedding front-end.  The library is asked about the launch that
    is then built, mask words included (which cannot change the answer today: masks need N <= 64, where the tile at
    D = 64 with eight scales of mask words is 58 384 B of the 128 KiB)."""
    masked = masks_apply(N)
    form = ops.graph_form(N, D, 0, S if route.graph_stage_masks(S, masked, ragged) else 0)
    return route.graph_stage_route(S, form, B * N, masked=masked, ragged=ragged, training=training, facts=facts,
                                   ragged_training=ragged_training)


_FORK_STREAMS = {}


def _fork_stream(device: torch.device) -> "torch.cuda.Stream":
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    st = _FORK_STREAMS.get(key)
    if st is None:
        st = _FORK_STREAMS[key] = torch.cuda.Stream(device=device)
    return st


def build_graphs(r: route.GraphStage, f: Optional[Tensor], scales: Sequence[int], *, width: int = 0, advance=None,
                 counts=None, embed=None):
    """The graph stage of a forward, as `r` states it.  ``width``: allocate ``final`` with that many columns (0: no final
    — a training forward concatenates); ``advance`` = (counter, n): add n to the device Philox counter; ``counts``: the
    ragged batch's `ops.AgentCounts`; ``embed`` = (x_raw, M, c) with f = None: the fused launch computes f itself.
    -> (f, the features the modules run on;  incidences, one per scale, what `run_message_passing` takes after the
    pairwise module's None;  new_H = cat(H_s, dim=1) where the route builds it;  the deferred job for
    `run_message_passing(affinity=)` or None;  join, to be called after the first node stage when the job runs on the
    side stream, or None;  final (B, N, width) with f in its first D columns;  cols, its 1+S module slices, written in
    place by the last MLP)."""
    x = f if embed is None else embed[0]
    B, N = x.shape[0], x.shape[1]
    D = f.shape[2] if embed is None else embed[1].shape[0]
    S = len(scales)
    final = cols = job = join = new_H = None
    incs = []
    if width:
        final = torch.empty((B, N, width), dtype=x.dtype, device=x.device)
        cols = [final[..., D * (1 + i):D * (2 + i)] for i in range(1 + S)]
    if r.kind == route.FUSED:
        # one launch: affinity, incidence of every scale, f -> final[..., :D], cat(H_s), Philox bump — on the side stream
        # where the route forks, handed on unlaunched where it defers
        side = _fork_stream(x.device) if r.fork else None
        if r.fork:
            main = torch.cuda.current_stream(x.device)
            side.wait_stream(main)
            join = lambda: main.wait_stream(side)
        with (torch.cuda.stream(side) if r.fork else contextlib.nullcontext()):
            # >= 1 scale per launch; N = the cheap all-ones edge, whose incidence is dropped
            job = ops.AffinityTail(f, list(scales) or [N], f_out=final[..., :D] if width else None, want_H_cat=r.H_cat,
                                   counter=advance[0] if advance else None, counter_add=advance[1] if advance else 0,
                                   embed=embed, want_masks=r.masks, n_agents=counts)
            if not r.deferred:
                job.launch()
        f, new_H, incs = job.f, job.H_cat, (job.incidences if S else [])
    elif r.kind == route.BANDED:
        # large N (N*(N+68)*4 B > LDS tile): banded affinity and banded top-k launches, plain copies
        incs = ops.topk_incidence(ops.affinity(f if f.dtype == torch.float32 else f.float()), list(scales), counts)
        new_H = torch.cat(incs, dim=1).to(f.dtype) if r.H_cat else None
    if r.own_copy:
        final[..., :D].copy_(f)
        if advance:
            ops.counter_add(advance[0], advance[1])
    return f, incs, new_H, (job if r.deferred else None), join, final, cols


_TRAINING = route.StageFacts(grouped=True, latency_form=False, capturing=False, embed=False, may_defer=False)


def multiscale_autograd(pair: MS_HGNN_oridinary, hypers: Sequence[MS_HGNN_hyper], scales: Sequence[int], f: Tensor,
                        noise_u: Optional[Sequence] = None, counts=None) -> Tuple[Tensor, Optional[Tensor]]:
    """cat(f, pairwise(f), hyper_s(f, corr)...) and cat(H_s) with autograd attached: incidences from the graph stage
    (constants of the backward), then ONE `MSHGNNFunction` node over all modules.  In mask form (`masks_apply(N)`) the
    fused launch also emits the member words, which the forward and the backward then read.  The device counter is the
    caller's to bump.  ``counts``: the `ops.AgentCounts` of a ragged batch (`set_ragged_training`) — the graph stage
    builds the ragged incidences, forward and backward take their count-aware routes."""
    from .backward import MSHGNNFunction
    S = len(hypers)
    fd = f.detach().contiguous()
    B, N, D = fd.shape
    ragged = counts is not None
    _, graphs, new_H, *_ = build_graphs(graph_route(S, B, N, D, _TRAINING, ragged=ragged, training=True,
                                                    ragged_training=ragged), fd, scales, counts=counts)
    mods = (pair, *hypers)
    if noise_u is None:
        noise_u = draw_noise(noise_shapes(pair, hypers, scales, B, N), pair.nmp_layers, fd.device)
    nz = tuple(noise_u)
    if len(nz) != 1 + S:
        raise ValueError(f"noise_u: need {1 + S} entries (pairwise + one per scale)")
    params = [p for m in mods for p in _plist(m)]
    res = MSHGNNFunction.apply(mods, (None, *graphs), nz, counts, *([f] * (1 + S)), *params)
    return torch.cat([f, *res[0::2]], dim=-1), new_H


class MultiScaleHGNN(nn.Module):
    """One pairwise module + one hyper module per scale on the same (f, corr).

    ``forward(f)`` -> ``(final_feature (B, N, 64*(2+S)), new_H (B, sum_s E_s, N))``.
    Unlike ``PastEncoder`` (three scales at most, model/GroupNet_nba.py:218-248) any number of
    scales up to 8 is accepted (BASELINE configs 4 and 5 use four).
    """

    def __init__(self, hyper_scales: Sequence[int] = (2, 5, 11), h_dim: int = 64, nmp_layers: int = 1,
                 grouped: bool = True):
        super().__init__()
        if not 0 <= len(hyper_scales) <= 8:
            raise ValueError("0..8 scales")
        self.hyper_scales = [int(s) for s in hyper_scales]
        self.h_dim = h_dim
        # same constructor arguments as PastEncoder.__init__ (model/GroupNet_nba.py:209-248)
        self.interaction = MS_HGNN_oridinary(embedding_dim=16, h_dim=h_dim, mlp_dim=64, bottleneck_dim=h_dim,
                                             batch_norm=0, nmp_layers=nmp_layers)
        self.interaction_hyper = nn.ModuleList(
            MS_HGNN_hyper(embedding_dim=h_dim, h_dim=h_dim, mlp_dim=64, bottleneck_dim=h_dim, batch_norm=0,
                          nmp_layers=nmp_layers, scale=s) for s in self.hyper_scales)
        self.grouped = grouped
        # The fused affinity + top-k launch rides as the tail workgroups of the first node-stage launch (one launch and
        # one boundary fewer: -5.5 us of 116 on a dependent chain of forwards at B = 512, N = 11).  A caller that overlaps
        # independent forwards on several streams may prefer it as its own small launch, which fits beside other
        # streams' kernels (+2.6 % throughput on 4 streams in the same measurement): set False.  The same switch selects
        # whether the typed-aggregation launch applies the closing MLPs itself (4 launches instead of 5: same latency,
        # -2 % throughput side by side — `run_message_passing(fuse_closing=)`).
        self.affinity_tail = True

    @property
    def out_features(self) -> int:
        return self.h_dim * (2 + len(self.hyper_scales))

    def noise_shapes(self, B: int, N: int) -> List[Tuple[int, int, int]]:
        """(B,E,K) of the uniforms each module draws per message-passing round, pairwise first."""
        return noise_shapes(self.interaction, self.interaction_hyper, self.hyper_scales, B, N)

    def forward(self, f: Tensor, noise_u: Optional[Sequence] = None, advance=None, n_agents=None
                ) -> Tuple[Tensor, Optional[Tensor]]:
        """``noise_u``: optional list with one entry per module (pairwise first), each a tensor or a
        list of ``nmp_layers`` tensors; default draws as the modules do (reference order).
        ``advance`` = (counter, n): add n to the device Philox counter at the START of this forward
        (used by the captured graph so that every replay draws fresh noise).
        ``n_agents`` (optional; INTEGRATION.md, "Ragged batches"): one count per scene, 1 <= n_b <= N — the first n_b
        rows of scene b are real agents, the rest is finite padding.  The valid rows of the module columns of ``final``
        and the valid block of ``new_H`` are what the block computes for each scene alone at its own size; padded
        positions are zeros (the first D columns of ``final`` stay the copy of f).  The noise keeps its padded shapes.
        Under autograd only with `set_ragged_training(True)` ("Ragged batches", Training)."""
        ops._req(f, "f", (None, None, self.h_dim), ops._ACT_DTYPES)
        B, N, D = f.shape
        S = len(self.hyper_scales)
        sub = _mods.subset_of(n_agents, f, _needs_grad(self, f), listall=any(m.listall for m in self.interaction_hyper))
        if sub is not None:
            return self._forward_subset(f, noise_u, advance, sub, _needs_grad(self, f))
        counts = ragged_counts(n_agents, f, **ragged_grad_refusals(_needs_grad(self, f), N),
                               listall=any(m.listall for m in self.interaction_hyper))
        if _needs_grad(self, f):
            if f.dtype == torch.bfloat16:
                # bf16 storage under autograd: the fp32 training path on the up-cast features, results back in bf16
                # (see MS_HGNN_batch._forward_autograd) — config 4 can train, with fp32 intermediates
                if advance:
                    ops.counter_add(advance[0], advance[1])
                out, new_H = multiscale_autograd(self.interaction, list(self.interaction_hyper), self.hyper_scales,
                                                 f.float(), noise_u, counts)
                return out.to(torch.bfloat16), (None if new_H is None else new_H.to(torch.bfloat16))
            if f.dtype != torch.float32:
                raise NotImplementedError("activations must be fp32 or bf16")
            # training: ONE autograd node for the 1+S modules (grouped fused forward, grouped HIP backward);
            # the concat is an ordinary differentiable torch.cat
            if advance:
                ops.counter_add(advance[0], advance[1])
            return multiscale_autograd(self.interaction, list(self.interaction_hyper), self.hyper_scales, f, noise_u,
                                       counts)
        if noise_u is None:
            noise_u = draw_noise(self.noise_shapes(B, N), self.interaction.nmp_layers, f.device)
        elif len(noise_u) != 1 + S:
            raise ValueError(f"noise_u: need {1 + S} entries (pairwise + one per scale)")
        facts = route.StageFacts(grouped=self.grouped, latency_form=self.affinity_tail,
                                 capturing=f.is_cuda and torch.cuda.is_current_stream_capturing(), embed=False,
                                 may_defer=True)
        r = graph_route(S, B, N, D, facts, ragged=counts is not None)
        _, Hs, new_H, job, join, final, cols = build_graphs(r, f, self.hyper_scales, width=self.out_features,
                                                            advance=advance, counts=counts)
        mods = [self.interaction, *self.interaction_hyper]
        if self.grouped:
            # every stage of the 1+S modules in ONE launch: launches always carry enough workgroups
            # to fill the chip, and nothing depends on how streams map to hardware queues
            # (latency form — `affinity_tail` — also folds the closing MLPs into the aggregation launch: 4 launches)
            run_message_passing(mods, [f] * (1 + S), [None, *Hs], list(noise_u), cols, join=join, affinity=job,
                                fuse_closing=r.ask_closing, n_agents=counts)
        else:
            for m, H, u, c in zip(mods, [None, *Hs], noise_u, cols):
                run_message_passing([m], [f], [H], [u], [c], n_agents=counts)
        return final, new_H

    def _forward_subset(self, f: Tensor, noise_u, advance, sub: "ops.AgentSubset", grad: bool):
        """``n_agents`` = an `ops.AgentSubset` ("Agents missing anywhere"): ONE launch compacts f and the
        noise tensors of every module and round into scratch, the block's ragged forward runs on them as with
        ``n_agents=<counts>``, ONE launch expands ``final`` — at its full width, so its first D columns are f at valid
        rows and zeros elsewhere — and the scale blocks of ``new_H``.  Invalid rows of f are never read."""
        B, N, _ = f.shape
        S = len(self.hyper_scales)
        if any(s > N for s in self.hyper_scales):
            raise RuntimeError("selected index k out of range")
        if noise_u is not None and len(noise_u) != 1 + S:
            raise ValueError(f"noise_u: need {1 + S} entries (pairwise + one per scale)")
        rounds = self.interaction.nmp_layers
        shapes = self.noise_shapes(B, N)
        # module-major, as `draw_noise` draws: every round of the pairwise module, then scale by scale
        us = [_mods.subset_noise(None if noise_u is None else noise_u[i], shp, rounds, f.device)
              for i, shp in enumerate(shapes)]
        kinds = [ops.REMAP_PAIR_ROWS] + [None if s == N else ops.REMAP_NODE_ROWS for s in self.hyper_scales]
        items: list = []
        uc = [_mods.remap_noise(u, k, items) for u, k in zip(us, kinds)]
        uc = None if all(u is None for u in uc) else uc
        if grad:
            if items:
                ops.remap_rows(items, sub.order)
            (fc,) = _mods._Remap.apply(sub, False, (ops.REMAP_NODE_ROWS,), f)
            outc, Hc = self.forward(fc, uc, advance, n_agents=sub.compacted)
            (final,) = _mods._Remap.apply(sub, True, (ops.REMAP_NODE_ROWS,), outc)
            back = []
        else:
            fc = torch.empty_like(f)
            ops.remap_rows([(f, fc, ops.REMAP_NODE_ROWS)] + items, sub.order)
            outc, Hc = self.forward(fc, uc, advance, n_agents=sub.compacted)
            final = torch.empty_like(outc)
            back = [(outc, final, ops.REMAP_NODE_ROWS)]
        new_H = None
        if Hc is not None:
            new_H, e0 = torch.empty_like(Hc), 0
            for s in self.hyper_scales:      # the scale blocks of cat(H_s, dim=1): E = 1 row where s == N, else N rows
                E = 1 if s == N else N
                back.append(_mods.incidence_item(Hc[:, e0:e0 + E], new_H[:, e0:e0 + E]))
                e0 += E
        if back:
            ops.remap_rows(back, sub.slot)
        return final, new_H
