"""Backward of the MS-HGNN modules on HIP, behind torch.autograd.

`train_hyper_nba.py:116` back-propagates through `MS_HGNN_oridinary` / `MS_HGNN_hyper`.  The forward
of the drop-in modules is the fused matrix-core path; when a gradient is needed a call goes through
`MSHGNNFunction`: forward = that same fused path (keeping only the node features entering each
message-passing round and the `dist` each round sampled, which carries the Gumbel noise), backward =
this file — the chain rule of model/MS_HGNN_batch.py:41-53, 116-141, 247-268, 357-370 written out stage
by stage for SEVERAL modules at once, every stage one grouped launch of libgroupnet_hip.so:

  * all dense contractions (re-computation of hidden activations, dX = dY W, dW = dY^T X with the bias
    gradient as a side output) are problems of `gn_gemm_grouped_f32` — fp32 matrix cores, many problems
    per launch; every weight gradient of a round goes into ONE launch at the end of the round;
  * the K typed MLPs of the aggregation are handled as one wide layer (hidden (rows, K*128)) plus
    `gn_typed_bwd_f32`;
  * `gn_gumbel_bwd_f32`, `gn_node2edge_bwd_f32` for the two non-GEMM stages; gather and scatter are each
    other's adjoints and reuse the forward kernels.

A round j of a module is two blocks: x_j --node2edge_j, edge MLP_j--> (ef_j, dist_j) and
(ef_j, x_j) --edge2node_j, MLP--> x_{j+1} (or node_feat).  `nmp_layers > 1` (:186-194, :432-440) is
the same two blocks repeated, walked backwards.  Which forms a round takes is `route.backward_round_route`'s
answer; `round_backward` follows it through the steps below it, each a function over the modules' `_RoundState`s.

A ragged batch (``n_agents`` under autograd, `MS_HGNN_batch.set_ragged_training`): the traces carry the forward's counts
and the same chain rule runs with four changes ("Ragged training") — the incoming gradients zeroed at padded
positions (`modules_backward`), 1/n_b for 1/N and the unordered pair rows with a padded end zeroed
(`_edge2node_backward`), and the count-aware pooling backward gn_node2edge_bwd_ragged_grouped_f32 (`_pooling_backward`).

The deterministic mode (`MS_HGNN_batch.set_deterministic`; DESIGN.md, "Deterministic training"): the same stages, with the
two that sum in an order of their own making replaced by their ordered forms — every `GemmBatch.run` goes to
gn_gemm_grouped_det_f32 and the pooling backward to gn_node2edge_bwd_det_grouped_f32 (full-batch and ragged).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib, ops, route, weights
from ._lib import addr, check, load, stream_handle
from .MS_HGNN_batch import _GUMBEL_TAU, deterministic
from .weights import _HID, _LGF_LD

Tensor = torch.Tensor
D = ops.FEAT


class GemmBatch:
    """Collects GEMM problems (2-D row-major views, unit column stride) and runs them as grouped launches."""

    def __init__(self):
        self.descs: List[_lib.GemmDesc] = []
        self.keep: List[Tensor] = []
        self.device = None

    def add(self, A: Tensor, Bm: Tensor, C: Tensor, tA=False, tB=False, bias=None, mask=None, relu=False, alpha=1.0,
            beta=0.0, rs: Optional[Tensor] = None, colsum: Optional[Tensor] = None, accum=False, tC=False) -> Tensor:
        for t in (A, Bm, C) + ((mask,) if mask is not None else ()):
            if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or t.dtype != torch.float32:
                raise ValueError("gemm: 2-D fp32 views with unit column stride")
        M, K = (A.shape[1], A.shape[0]) if tA else (A.shape[0], A.shape[1])
        K2, N = (Bm.shape[1], Bm.shape[0]) if tB else (Bm.shape[0], Bm.shape[1])
        if K != K2 or tuple(C.shape) != ((N, M) if tC else (M, N)) or (mask is not None and tuple(mask.shape) != (M, N)):
            raise ValueError(f"gemm: ({M},{K}) x ({K2},{N}) -> {tuple(C.shape)}")
        if rs is not None and (rs.dim() != 1 or rs.shape[0] != A.shape[0]):
            raise ValueError("gemm: rs scales the stored rows of A")
        if colsum is not None and (not tA or colsum.numel() != M or not colsum.is_contiguous()):
            raise ValueError("gemm: colsum needs transA and M contiguous entries")
        flags = (_lib.GEMM_TRANS_A if tA else 0) | (_lib.GEMM_TRANS_B if tB else 0) | \
                (_lib.GEMM_RELU if relu else 0) | (_lib.GEMM_ACCUM if accum else 0) | (_lib.GEMM_TRANS_C if tC else 0)
        if tC and not accum:
            raise ValueError("gemm: tC (write the product transposed) exists for accumulate mode only")
        ld = lambda t: max(t.stride(0), t.shape[1])
        self.descs.append(_lib.GemmDesc(A=A.data_ptr(), B=Bm.data_ptr(), C=C.data_ptr(), bias=addr(bias), mask=addr(mask),
                                        rs=addr(rs), colsum=addr(colsum), M=M, N=N, K=K, lda=ld(A), ldb=ld(Bm), ldc=ld(C),
                                        ldmask=0 if mask is None else ld(mask), rs_ld=0 if rs is None else rs.stride(0),
                                        flags=flags, alpha=float(alpha), beta=float(beta)))
        self.keep += [t for t in (A, Bm, C, bias, mask, rs, colsum) if t is not None]
        self.device = A.device
        return C

    def run(self) -> None:
        if not self.descs:
            return
        if deterministic():
            self._run_ordered()
        else:
            arr = (_lib.GemmDesc * len(self.descs))(*self.descs)
            with torch.cuda.device(self.device):
                check(load().gn_gemm_grouped_f32(arr, len(self.descs), stream_handle()), "gn_gemm_grouped_f32")
        self.descs, self.keep = [], []

    def _run_ordered(self) -> None:
        """The deterministic mode (`MS_HGNN_batch.set_deterministic`): gn_gemm_grouped_det_f32, whose accumulate problems
        sum their K splits in a fixed order through a workspace.  Its size is the plan query's answer; it comes from
        torch's allocator (inside a capture: from the graph's pool, like every other temporary of a step).  A batch
        beyond the entry's GN_GEMM_DET_MAX problems goes in pieces: a chain that spans two of them continues from the sum
        the first left in the destination, which is the same order."""
        lib = load()
        for i in range(0, len(self.descs), _lib.GEMM_DET_MAX):
            part = self.descs[i:i + _lib.GEMM_DET_MAX]
            arr = (_lib.GemmDesc * len(part))(*part)
            ws, nbytes = None, 0
            if any(d.flags & _lib.GEMM_ACCUM for d in part):
                plan = _lib.GemmDetPlan()
                check(lib.gn_gemm_grouped_det_plan(arr, len(part), plan), "gn_gemm_grouped_det_plan")
                nbytes = plan.workspace_bytes
                ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                check(lib.gn_gemm_grouped_det_f32(arr, len(part), addr(ws), nbytes, stream_handle()),
                      "gn_gemm_grouped_det_f32")


def gemm(A: Tensor, Bm: Tensor, transA=False, transB=False, bias=None, mask=None, relu=False, alpha=1.0,
         out: Optional[Tensor] = None, beta=0.0) -> Tensor:
    """out (M,N) = beta*out + alpha*op(A) op(B) (+bias) (relu) (zeroed where mask <= 0) — one problem."""
    M = A.shape[1] if transA else A.shape[0]
    N = Bm.shape[0] if transB else Bm.shape[1]
    if out is None:
        out, beta = torch.empty((M, N), dtype=A.dtype, device=A.device), 0.0
    gb = GemmBatch()
    gb.add(A, Bm, out, transA, transB, bias, mask, relu, alpha, beta)
    gb.run()
    return out


def axpby(out: Tensor, a: Tensor, alpha=1.0, beta=0.0) -> Tensor:
    """out = alpha*a + beta*out on 2-D (possibly column-sliced) views."""
    assert out.shape == a.shape and out.stride(1) == 1 and a.stride(1) == 1
    with torch.cuda.device(a.device):
        check(load().gn_axpby2d_f32(addr(out), out.stride(0), addr(a), a.stride(0), a.shape[0], a.shape[1], float(alpha),
                                    float(beta), stream_handle()), "gn_axpby2d_f32")
    return out


def pairwise_incidence(B: int, N: int, device, dtype=torch.float32) -> Tensor:
    """The (B, N*N, N) incidence rel_rec + rel_send of the pairwise graph (model/MS_HGNN_batch.py:118,
    143-160): edge e = i*N + j has weight 1 on i and on j, 2 when i == j.  A constant; only the backward
    of node2edge materialises it."""
    e = torch.arange(N * N, device=device)
    H = torch.zeros(N * N, N, dtype=dtype, device=device)
    H[e, e % N] += 1
    H[e, e // N] += 1
    return H[None].expand(B, -1, -1).contiguous()


_pair_w_cache: Dict[tuple, Tensor] = {}


def _pair_row_weights(B: int, N: int, device) -> Tensor:
    """(B * N(N+1)/2) incidence weight of each unordered-pair row on its nodes: 2 on self-loops, else 1."""
    key = (B, N, str(device))
    w = _pair_w_cache.get(key)
    if w is None:
        i = torch.arange(N, device=device)
        one = torch.ones(ops.pair_count(N), dtype=torch.float32, device=device)
        one[i * N - (i * (i - 1)) // 2] = 2.0          # row of the pair (i, i)
        w = _pair_w_cache[key] = one.repeat(B).contiguous()
        if len(_pair_w_cache) > 16:
            _pair_w_cache.pop(next(iter(_pair_w_cache)))
    return w


class _Pool:
    """Zero-initialised scratch handed out in slices: every accumulate-by-atomics target of a round comes
    from one fill instead of one fill each."""

    def __init__(self, numel: int, device, buf: Optional[Tensor] = None):
        # (buf: a zeroed slice of a larger fill — the modules of a round share ONE fill)
        self.buf = torch.zeros(numel, dtype=torch.float32, device=device) if buf is None else buf
        self.used = 0

    def take(self, *shape: int) -> Tensor:
        n = 1
        for s in shape:
            n *= s
        n4 = (n + 3) // 4 * 4
        if self.used + n4 > self.buf.numel():
            return torch.zeros(shape, dtype=torch.float32, device=self.buf.device)
        out = self.buf[self.used:self.used + n].view(*shape)
        self.used += n4
        return out


class ModuleTrace:
    """What one module's fused forward keeps for its backward."""

    def __init__(self, mod, h: Tensor, H):
        self.mod = mod
        self.H = H.H if isinstance(H, ops.Incidence) else H      # dense (None: the pairwise graph)
        self.masks = None                    # `ops.IncidenceMasks` of H where `run_message_passing` ran the step on them
        self.counts = None                   # `ops.AgentCounts` where `run_message_passing` ran a ragged batch
        self.xs: List[Tensor] = [h]          # node features entering round j
        self.dists: List[Tensor] = []        # dist of round j (B,E,K)
        self.tails: List[dict] = []          # round j's closing MLP: {"x": cat(H^T feat, ori)/N, "hid": relu(layer 0)}
        self.n2e: List[dict] = []            # round j: {"x1" hidden of node2edge_start_mlp, "xp", "pq", "edges"}
        self.estage: List[dict] = []         # round j's edge MLP: {"z1", "z", "dh1", "lgf"}
        # what the backward leaves here for its later rounds
        self.pair_H: Optional[Tensor] = None     # `pairwise_incidence`, where a round walks the pairwise graph's ordered rows
        self.npar: Dict[int, int] = {}           # round j -> number of parameter elements of its layers


def _round_layers(mod, j: int):
    L = mod.nmp_layers - 1
    stage = mod.nmp_mlp_start if j == 0 else mod.nmp_mlps[2 * j - 1]
    tail = mod.nmp_mlp_end if j == L else mod.nmp_mlps[2 * j]
    return (mod.node2edge_start_mlp[j].layers, mod.attention_mlp[j].layers, stage, mod.edge_aggregation_list[j],
            tail.layers)


def _bwd_weights(mod, j: int) -> dict:
    """The concatenated weight matrices round j's backward GEMMs read (layout: `weights.backward_cat`), assembled
    from the parameters by ONE `PackPlan` launch (no torch.cat, capturable).  A backward is by definition part of a
    training step, where parameters may have been rewritten through `.data` without a version bump: the cache
    refreshes on every call."""
    _, (a0, _), st, agg, _ = _round_layers(mod, j)
    d, f = st.MLP_distribution.layers, st.MLP_factor.layers
    l0 = [m.layers[0] for m in agg.agg_mlp]
    l1 = [m.layers[1] for m in agg.agg_mlp]
    params = [a0.weight, a0.bias] + [p for l in (*d, *f, *l0, *l1) for p in (l.weight, l.bias)]
    return weights.cache(mod, ("bwd", j), always=True).get(params, lambda plan: weights.backward_cat(
        plan, a0, d, f, l0, l1))


def _arena_floats(npar: int, B: int, N: int, E: int, K: int) -> int:
    """fp32 elements of the zeroed scratch one module takes from the round's arena (`_Pool`), a multiple of 64."""
    n = (npar                       # every parameter gradient of the round
         + 2 * B * N * D            # dxp, dpq
         + B * E * (2 * K + 4)      # ef (leading dimension K rounded up to 4) and def
         + B * E * D                # deo
         # room for what the gradient images hold beyond their parameters (MLP_distribution | MLP_factor layer 1 as
         # (32, 256), the typed MLPs' output bias in Kp rows) and for the rounding of each take to 4 elements; a take
         # beyond the arena gets a fill of its own (`_Pool.take`)
         + B * E * D + 4096)
    return (n + 63) // 64 * 64


class _RoundState:
    """One module's part of one backward round: what the steps of `round_backward` read and what each of them fills.
    Tensors are 2-D views: BN = B*N node rows, R = B*E edge rows (E = N(N+1)/2 pair rows where `sym`)."""
    __slots__ = (
        # the constructor — the round's inputs and constants:
        "x", "x2", "H", "masks", "sym",         # x_j (B,N,D) and as (BN,D); dense incidence (None where sym) and its masks
        "counts", "inv_n",      # ragged batch: its `ops.AgentCounts` and 1/n_b per node row (BN,); else None and None
        "B", "N", "E", "K", "Kp", "R", "BN",    # Kp: K rounded up to 4, the leading dimension of ef
        "s0", "s1", "a0", "a1", "i", "d", "f", "agg", "e0", "e1",      # the round's layers (`_round_layers`)
        "tw", "w2", "b2",                       # `_bwd_weights`; attention layer 1 as a vector and its bias
        "agg2", "y1",                           # the closing MLP's input cat(H^T feat, ori)/N and hidden layer, as kept
        "dist", "g_y", "g_d",                   # (R', K) dist of the ordered rows; incoming gradients (None: not used)
        "pool_n", "dx",     # `_arena_floats`; d x_j (BN,D): None until `_edge2node_backward` or `_pooling_backward`
        # `round_backward`, from the round's one zero fill:
        "pool",
        # `_forward_activations`:
        "x1", "xp", "pq", "edges", "z1", "z", "dh1", "lgf",
        # `_edge_weights`:
        "ef", "def_",                           # (R,Kp) ef per edge row; (R,K) its gradient, zero where the module is not live
        # `_edge2node_backward` (live modules only):
        "eo2", "Hc", "dy1", "da", "dfeat", "T", "deo",
        # `_edge_mlp_backward`:
        "dlgf", "dd1", "dz", "dz1", "dedges",
        # `_pooling_backward`:
        "dxp", "dpq", "dx1")

    def __init__(self, t: ModuleTrace, j: int, pair_rows: bool, g_y: Optional[Tensor], g_d: Optional[Tensor]):
        mod, x = t.mod, t.xs[j]
        B, N, _ = x.shape
        # The pairwise graph is symmetric: the ordered edges (i,j) and (j,i) pool the same feature and feed
        # the same typed MLP, so (as in the forward) every per-edge stage runs on the N(N+1)/2 unordered
        # pairs; only dist (its own Gumbel noise per ordered edge) stays ordered.
        self.sym, self.H = t.H is None and pair_rows, t.H
        if t.H is None and not self.sym:
            if t.pair_H is None:
                t.pair_H = pairwise_incidence(B, N, x.device, x.dtype)
            self.H = t.pair_H
        E = ops.pair_count(N) if self.sym else self.H.shape[1]
        K = mod.edge_types
        (self.s0, self.s1), (self.a0, self.a1), st, self.agg, (self.e0, self.e1) = _round_layers(mod, j)
        if j not in t.npar:
            t.npar[j] = sum(p.numel() for m in (mod.node2edge_start_mlp[j], mod.attention_mlp[j], st, self.agg,
                                                nn.ModuleList([self.e0, self.e1])) for p in m.parameters())
        self.x, self.x2, self.masks = x, x.reshape(B * N, D), t.masks
        self.counts, self.inv_n = t.counts, None
        self.B, self.N, self.E, self.K, self.Kp, self.R, self.BN = B, N, E, K, (K + 3) // 4 * 4, B * E, B * N
        self.i, self.d, self.f = st.init_MLP.layers, st.MLP_distribution.layers, st.MLP_factor.layers
        self.tw = _bwd_weights(mod, j)
        self.w2, self.b2 = _w(self.a1)[0], _b(self.a1)
        self.agg2, self.y1 = t.tails[j]["x"], t.tails[j]["hid"]
        self.dist = t.dists[j].reshape(-1, K)
        self.g_y = None if g_y is None else g_y.reshape(B * N, -1).contiguous()
        self.g_d = None if g_d is None else g_d.reshape(-1, K).contiguous()
        self.pool_n = _arena_floats(t.npar[j], B, N, E, K)
        self.dx = None

    def new(self, *shape: int) -> Tensor:
        return torch.empty(shape, dtype=torch.float32, device=self.x.device)


def _w(lin) -> Tensor:
    return lin.weight.detach()


def _b(lin) -> Tensor:
    return lin.bias.detach()


def _each(S: List[_RoundState], gb: GemmBatch):
    """The modules of one stage: the problems the loop body adds for them run as ONE grouped launch when the loop ends."""
    yield from S
    gb.run()


def _wgrad(gb: GemmBatch, grads: dict, pool: _Pool, lin, dY: Tensor, X: Tensor) -> None:
    """dW = dY^T X of one linear layer, its bias gradient as the side output, both from the zeroed pool."""
    grads[lin.weight] = gb.add(dY, X, pool.take(*lin.weight.shape), tA=True, accum=True,
                               colsum=grads.setdefault(lin.bias, pool.take(*lin.bias.shape)))


def _forward_activations(S: List[_RoundState], gb: GemmBatch, traces: Sequence[ModuleTrace], j: int, kept: bool) -> None:
    """x1 .. lgf of round j: taken over from what the fused forward kept (training mode writes these on request), or
    re-computed.  The forward runs the pairwise module on unordered pairs; if this backward has to use ordered edge rows
    (N too large for the per-scene node2edge backward), its edge-row activations do not serve."""
    if kept:
        for c, tr in zip(S, traces):
            a, e = tr.n2e[j], tr.estage[j]
            c.x1, c.xp, c.pq, c.edges = a["x1"], a["xp"].view(-1, D), a["pq"].view(-1, D), a["edges"].view(c.R, D)
            c.z1, c.z, c.dh1, c.lgf = e["z1"], e["z"], e["dh1"], e["lgf"]
        return
    for c in _each(S, gb):
        c.x1 = gb.add(c.x2, _w(c.s0), c.new(c.BN, 256), tB=True, bias=_b(c.s0), relu=True)
    for c in _each(S, gb):
        c.xp = gb.add(c.x1, _w(c.s1), c.new(c.BN, D), tB=True, bias=_b(c.s1))
    # attention layer 0 on cat(x'_n, e0_e), split by linearity: P = W[:, :64] x' + b, Qn = W[:, 64:] x'
    for c in _each(S, gb):
        c.pq = gb.add(c.xp, c.tw["Wpq"], c.new(c.BN, D), tB=True, bias=c.tw["bpq"])
    edges = ops.node2edge_grouped([(c.xp.view(c.B, c.N, D), c.pq.view(c.B, c.N, D), c.H, c.w2, c.b2, c.sym) for c in S])
    for c, e in zip(S, edges):
        c.edges = e.view(c.R, D)
    for c in _each(S, gb):
        c.z1 = gb.add(c.edges, _w(c.i[0]), c.new(c.R, 128), tB=True, bias=_b(c.i[0]), relu=True)
    for c in _each(S, gb):
        c.z = gb.add(c.z1, _w(c.i[1]), c.new(c.R, D), tB=True, bias=_b(c.i[1]))
    # hidden layers of MLP_distribution | MLP_factor side by side, then (logits | factor pre-activation)
    for c in _each(S, gb):
        c.dh1 = gb.add(c.z, c.tw["Wd0"], c.new(c.R, 256), tB=True, bias=c.tw["bd0"], relu=True)
    for c in _each(S, gb):
        c.lgf = gb.add(c.dh1, c.tw["Wd1"], c.new(c.R, _LGF_LD), tB=True, bias=c.tw["bd1"])


def _edge_weights(S: List[_RoundState]) -> None:
    """ef per edge row; for pair rows ef_ij + ef_ji (self-loop rows not doubled: the typed backward works with
    dfeat = the pair gather of d(H^T feat), which carries the self-loop's 2).  Its leading dimension is padded to a
    multiple of 4, zero-filled: the GEMMs reading ef stay on the vector path."""
    for c in S:
        c.ef = c.pool.take(c.R, c.Kp)
        with torch.cuda.device(c.x.device):
            check(load().gn_gumbel_ef_f32(addr(c.dist), addr(c.lgf), addr(c.ef), c.R, c.K, _LGF_LD, c.N if c.sym else 0,
                                          1.0, c.Kp, stream_handle()), "gn_gumbel_ef_f32")
        c.def_ = c.pool.take(c.R, c.K)


def _edge2node_backward(S: List[_RoundState], gb: GemmBatch) -> None:
    """Back through edge2node + the closing MLP of the modules whose round output is used: def_ and the ori half of dx."""
    for c, eo in zip(S, ops.agg_gather_grouped([(c.x, c.H, c.sym, c.masks) for c in S])):
        c.eo2 = eo.view(c.R, D)
    for c in _each(S, gb):
        c.Hc = gb.add(c.eo2, c.tw["W1cat"], c.new(c.R, c.K * _HID), tB=True, bias=c.tw["b1cat"], relu=True)
    # cat(H^T feat, ori) / N and the closing MLP's hidden layer were kept by the forward (the fused scatter+MLP kernel
    # writes them on request: agg2, y1), so feat is not re-computed
    for c in _each(S, gb):
        c.dy1 = gb.add(c.g_y, _w(c.e1), c.new(c.BN, 128), mask=c.y1)
    # (a ragged batch: edge2node divided scene b by its own n_b — the rows of dy1 are scaled by 1/n_b instead of 1/N)
    for c in _each(S, gb):
        div = dict(alpha=1.0 / c.N) if c.counts is None else dict(rs=c.inv_n)
        c.da = gb.add(c.dy1, _w(c.e0)[:, :D], c.new(c.BN, D), **div)     # d(H^T feat)
        c.dx = gb.add(c.dy1, _w(c.e0)[:, D:], c.new(c.BN, D), **div)     # ori half of the cat
    dfeats = ops.agg_gather_grouped([(c.da.view(c.B, c.N, D), c.H, c.sym, c.masks) for c in S])    # adjoint of H^T feat
    for c, df in zip(S, dfeats):
        c.dfeat = df.view(c.R, D)
    # A ragged batch: the pair gather forms da_i + da_j, so a pair with ONE valid end carries a non-zero row, which
    # would reach T, def_, deo and the weight gradients: such rows become zero before anything reads them.  (The hyper
    # modules' H has zero rows e >= n_b and zero columns n >= n_b: their gather and scatter need nothing.)  From here on
    # every stage is row-wise or linear in its incoming gradient, up to the count-aware pooling backward.
    ragged_pairs = [(c.dfeat.view(c.B, c.E, D), ops.ZERO_SYM_PAIR_ROWS) for c in S if c.counts is not None and c.sym]
    if ragged_pairs:
        ops.zero_padding(ragged_pairs, S[0].counts)
    for c in _each(S, gb):
        c.T = gb.add(c.dfeat, c.tw["W2cat"], c.new(c.R, c.K * _HID))
    for c in S:
        with torch.cuda.device(c.x.device):
            check(load().gn_typed_bwd_f32(addr(c.T), addr(c.Hc), addr(c.ef), c.Kp, addr(c.dfeat), addr(c.tw["b2mat"]),
                                          addr(c.def_), c.R, c.K, _HID, stream_handle()), "gn_typed_bwd_f32")
    # (pair rows: the self-loop's eo = 2 ori, and the pair-form scatter below weighs every row once)
    # (K = K_types*128 is long and the output has few tiles: split K over workgroups, atomic accumulate)
    for c in _each(S, gb):
        c.deo = gb.add(c.T, c.tw["W1cat"], c.pool.take(c.R, D), accum=True,
                       rs=_pair_row_weights(c.B, c.N, c.x.device) if c.sym else None)
    # eo = H ori  ->  d ori += H^T d eo  (the scatter kernel with divisor 1; its ori half is unused)
    scs = ops.agg_scatter_grouped([(c.deo.view(c.B, c.E, D), c.H, c.x, c.sym, c.masks) for c in S], 1.0)
    for c, sc in zip(S, scs):
        axpby(c.dx, sc.view(c.BN, 2 * D)[:, :D], 1.0, 1.0)


def _edge2node_weight_grads(S: List[_RoundState], gb: GemmBatch, grads: dict) -> None:
    """The closing MLP's and the K typed MLPs' gradients of the live modules: one grouped launch."""
    for c in _each(S, gb):
        K, pool = c.K, c.pool
        _wgrad(gb, grads, pool, c.e1, c.g_y, c.y1)
        _wgrad(gb, grads, pool, c.e0, c.dy1, c.agg2)
        gW1, gb1 = pool.take(K * _HID, D), pool.take(K * _HID)
        gb.add(c.T, c.eo2, gW1, tA=True, accum=True, colsum=gb1)
        gb2 = gb.add(c.ef, c.dfeat, pool.take(c.Kp, D), tA=True, accum=True)     # rows >= K stay zero
        for k, m in enumerate(c.agg.agg_mlp):
            l0, l1 = m.layers
            grads[l0.weight], grads[l0.bias] = gW1[k * _HID:(k + 1) * _HID], gb1[k * _HID:(k + 1) * _HID]
            grads[l1.bias] = gb2[k]
            # dW2_k = sum_r ef[r,k] dfeat[r] (x) h_k[r]
            # (as (ef_k h_k)^T dfeat written transposed: 128-row tiles instead of half-empty 64-row ones)
            grads[l1.weight] = gb.add(c.Hc[:, k * _HID:(k + 1) * _HID], c.dfeat, pool.take(D, _HID), tA=True,
                                      accum=True, rs=c.ef[:, k], tC=True)


def _edge_mlp_backward(S: List[_RoundState], gb: GemmBatch) -> None:
    """Back through the Gumbel softmax (one grouped launch for all modules: these launches take ~14 us whatever their
    size) and the edge MLP: def_, g_d -> dedges."""
    arr = (_lib.GumbelBwdGroup * len(S))()
    for i, c in enumerate(S):
        c.dlgf = c.new(c.R, _LGF_LD)
        arr[i] = _lib.GumbelBwdGroup(dist=c.dist.data_ptr(), lgf=c.lgf.data_ptr(), def_=c.def_.data_ptr(),
                                     gdist=addr(c.g_d), dlgf=c.dlgf.data_ptr(), rows=c.R, K=c.K,
                                     sym_N=c.N if c.sym else 0)
    with torch.cuda.device(S[0].x.device):
        check(load().gn_gumbel_bwd_grouped_f32(arr, len(S), _LGF_LD, _GUMBEL_TAU, stream_handle()),
              "gn_gumbel_bwd_grouped_f32")
    for c in _each(S, gb):
        c.dd1 = gb.add(c.dlgf, c.tw["Wd1"], c.new(c.R, 256), mask=c.dh1)
    for c in _each(S, gb):
        c.dz = gb.add(c.dd1, c.tw["Wd0"], c.new(c.R, D))
    for c in _each(S, gb):
        c.dz1 = gb.add(c.dz, _w(c.i[1]), c.new(c.R, 128), mask=c.z1)
    for c in _each(S, gb):
        c.dedges = gb.add(c.dz1, _w(c.i[0]), c.new(c.R, D))


def _pooling_backward(S: List[_RoundState], gb: GemmBatch, grads: dict, grouped: bool) -> None:
    """Back through the attention-weighted pooling and the node MLP: dedges -> dx (added to the ori half where the
    module is live), with the gradients of attention layer 1 out of the node->edge kernel."""
    for c in S:
        c.dxp, c.dpq = c.pool.take(c.BN, D), c.pool.take(c.BN, D)
        grads[c.a1.weight], grads[c.a1.bias] = c.pool.take(1, 32), c.pool.take(1)
    with torch.cuda.device(S[0].x.device):
        if grouped:
            # every module in one launch (blockIdx.y = module): the pairwise module's 88 us and the hyper modules'
            # 24-41 us side by side instead of end to end
            arr = (_lib.N2EBwdGroup * len(S))()
            for i, c in enumerate(S):
                arr[i] = _lib.N2EBwdGroup(xp=c.xp.data_ptr(), pq=c.pq.data_ptr(), H=addr(c.H), w2=c.w2.data_ptr(),
                                          b2=c.b2.data_ptr(), dedges=c.dedges.data_ptr(), dxp=c.dxp.data_ptr(),
                                          dpq=c.dpq.data_ptr(), dw2=grads[c.a1.weight].data_ptr(),
                                          db2=grads[c.a1.bias].data_ptr(), E=c.E, sym=int(c.sym))
            if deterministic():
                # the ordered form, full-batch or ragged: one wave per (scene, module) adds a scene's edges in ascending
                # order, the 33 attention sums of every (module, scene) go through `partials` and are added in scene order
                partials = torch.empty(len(S) * S[0].B * 33, dtype=torch.float32, device=S[0].x.device)
                check(load().gn_node2edge_bwd_det_grouped_f32(
                    arr, len(S), S[0].B, S[0].N, None if S[0].counts is None else addr(S[0].counts.dev), addr(partials),
                    stream_handle()), "gn_node2edge_bwd_det_grouped_f32")
            elif S[0].counts is None:
                check(load().gn_node2edge_bwd_grouped_f32(arr, len(S), S[0].B, S[0].N, stream_handle()),
                      "gn_node2edge_bwd_grouped_f32")
            else:
                # a ragged batch: the softmax of a hyperedge ran over the scene's n_b nodes and the pairwise edges
                # exist only with both ends < n_b — the one stage where the count enters a kernel's arithmetic
                check(load().gn_node2edge_bwd_ragged_grouped_f32(arr, len(S), S[0].B, S[0].N, addr(S[0].counts.dev),
                                                                 stream_handle()), "gn_node2edge_bwd_ragged_grouped_f32")
        else:
            for c in S:
                check(load().gn_node2edge_bwd_f32(addr(c.xp), addr(c.pq), addr(c.H), addr(c.w2), addr(c.b2),
                                                  addr(c.dedges), addr(c.dxp), addr(c.dpq), addr(grads[c.a1.weight]),
                                                  addr(grads[c.a1.bias]), c.B, c.N, c.E, int(c.sym), stream_handle()),
                      "gn_node2edge_bwd_f32")
    for c in _each(S, gb):
        gb.add(c.dpq, c.tw["Wpq"], c.dxp, beta=1.0)
    for c in _each(S, gb):
        c.dx1 = gb.add(c.dxp, _w(c.s1), c.new(c.BN, 256), mask=c.x1)
    for c in _each(S, gb):
        if c.dx is None:
            c.dx = gb.add(c.dx1, _w(c.s0), c.new(c.BN, D))
        else:
            gb.add(c.dx1, _w(c.s0), c.dx, beta=1.0)


def _node2edge_weight_grads(S: List[_RoundState], gb: GemmBatch, grads: dict) -> None:
    """The edge MLP's, the attention layer 0's and the node MLP's gradients of every module: one grouped launch."""
    for c in _each(S, gb):
        K, pool = c.K, c.pool
        # MLP_distribution | MLP_factor: gradients of the side-by-side matrices, handed out as views
        gWd1, gbd1 = pool.take(_LGF_LD, 256), pool.take(_LGF_LD)
        gb.add(c.dlgf, c.dh1, gWd1, tA=True, accum=True, colsum=gbd1)
        grads[c.d[1].weight], grads[c.f[1].weight] = gWd1[:K, :128], gWd1[K:K + 1, 128:]
        grads[c.d[1].bias], grads[c.f[1].bias] = gbd1[:K], gbd1[K:K + 1]
        gWd0, gbd0 = pool.take(256, D), pool.take(256)
        gb.add(c.dd1, c.z, gWd0, tA=True, accum=True, colsum=gbd0)
        grads[c.d[0].weight], grads[c.f[0].weight] = gWd0[:128], gWd0[128:]
        grads[c.d[0].bias], grads[c.f[0].bias] = gbd0[:128], gbd0[128:]
        _wgrad(gb, grads, pool, c.i[1], c.dz, c.z1)
        _wgrad(gb, grads, pool, c.i[0], c.dz1, c.edges)
        ga0 = pool.take(32, 2 * D)                               # the (32,128) layout of attention layer 0
        gb.add(c.dpq[:, :32], c.xp, ga0[:, :D], tA=True, accum=True, colsum=grads.setdefault(c.a0.bias, pool.take(32)))
        gb.add(c.dpq[:, 32:], c.xp, ga0[:, D:], tA=True, accum=True)
        grads[c.a0.weight] = ga0
        _wgrad(gb, grads, pool, c.s1, c.dxp, c.x1)
        _wgrad(gb, grads, pool, c.s0, c.dx1, c.x2)


def round_backward(traces: Sequence[ModuleTrace], j: int, g_ys: Sequence[Optional[Tensor]],
                   g_dists: Sequence[Optional[Tensor]], grads: Dict[nn.Parameter, Tensor]) -> List[Tensor]:
    """Back through round j of several modules at once (same B and N: `run_message_passing` groups no others).

    g_ys[i] = gradient w.r.t. the output of round j's edge2node + MLP block (node_feat for the last round),
    g_dists[i] = gradient w.r.t. dist_j (the returned `factors` for round 0), either may be None.
    Adds the parameter gradients to `grads`, returns d x_j per module.

    A ragged batch (the traces carry the forward's `ops.AgentCounts`; DESIGN.md, "Ragged training"): the chain rule is
    the same, with the incoming gradients zero at padded positions (`modules_backward` sees to the caller's; the d x an
    earlier round receives from a later one is zero at rows n >= n_b already — there it is a sum of the ori half, a GEMM
    on rows of dy1 that are zero because the incoming rows are, of the scatter, which meets a padded node only through
    zero columns of H or through pair rows that `_edge2node_backward` zeroed, and of the node MLP's backward on rows of
    dxp and dpq that the count-aware pooling backward never writes), 1/n_b for 1/N, the unordered pair rows with a padded
    end zeroed, and the count-aware pooling backward.  d x_j comes back with rows n >= n_b exactly zero."""
    counts = traces[0].counts
    # (the deterministic mode: the route refuses an N beyond the ordered pooling backward before anything is launched)
    det = dict(deterministic=True) if deterministic() else {}
    rt = route.backward_round_route(traces[0].xs[j].shape[1], tuple(t.H is None for t in traces), counts is not None, **det)
    S = [_RoundState(t, j, rt.pair_rows, g_y, g_d) for t, g_y, g_d in zip(traces, g_ys, g_dists)]
    dev = S[0].x.device
    if counts is not None:
        # 1 / n_b per node row, from the device counts (no host read; an empty slot's rows are zero anyway)
        inv_n = counts.dev.clamp(min=1).to(torch.float32).reciprocal().repeat_interleave(S[0].N)
        for c in S:
            c.inv_n = inv_n
    # one zero fill for the accumulate-by-atomics targets of every module of the round
    arena = torch.zeros(sum(c.pool_n for c in S), dtype=torch.float32, device=dev)
    off = 0
    for c in S:
        c.pool = _Pool(c.pool_n, dev, arena[off:off + c.pool_n])
        off += c.pool_n
    gb = GemmBatch()
    with torch.no_grad():
        _forward_activations(S, gb, traces, j, rt.kept)
        _edge_weights(S)
        live = [c for c in S if c.g_y is not None]
        if live:
            _edge2node_backward(live, gb)
            _edge2node_weight_grads(live, gb, grads)
        _edge_mlp_backward(S, gb)
        _pooling_backward(S, gb, grads, rt.n2e_grouped)
        _node2edge_weight_grads(S, gb, grads)
    return [c.dx.view(c.B, c.N, D) for c in S]


def modules_backward(traces: Sequence[ModuleTrace], g_nfs: Sequence[Optional[Tensor]],
                     g_facs: Sequence[Optional[Tensor]]) -> Tuple[List[Tensor], Dict[nn.Parameter, Tensor]]:
    """Gradients of (node_feat, factors) of several modules (same nmp_layers) w.r.t. their h_states and
    parameters: the rounds walked backwards, each round grouped over the modules.
    A ragged batch: the outputs at padded positions are constants (zeros), so whatever the caller's loss put into the
    gradients there is dropped — in COPIES (the caller's tensors are never written), all of them in one launch."""
    L = traces[0].mod.nmp_layers - 1
    grads: Dict[nn.Parameter, Tensor] = {}
    counts = traces[0].counts
    if counts is not None:
        g_nfs, g_facs, items, single = list(g_nfs), list(g_facs), [], []
        for i, t in enumerate(traces):
            if g_nfs[i] is not None:
                g_nfs[i] = g_nfs[i].clone(memory_format=torch.contiguous_format)
                items.append((g_nfs[i], ops.ZERO_NODE_ROWS))
            if g_facs[i] is not None and g_facs[i].shape[1] != 1:      # (the single row of a scale-N module is valid)
                g_facs[i] = g_facs[i].clone(memory_format=torch.contiguous_format)
                items.append((g_facs[i], ops.ZERO_PAIR_ROWS if t.H is None else ops.ZERO_EDGE_ROWS))
            elif g_facs[i] is not None and counts.admits_empty:
                # ... except in an EMPTY slot, where the forward zeroed it (`ops.zero_empty_scenes`): a constant too
                g_facs[i] = g_facs[i].clone(memory_format=torch.contiguous_format)
                single.append(g_facs[i])
        ops.zero_padding(items, counts)
        if single:
            ops.zero_empty_scenes(single, counts)
    g_ys = list(g_nfs)
    for j in range(L, -1, -1):
        g_ds = list(g_facs) if j == 0 else [None] * len(traces)
        g_ys = round_backward(traces, j, g_ys, g_ds, grads)
    return g_ys, grads


class MSHGNNFunction(torch.autograd.Function):
    """Several modules on their inputs: forward = the grouped fused HIP path, backward = `modules_backward`.

    apply(mods, Hs, noises, counts, h_0..h_{n-1}, *params) -> (nf_0, fac_0, nf_1, fac_1, ...).  ``Hs``: per module None
    (the pairwise graph), a dense tensor or an `ops.Incidence`; where `run_message_passing` decides for the mask form it
    leaves the masks on the traces, and the backward reads them there.  ``counts``: None, or the `ops.AgentCounts` of a
    ragged batch (``Hs`` are then the ragged incidences); the traces carry them to the backward the same way."""

    @staticmethod
    def forward(ctx, mods, Hs, noises, counts, *tensors):
        from . import MS_HGNN_batch as M
        n = len(mods)
        hs, params = tensors[:n], tensors[n:]
        traces = [ModuleTrace(m, h.detach(), H) for m, h, H in zip(mods, hs, Hs)]
        with torch.no_grad(), M.training_call():     # a training step: packed-weight caches are not trusted
            res = M.run_message_passing(list(mods), [t.xs[0] for t in traces], list(Hs), list(noises), [None] * n,
                                        traces=traces, n_agents=counts)
        # `factors` is an output of this node AND what the backward reads as the first dist: kept as the tensor itself it
        # would close a cycle ctx -> trace -> output -> grad_fn -> ctx, and the whole autograd graph — the parameters'
        # AccumulateGrad nodes with the stream they were made on — would outlive the step until a gc pass
        for t in traces:
            t.dists = [d.detach() for d in t.dists]
        ctx.traces, ctx.params, ctx.n = traces, params, n
        # the backward reads the LIVE weights (and re-packs them): remember which versions the activations belong to
        ctx.param_key = M._param_key(params)
        out = []
        for nf, fac in res:
            out += [nf, fac]
        return tuple(out)

    @staticmethod
    def backward(ctx, *gs):
        from .MS_HGNN_batch import _param_key
        if _param_key(ctx.params) != ctx.param_key:
            raise RuntimeError("one of the parameters of an MS-HGNN module was modified in place between the forward and "
                               "this backward (e.g. an optimizer step before backward()): the saved activations belong "
                               "to the old weights.  torch's own autograd raises here too.")
        n = ctx.n
        g_nfs = [None if g is None else g.contiguous() for g in gs[0::2]]
        g_facs = [None if g is None else g.contiguous() for g in gs[1::2]]
        # a module none of whose outputs is used downstream contributes nothing
        live = [i for i in range(n) if g_nfs[i] is not None or g_facs[i] is not None]
        dhs: List[Optional[Tensor]] = [None] * n
        grads: Dict[nn.Parameter, Tensor] = {}
        if live:
            d, grads = modules_backward([ctx.traces[i] for i in live], [g_nfs[i] for i in live],
                                        [g_facs[i] for i in live])
            for i, dh in zip(live, d):
                dhs[i] = dh
        return (None, None, None, None) + tuple(dhs) + tuple(grads.get(p) for p in ctx.params)
