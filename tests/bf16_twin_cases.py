"""Test helper: the bf16 twins (`gn_*_bf16`) element by element (no GPU needed to import).

Every comparison of a twin with a reference in the suite was a whole-tensor gate, max|twin - ref| <= 8e-3 max|ref|
(`OLD_GATE`).  Correct rounding noise fills half of it, so a precision flaw of a few 1e-3 of the LARGEST element, or any
flaw confined to small elements, passes.  This module holds two instruments that take nothing from the code under test:

A. `emulate(case, Arith(...))`: every stage restated from the same bf16-representable inputs and the module's weights
   rounded to bf16, written out as products and sums in float64, rounded to bf16 (round to nearest even) exactly where
   the twin stores or re-feeds a value in bf16.  Only the PLACEMENT of these roundings is read from the kernels
   (groupnet_amd/csrc/gn_mlp_bf16.hpp):
     * operands (inputs, weights) and every hidden activation that feeds a matrix-core layer; biases stay fp32 and start
       the fp32 accumulator; the packed ReLU runs behind the rounding, which is the same function as rounding behind it;
     * node stage: x' is stored in bf16 and that value feeds the pq layer;
     * edge head: z feeds both heads in bf16; logits and the factor pre-activation stay fp32 through the Gumbel softmax
       and the sigmoid; `dist` is stored in bf16, factor * dist in fp32;
     * typed aggregation, one row block per wave: feat = sum_k ef_k (W2k bf16(relu(W1k x + b1k)) + b2k), an fp32 FMA per
       type; TWO row blocks per wave (GN_AGG_RB2 = 1): ef_k >= 0 is applied BEFORE the rounding, feat = sum_k W2k
       bf16(relu(ef_k (W1k x + b1k))) + sum_k ef_k b2k; gathered rows (H ori, ori_i + ori_j) are fp32 sums rounded once;
     * scene form: A'_n = W1k ori_n + b1k / 2 stays fp32 (an LDS stage), S_n = sum_j ef relu(A'_n + A'_j) is an fp32 VALU
       sum rounded to bf16 as the operand of W2k, the b2 term is c_n b2k with c_n = sum_j ef;
     * closing MLP: the fused-scatter input cat(H^T feat, ori) / N is an fp32 sum rounded once.
   Beside every pre-rounding value `pre` the emulation carries a slack `s` (see `Arith`), and THE RULE is: every element
   of the twin's output is the rounding (bf16, or fp32 for factor * dist) of some value in [pre - s, pre + s].
   Where the worst-case propagation of that slack through a RE-FED bf16 value is wider than the old gate, the value is
   taken where the twin stores it (pq on the stored x': `node_emul`), or the chain in front of it is made exact (the edge
   head, held in two halves: EDGE_CASES); every condition and every named flaw is asserted in every case.
B. `probe_eval(...)`: the same stages with weights and inputs on which nothing rounds, so that the float64 result is THE
   result of every correct evaluation, bit for bit, on bf16 storage and on all three matrix paths of fp32 storage.

tests/test_bf16_twins_cpu.py holds the conditions on the references, tests/test_bf16_twins_gpu.py runs the kernels.
"""
from __future__ import annotations

import functools
import zlib
from collections import namedtuple
from typing import Dict, Optional, Tuple

import torch

from bottleneck_cases import ROWS, X_FORM, bf16r, closing_case, closing_input, closing_mlp, form_id, pair_rows_incidence
from edge_type_cases import agg_module, edge_head, pair_index, pair_module, state_of
from launch_forms import pair_count
from oracle import ms_hgnn_oracle as O

U24 = 2.0 ** -24          # unit round-off of fp32
U23 = 2.0 ** -23
# The a-priori bound of a K-term fp32 sum in ANY order is (K - 1) u sum|terms|; the matrix cores' internal accumulation
# (how a k = 16 MFMA adds its 16 products to the accumulator) has not been measured here: twice the textbook bound.
MARGIN = 2.0
OLD_GATE = 8e-3           # tests/test_bf16_gpu.py TOL_ORACLE: the whole-tensor gate this module is held against
TAU = O.GUMBEL_TAU
EPS = O.GUMBEL_EPS
DRAWS = 16
FIRST_ORDER_MAX = 0.05    # the softmax slack is first order with a factor 2: the logits' slack / tau stays below this

# The named flaws, applied to the emulation (tests/test_bf16_twins_cpu.py: each must break the rule).
FLAWS = ("hid_trunc",      # hidden activations truncated to bf16 instead of rounded
         "out_trunc",      # a stored / re-fed result truncated
         "bias_late",      # the output bias added after the result was rounded (double rounding)
         "tile_bias",      # the second 32-wide output tile takes the first tile's bias
         "b2_drop",        # typed aggregation: b2 of one type dropped
         "ef_neighbour",   # typed aggregation: one type weight ef_k taken from the neighbouring edge
         "last_hidden",    # the last hidden column skipped
         "scene_row")      # scene form: one row reads the next scene's row
ROUTING_FLAWS = ("tile_bias", "b2_drop", "ef_neighbour", "last_hidden", "scene_row")

Out = namedtuple("Out", "pre s val fmt")      # pre-rounding value, slack, the emulation's own stored value, "bf16" | "fp32"


def bf16_trunc(t: torch.Tensor) -> torch.Tensor:
    """t (rounded to fp32: the accumulator) truncated to bf16, in t's dtype."""
    bits = t.to(torch.float32).contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(t.dtype)


def ulp_bf16(t: torch.Tensor) -> torch.Tensor:
    """The spacing of bf16 at |t| (0 at 0), float64."""
    a = t.detach().abs().double()
    _, e = torch.frexp(a)
    return torch.where(a == 0, torch.zeros_like(a), torch.ldexp(torch.ones_like(a), e.clamp(min=-125) - 8))


def f32r(t: torch.Tensor) -> torch.Tensor:
    return t.to(torch.float32).to(t.dtype)


def sum_slack(mag: torch.Tensor, quantum: torch.Tensor, n: int) -> torch.Tensor:
    """Slack of an fp32 sum of n bf16 VALUES (a gather: no products) with sum|terms| = mag, every term a multiple of
    `quantum` (a power of two: the smallest bf16 spacing among the terms).  Where mag < 2^24 quantum every partial sum, in
    any order, is a multiple of the quantum below 2^24 of them — an fp32 number: the sum is EXACT and its one rounding to
    bf16 is determined, ties included (two bf16 values of one binade add up to a tie half of the time; an a-priori slack
    there would call every such tie flippable).  Elsewhere the a-priori bound of `Arith.dot`."""
    return torch.where(mag < 2.0 ** 24 * quantum, torch.zeros_like(mag), MARGIN * (n + 1) * U24 * mag)


def _quantum(vals: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """min over the summed axis (-2 of vals (.., n, D), weight (.., E, n)) of ulp_bf16 of the nonzero members -> (.., E, D)."""
    u = ulp_bf16(vals)
    u = torch.where(u == 0, torch.full_like(u, float("inf")), u)
    q = torch.where(weight[..., :, :, None] != 0, u[..., None, :, :], torch.full_like(u[..., None, :, :], float("inf")))
    return q.min(-2).values.clamp(max=1.0)


class Arith:
    """The arithmetic of one evaluation of a stage.

    dtype float64 (the reference): sums are written out as products and sums and every value carries a slack `s`,
    derived from the reference alone:
      * a K-term dot product (a bias counts as a term): s = MARGIN (K + 1) 2^-24 sum|terms| — the a-priori bound of an fp32
        sum in any order, MARGIN for the matrix cores' internal accumulation;
      * an input x_i known only to within d_i adds |w_i| d_i.  A bf16-rounded value is uncertain exactly when it is
        FLIPPABLE — when [f(pre - s), f(pre + s)] (f = ReLU or identity) rounds to two different bf16 values — and then by
        the distance of those two values from the emulation's own, one bf16 ulp: |w| ulp_bf16 into everything it feeds;
      * everything else (`softmax`, `sigmoid` below) to first order with a factor 2.
    dtype float32: a real fp32 evaluation (torch matmul on the CPU) of the same chain, without slack: condition (a).
    rounding False: no rounding anywhere (the oracle's function).  flaw: one of FLAWS.  slack False (float64): the sums
    through torch.matmul and no slack — the flawed variants, of which only the stored values are read."""

    def __init__(self, dtype=torch.float64, rounding: bool = True, flaw: Optional[str] = None, slack: bool = True):
        assert flaw is None or flaw in FLAWS
        self.dtype, self.rounding, self.flaw = dtype, rounding, flaw
        self.exact = dtype == torch.float64 and slack

    def R(self, t: torch.Tensor) -> torch.Tensor:
        return bf16r(t) if self.rounding else t

    def w(self, t: torch.Tensor) -> torch.Tensor:
        """A weight operand: rounded once to bf16."""
        return self.R(t.to(self.dtype))

    def dot(self, x, W, b=None, xs=None):
        """pre = W x + b over the last axis of x (W: (out, in)) -> (pre, s, sum|terms|)."""
        if not self.exact:
            pre = torch.matmul(x, W.transpose(-1, -2))
            pre = pre if b is None else pre + b
            return pre, torch.zeros_like(pre), pre.abs()
        terms = x[..., None, :] * W
        pre, mag, n = terms.sum(-1), terms.abs().sum(-1), W.shape[-1]
        if b is not None:
            pre, mag, n = pre + b, mag + b.abs(), n + 1
        s = MARGIN * (n + 1) * U24 * mag
        if xs is not None:
            s = s + (xs[..., None, :] * W.abs()).sum(-1)
        return pre, s, mag

    def _round(self, pre, s, f, trunc: bool):
        clean = self.R(f(pre))
        val = bf16_trunc(f(pre)) if trunc and self.rounding else clean
        if not (self.exact and self.rounding):
            return val, torch.zeros_like(val)
        lo, hi = self.R(f(pre - s)), self.R(f(pre + s))
        return val, torch.maximum(hi - clean, clean - lo)

    def note_relu(self, pre, weight):
        """(scene form: the ReLU inputs A'_n + A'_j of the weighted pairs — `Exact` records them)"""

    def hidden(self, pre, s):
        """bf16(relu(pre)) as the next layer's operand -> (value, its uncertainty: 0 unless flippable)."""
        return self._round(pre, s, torch.relu, self.flaw == "hid_trunc")

    def store(self, pre, s):
        """bf16(pre) as stored or re-fed -> (value, its uncertainty)."""
        return self._round(pre, s, lambda t: t, self.flaw == "out_trunc")


def _tile_bias(A: Arith, b: torch.Tensor) -> torch.Tensor:
    if A.flaw == "tile_bias" and b.shape[-1] > 32:
        return torch.cat((b[..., :32], b[..., :b.shape[-1] - 32]), dim=-1)
    return b


def out_layer(A: Arith, h, hu, W, b):
    """The layer whose result is rounded to bf16: -> (pre, s, stored value, its uncertainty)."""
    b = _tile_bias(A, b)
    pre, s, _ = A.dot(h, W, b, hu)
    val, unc = A.store(pre, s)
    if A.flaw == "bias_late" and A.rounding:
        val = A.R(A.R(A.dot(h, W, None, hu)[0]) + b)
    return pre, s, val, unc


def two_layer(A: Arith, x, xs, W0, b0, W1, b1):
    """W1 bf16(relu(W0 x + b0)) + b1 -> `out_layer`'s tuple."""
    p0, s0, _ = A.dot(x, A.w(W0), b0.to(A.dtype), xs)
    h, hu = A.hidden(p0, s0)
    if A.flaw == "last_hidden":
        h = h.clone()
        h[..., -1] = 0
    return out_layer(A, h, hu, A.w(W1), b1.to(A.dtype))


def _mlp(state, prefix: str, dtype):
    return tuple(state[f"{prefix}.layers.{i}.{n}"].to(dtype) for i in (0, 1) for n in ("weight", "bias"))


# ---------------------------------------------------------------------------------------------------------------------
# the stages
# ---------------------------------------------------------------------------------------------------------------------
def node_emul(state, x: torch.Tensor, A: Arith, xp_stored: Optional[torch.Tensor] = None) -> Dict[str, Out]:
    """Node stage: x' = MLP_{64->256->64}(x) stored in bf16, pq = [W[:, :64] x' + b | W[:, 64:] x'] of attention layer 0.
    pq is one layer behind a value the twin STORES: it is held on that stored x' (xp_stored: the twin's own output; None:
    the emulation's), which enters without uncertainty — through the worst-case propagation of x's flippable elements
    (6 of 10 are, under the a-priori bound) the allowance of pq would exceed the old gate.  "pq_apriori" is that wider
    reference, which takes nothing from the kernels: the twin's pq is held against it as well."""
    W0, b0, W1, b1 = _mlp(state, "node2edge_start_mlp.0", A.dtype)
    Wa, ba = state["attention_mlp.0.layers.0.weight"].to(A.dtype), state["attention_mlp.0.layers.0.bias"].to(A.dtype)
    pre, s, xp, xu = two_layer(A, x.to(A.dtype), None, W0, b0, W1, b1)
    Wpq, bpq = torch.cat((Wa[:, :64], Wa[:, 64:]), dim=0), torch.cat((ba, torch.zeros_like(ba)))
    fed = xp if xp_stored is None else xp_stored.detach().cpu().to(A.dtype).reshape(xp.shape)
    ppre, ps, pq, _ = out_layer(A, fed, None, A.w(Wpq), bpq)
    apre, as_, aval, _ = out_layer(A, xp, xu if A.exact else None, A.w(Wpq), bpq)
    return dict(xp=Out(pre, s, xp, "bf16"), pq=Out(ppre, ps, pq, "bf16"), pq_apriori=Out(apre, as_, aval, "bf16"))


def gumbel(U: torch.Tensor, A: Arith) -> Tuple[torch.Tensor, torch.Tensor]:
    """g = -log(eps - log(U + eps)) -> (g, its slack under the twins' fp32 evaluation).
    With a = fl(U + eps) (relative 2^-24, so 2^-24 absolute in log a), hardware logarithms of a few ulp (4 x 2^-23 relative
    each) and L = eps - log a: |dL| <= 2^-24 + 5 x 2^-23 L, |dg| <= |dL| / L + 4 x 2^-23 |g|; doubled."""
    L = EPS - torch.log(U + EPS)
    g = -torch.log(L)
    return g, (2 * (U24 / L + 5 * U23 + 4 * U23 * g.abs()) if A.exact else torch.zeros_like(g))


def softmax_slack(y, d, delta):
    """Slack of d = softmax(y) where y = (logit + g) / tau and |d(logit + g)| <= delta per element.
    dd_k = d_k (dy_k - sum_j d_j dy_j) = d_k sum_{j != k} d_j (dy_k - dy_j), so |dd_k| <= d_k (1 - d_k) 2 max|dy| =
    d_k (1 - d_k) 2 max(delta) / tau to first order (never more than p_k 2 max|s| / tau; exactly 0 for one type); a factor 2
    for the second-order terms (max(delta) / tau <= FIRST_ORDER_MAX is a condition on the inputs).  The fp32 evaluation: y - max(y)
    carries three roundings of |y| (3 x 2^-24 |y|_max, into the exponent), exp2-based exp of argument x is relative
    (4 + |x|) 2^-23, the sum inherits the weighted mean of that, the reciprocal and product 4 x 2^-23."""
    x = y - y.max(-1, keepdim=True).values
    dmax = delta.max(-1, keepdim=True).values
    rel = (4 + x.abs()) * U23 + 3 * U24 * y.abs().max(-1, keepdim=True).values
    return d * ((1 - d) * 4 * dmax / TAU + rel + (d * rel).sum(-1, keepdim=True) + 4 * U23)


def edge_emul(state, edges: torch.Tensor, U: torch.Tensor, sym_N: int, A: Arith) -> Dict[str, Out]:
    """Edge head (keys behind "head."): z = init_MLP(edges) re-fed in bf16; logits and factor stay fp32; -> "fd" (fp32:
    fac * dist; sym_N: fac (dist_ij + dist_ji) per unordered pair row, 2 fac dist on a self-loop), "dist" (bf16, ordered),
    and "margin" / "delta" for condition (c)."""
    x, u = edges.to(A.dtype), U.to(A.dtype)
    _, _, z, zu = two_layer(A, x, None, *_mlp(state, "head.init_MLP", A.dtype))
    heads = []
    for name in ("MLP_distribution", "MLP_factor"):
        W0, b0, W1, b1 = _mlp(state, f"head.{name}", A.dtype)
        p0, s0, _ = A.dot(z, A.w(W0), b0, zu)
        h, hu = A.hidden(p0, s0)
        heads.append(A.dot(h, A.w(W1), b1, hu)[:2])
    (lg, lgs), (fp, fs) = heads
    if sym_N:
        ii, jj, row = pair_index(sym_N)
        lg, lgs = lg[:, row], lgs[:, row]
    g, gs = gumbel(u, A)
    y = (lg + g) / TAU
    d = torch.softmax(y, dim=-1)
    delta = lgs + gs + 4 * U24 * (lg.abs() + g.abs())
    ds = softmax_slack(y, d, delta) if A.exact else torch.zeros_like(d)
    sig = torch.sigmoid(fp)
    sigs = 2 * sig * (1 - sig) * fs + 8 * U24 * sig if A.exact else torch.zeros_like(sig)
    dist, _ = A.store(d, ds)
    if sym_N:
        N = sym_N
        o1, o2 = ii * N + jj, jj * N + ii
        diag = (ii == jj).to(A.dtype)[None, :, None]
        d2, d2s = d[:, o2] * (1 - diag) + d[:, o1] * diag, ds[:, o2] * (1 - diag) + ds[:, o1] * diag
        fd = sig * d[:, o1] + sig * d2
        fds = sig * (ds[:, o1] + d2s) + sigs * (d[:, o1] + d2) + sigs * (ds[:, o1] + d2s) + 6 * U24 * fd
    else:
        fd = sig * d
        fds = sig * ds + sigs * d + sigs * ds + 4 * U24 * fd
    top = torch.topk(y, min(2, y.shape[-1]), dim=-1).values
    margin = (top[..., 0] - top[..., -1]) * TAU if y.shape[-1] > 1 else torch.full(y.shape[:-1], float("inf"), dtype=A.dtype)
    return dict(fd=Out(fd, fds if A.exact else torch.zeros_like(fd), f32r(fd) if A.rounding else fd, "fp32"), dist=Out(d, ds, dist, "bf16"),
                margin=margin, delta=delta.max(-1).values)


def _typed(state, K: int, dtype):
    W1 = torch.stack([state[f"agg.agg_mlp.{k}.layers.0.weight"] for k in range(K)]).to(dtype)
    b1 = torch.stack([state[f"agg.agg_mlp.{k}.layers.0.bias"] for k in range(K)]).to(dtype)
    W2 = torch.stack([state[f"agg.agg_mlp.{k}.layers.1.weight"] for k in range(K)]).to(dtype)
    b2 = torch.stack([state[f"agg.agg_mlp.{k}.layers.1.bias"] for k in range(K)]).to(dtype)
    return W1, b1, W2, b2


def agg_emul(state, case, inp: Dict[str, torch.Tensor], K: int, rb2: bool, A: Arith) -> Dict[str, Out]:
    """Typed aggregation (keys behind "agg."; case: edge_type_cases.AggCase with forms "eo", "gather", "twin-pair",
    "scene") -> "feat".  rb2: the placement of the two-row-blocks kernel (module docstring); the scene form has one."""
    form, B, N, _ = case
    W1, b1, W2, b2 = _typed(state, K, A.dtype)
    W1, W2 = A.w(W1), A.w(W2)
    ef = inp["ef"].to(A.dtype)
    if A.flaw == "b2_drop":
        b2 = b2.clone()
        b2[K // 2] = 0
    if A.flaw == "ef_neighbour":
        ef = ef.clone()
        ef[:, :, K // 2] = inp["ef"].to(A.dtype).roll(-1, dims=1)[:, :, K // 2]
    b2 = _tile_bias(A, b2)
    if form == "scene":
        return dict(feat=_scene_emul(A, inp["ori"].to(A.dtype), ef, W1, b1, W2, b2, K))
    xs = None
    if form == "eo":
        x = inp["eo"].to(A.dtype)
    else:
        ori = inp["ori"].to(A.dtype)
        if form == "gather":
            H = inp["H"].to(A.dtype)
            xpre, mag, n = torch.matmul(H, ori), torch.matmul(H.abs(), ori.abs()), int(H.abs().sum(-1).max())
            q = _quantum(ori.double(), H.double())
        else:
            ii, jj, _ = pair_index(N)
            xpre, mag, n = ori[:, ii] + ori[:, jj], ori[:, ii].abs() + ori[:, jj].abs(), 2
            inf = torch.full_like(ori.double(), float("inf"))
            u = torch.where(ori == 0, inf, ulp_bf16(ori))
            q = torch.minimum(u[:, ii], u[:, jj]).clamp(max=1.0)
        x, xs = A.store(xpre, sum_slack(mag.double(), q, n).to(A.dtype))
        xs = xs if A.exact else None
    acc, accb, s, mag = 0, 0, 0, 0
    for k in range(K):
        e = ef[..., k:k + 1]
        p0, s0, _ = A.dot(x, W1[k], b1[k], xs)
        if rb2:
            p0, s0 = e * p0, e * s0 + U24 * (e * p0).abs()
        h, hu = A.hidden(p0, s0)
        if A.flaw == "last_hidden":
            h = h.clone()
            h[..., -1] = 0
        t, ts, tm = A.dot(h, W2[k], None, hu)
        if rb2:
            acc, s, mag = acc + t, s + ts, mag + tm + e * b2[k].abs()
        else:
            acc, s, mag = acc + e * t, s + e * ts, mag + e * (tm + b2[k].abs())
        accb = accb + e * b2[k]
    return dict(feat=_typed_out(A, acc, accb, s, mag, K))


def _typed_out(A: Arith, acc, accb, s, mag, K: int) -> Out:
    """feat = acc + accb (the b2 terms), K partial results meeting in fp32 (FMAs, or the waves' partial sums)."""
    pre = acc + accb
    s = s + MARGIN * (K + 2) * U24 * mag if A.exact else torch.zeros_like(pre)
    val, _ = A.store(pre, s)
    if A.flaw == "bias_late" and A.rounding:
        val = A.R(A.R(acc) + accb)
    return Out(pre, s, val, "bf16")


def _scene_emul(A: Arith, ori, ef, W1, b1, W2, b2, K: int) -> Out:
    B, N, _ = ori.shape
    P = pair_index(N)[2].reshape(N, N)
    acc, accb, s, mag = 0, 0, 0, 0
    for k in range(K):
        Ap, As, _ = A.dot(ori, W1[k], b1[k] / 2)                      # (B, N, 128), fp32 in an LDS stage
        own = Ap
        if A.flaw == "scene_row" and B > 1:
            own = Ap.clone()
            own[0, N - 1] = Ap[1, N - 1]
        e = ef[:, P, k]                                               # (B, N, N): the pair weight of (n, j)
        pre = own[:, :, None, :] + Ap[:, None, :, :]
        A.note_relu(pre, e)
        T = e[..., None] * torch.relu(pre)
        S = T.sum(2)
        Ss = ((e[..., None] * (As[:, :, None, :] + As[:, None, :, :] + U24 * pre.abs())).sum(2) + MARGIN * (N + 1) * U24 * S
              if A.exact else torch.zeros_like(S))
        h, hu = A.hidden(S, Ss)
        if A.flaw == "last_hidden":
            h = h.clone()
            h[..., -1] = 0
        c = e.sum(2)[..., None]
        t, ts, tm = A.dot(h, W2[k], None, hu)
        acc, accb = acc + t, accb + c * b2[k]
        s, mag = s + ts + MARGIN * (N + 1) * U24 * c * b2[k].abs(), mag + tm + c * b2[k].abs()
    return _typed_out(A, acc, accb, s, mag, K)


def closing_emul(state, form, src, A: Arith) -> Dict[str, Out]:
    """Closing MLP on plain rows or on the fused-scatter input cat(H^T feat, ori) / N (bottleneck_cases.closing_input)."""
    x = closing_input(form, src, A.dtype)
    xs = None
    if form[0] != "x":
        # N x = cat(H^T feat, ori): a sum of bf16 values (`sum_slack`), then ONE division (or a reciprocal and a product:
        # 3 x 2^-24 relative)
        N = form[2]
        mag = closing_input(form, {k: v.abs() for k, v in src.items()}, torch.float64) * N
        H = (src["H"] if "H" in src else pair_rows_incidence(N)[None].expand(form[1], -1, -1)).double()
        q = torch.cat((_quantum(src["feat"].double(), H.transpose(1, 2)), ulp_bf16(src["ori"]).clamp(min=2.0 ** -140)), dim=-1)
        n = int(H.sum(1).max())
        slack = (sum_slack(mag, q.reshape(mag.shape), n) / N + 3 * U24 * mag / N).to(A.dtype)
        x, xs = A.store(x, slack)
        xs = xs if A.exact else None
    pre, s, val, _ = two_layer(A, x, xs, *_mlp({"m." + k: v for k, v in state.items()}, "m", A.dtype))
    return dict(y=Out(pre, s, val, "bf16"))


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def bounds(o: Out) -> Tuple[torch.Tensor, torch.Tensor]:
    r = bf16r if o.fmt == "bf16" else f32r
    return r(o.pre - o.s), r(o.pre + o.s)


def rule_failures(got: torch.Tensor, o: Out) -> int:
    """Elements of `got` that are not the rounding of any value within the slack."""
    g = got.detach().double().cpu().reshape(o.pre.shape)
    lo, hi = bounds(o)
    return int(((g < lo) | (g > hi) | ~torch.isfinite(g)).sum())


def rule_report(got: torch.Tensor, o: Out) -> Dict[str, float]:
    """The records of DESIGN section 2 (not gates): share of elements not bit-identical to the emulation, worst
    |got - pre| / (s + ulp)."""
    g = got.detach().double().cpu().reshape(o.pre.shape)
    ulp = ulp_bf16(o.pre) if o.fmt == "bf16" else o.pre.abs() * U23
    return dict(differ=float((g != o.val).double().mean()), worst=float(((g - o.pre).abs() / (o.s + ulp).clamp_min(1e-300)).max()),
                fail=rule_failures(got, o), n=g.numel())


def old_gate_passes(val: torch.Tensor, ref64: torch.Tensor) -> bool:
    return float((val - ref64).abs().max()) <= OLD_GATE * float(ref64.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# the cases of part A: (stage, ...) tuples; `emulate(case, A)` evaluates one
# ---------------------------------------------------------------------------------------------------------------------
# 69 rows everywhere a stage takes plain rows: two full 32-row blocks and a ragged one, an ODD number of row blocks (one
# two-row-block wave holds a single block), fewer than 128 row blocks.
NODE_CASES = (("node", 3, 23), ("node", 5, 33))                       # 69 rows; 165 rows: two workgroups, a ragged block
# (K, B, E, sym_N, kind).  With the module as initialised the outputs lie FOUR bf16-fed layers behind the input and z is not
# stored: the worst-case propagation of the slack through z (4 of 10 elements flippable under the a-priori bound) and the
# heads' hidden layers would widen the allowance to three times the old gate.  So the chain is held in two halves, each one
# layer pair behind determined values, each with every rounding of its half as initialised:
#   kind "heads": init_MLP replaced by an exact pass-through (z = relu(x) - relu(-x) = x: nothing rounds) — the two heads,
#     the Gumbel softmax and the sigmoid;
#   kind "init<j>": init_MLP as initialised, one type (dist == 1) and a factor head that passes column j of z through
#     exactly (f = relu(z_j) - relu(-z_j)), so that the fp32 output factor * dist = sigmoid(z_j) shows the re-fed bf16 z_j
#     through the sigmoid's linear range: the init pair's hidden rounding, its bias and the rounding of z, in both output
#     tiles (j = 0, 31 | 32, 63) and in the pair form (j = 40); 207 rows: six full row blocks and a ragged one.
EDGE_CASES = (tuple(("edge",) + c + ("heads",) for c in ((6, 3, 23, 0), (10, 3, 23, 0), (6, 3, 15, 5), (1, 3, 23, 0)))
              + tuple(("edge", 1, 9, 23, 0, f"init{j}") for j in (0, 31, 32, 63)) + (("edge", 1, 3, 15, 5, "init40"),))
AGG_FORMS = (("eo", 3, 0, 23), ("gather", 3, 11, 3), ("gather", 3, 20, 5), ("twin-pair", 3, 5, 0), ("twin-pair", 3, 11, 0),
             ("scene", 12, 1, 0), ("scene", 3, 33, 0), ("scene", 2, 50, 0), ("scene", 2, 64, 0))
AGG_CASES = tuple(("agg", K, rb2) + f for f in AGG_FORMS for K in ((1, 6, 10, 16) if f[0] == "eo" else (6, 10))
                  for rb2 in ((False,) if f[0] == "scene" else (False, True)))
# Scene form: every node keeps 8 of its 64 features (at random per node: every column is used).  The a-priori slack of
# A' = W1k ori + b1k / 2 grows with sum|terms|, the type sums S it feeds do not: on dense inputs a percent of the 128 K
# rounded type sums behind a result are flippable and nearly every element has two admissible values, so that a double
# rounding (the late bias) moves an element only to its other admissible value.
SCENE_KEEP = 8
CLOSING_SCATTER = ("hyper", 3, 11, 3)
# (the fused scatter at 40: two output tiles, the second ragged; its inputs are cat(H^T feat, ori) / 11, small against the
# biases, and at 64 this seed's last hidden unit moves no output by a bf16 step)
CLOSING_CASES = tuple(("closing", d, f) for f, ds in ((X_FORM, (64, 33, 32)), (CLOSING_SCATTER, (40,))) for d in ds)
CASES = NODE_CASES + EDGE_CASES + AGG_CASES + CLOSING_CASES
PRECISION_FLAWS = FLAWS[:3]
STAGE_FLAWS = dict(node=FLAWS[:4] + ("last_hidden",), edge=FLAWS[:4] + ("last_hidden",), closing=FLAWS[:4] + ("last_hidden",),
                   agg=FLAWS[:7], scene=FLAWS)


def case_id(case) -> str:
    st = case[0]
    if st == "node":
        return f"node-B{case[1]}-N{case[2]}"
    if st == "edge":
        return f"edge-{case[5]}-K{case[1]}-{case[2]}x{case[3]}" + (f"-sym{case[4]}" if case[4] else "")
    if st == "agg":
        _, K, rb2, form, B, N, x = case
        return f"agg-{form}-K{K}-B{B}-" + (f"E{x}" if form == "eo" else f"N{N}" + (f"-s{x}" if x else "")) + ("-rb2" if rb2 else "")
    return f"closing-d{case[1]}-{form_id(case[2])}"


def stage_of(case) -> str:
    return "scene" if case[0] == "agg" and case[3] == "scene" else case[0]


@functools.lru_cache(maxsize=None)
def case_flaws(case) -> Tuple[str, ...]:
    """The named flaws a case exercises.  A routing flaw: iff it changes the float64 function on the case's inputs (a
    closing MLP up to 32 outputs has no second tile, a scene of one node no neighbouring edge, a hidden unit that is off on
    every row reaches nothing).  A precision flaw: wherever the value it names is rounded — the pass-through init_MLP has
    no bias to add late, a one-type distribution is exactly 1 however it is rounded."""
    c = case_inputs(case)
    r64 = ref64(case)
    keep = []
    for f in STAGE_FLAWS[stage_of(case)]:
        if f in ROUTING_FLAWS:
            moved = _emulate(case, c, Arith(rounding=False, slack=False, flaw=f))
            if all(torch.equal(moved[k].pre, r64[k]) for k in r64):
                continue
        elif case[0] == "edge" and case[5] == "heads" and (f == "bias_late" or (f == "out_trunc" and case[1] == 1)):
            continue
        keep.append(f)
    return tuple(keep)


def _gen(*key: int) -> torch.Generator:
    seed = 0
    for k in key:
        seed = (seed * 1009 + int(k)) % ((1 << 61) - 1)
    return torch.Generator().manual_seed(seed)


def _rnd16(g, *shape) -> torch.Tensor:
    return torch.randn(*shape, generator=g).bfloat16().float()


def pass_through_(mlp) -> None:
    """In place: a 64 -> 128 -> 64 MLP that returns its input exactly, y = relu(x) - relu(-x)."""
    eye = torch.eye(64)
    with torch.no_grad():
        mlp.layers[0].weight.copy_(torch.cat((eye, -eye), dim=0))
        mlp.layers[1].weight.copy_(torch.cat((eye, -eye), dim=1))
        mlp.layers[0].bias.zero_()
        mlp.layers[1].bias.zero_()


def column_factor_(mlp, j: int) -> None:
    """In place: a 64 -> 128 -> 1 MLP that returns column j of its input exactly, f = relu(z_j) - relu(-z_j)."""
    with torch.no_grad():
        for layer in mlp.layers:
            layer.weight.zero_()
            layer.bias.zero_()
        mlp.layers[0].weight[0, j], mlp.layers[0].weight[1, j] = 1, -1
        mlp.layers[1].weight[0, 0], mlp.layers[1].weight[0, 1] = 1, -1


def _draw(case, draw: int) -> Dict:
    st = case[0]
    if st == "node":
        _, B, N = case
        mod = pair_module(6, 4100 + N)
        return dict(mod=mod, state=state_of(mod), x=_rnd16(_gen(21, B, N, draw), B, N, 64))
    if st == "edge":
        _, K, B, E, sym_N, kind = case
        mod = edge_head(K)
        if kind == "heads":
            pass_through_(mod.init_MLP)
        else:
            column_factor_(mod.MLP_factor, int(kind[4:]))
        g = _gen(22, K, B, E, sym_N, draw)
        edges, U = _rnd16(g, B, E, 64), torch.rand(B, sym_N * sym_N if sym_N else E, K, generator=g)
        return dict(mod=mod, state=state_of(mod, "head"), edges=edges, U=U, sym_N=sym_N, K=K)
    if st == "agg":
        _, K, rb2, form, B, N, x = case
        mod = agg_module(K)
        g = _gen(23, K, B, N, x, AGG_FORMS.index((form, B, N, x)), draw)
        inp = dict(eo=_rnd16(g, B, x, 64)) if form == "eo" else dict(ori=_rnd16(g, B, N, 64))
        if form == "scene":
            keep = torch.rand(B, N, 64, generator=g).argsort(-1) < SCENE_KEEP
            inp["ori"] = inp["ori"] * keep
        E = x if form == "eo" else pair_count(N)
        if form == "gather":
            inp["H"] = O.topk_incidence_ranked(O.affinity(inp["ori"]), x)
            E = inp["H"].shape[1]
        inp["ef"] = torch.rand(B, E, K, generator=g)
        return dict(mod=mod, state=state_of(mod, "agg"), inp=inp, K=K)
    _, d, form = case
    c = closing_case((form,), d, True)          # (its own seeded draws: bottleneck_cases)
    return dict(mod=c["mlps"][0], state=c["states"][0], src=c["srcs"][0], form=form)


def _emulate(case, c: Dict, A: Arith) -> Dict:
    with torch.no_grad():
        if case[0] == "node":
            return node_emul(c["state"], c["x"], A)
        if case[0] == "edge":
            return edge_emul(c["state"], c["edges"], c["U"], c["sym_N"], A)
        if case[0] == "agg":
            return agg_emul(c["state"], case[3:], c["inp"], c["K"], case[2], A)
        return closing_emul(c["state"], c["form"], c["src"], A)


def conditions(case, ref: Dict, r64: Dict) -> Dict[str, float]:
    """The conditions on the inputs, on the reference alone: "b": the largest allowance s + ulp_bf16(pre) (fp32 output: s)
    as a share of the old gate OLD_GATE max|ref64| (asked: <= 1); edge head, "c": the smallest winner margin less twice the
    logits' slack over the ordered edges (asked: > 0) and "first": the largest slack / tau (asked: <= FIRST_ORDER_MAX)."""
    out = dict(b=max(float(allowance_share(ref[k], r64[k].pre).max()) for k in OUTPUTS[case[0]]))
    if case[0] == "edge":
        out.update(c=float((ref["margin"] - 2 * ref["delta"]).min()), first=float(ref["delta"].max()) / TAU)
    return out


def conditions_hold(case, cond: Dict[str, float]) -> bool:
    return cond["b"] <= 1.0 and cond.get("c", 1.0) > 0 and cond.get("first", 0.0) <= FIRST_ORDER_MAX


OUTPUTS = dict(node=("xp", "pq"), edge=("fd", "dist"), agg=("feat",), closing=("y",))


@functools.lru_cache(maxsize=None)
def case_inputs(case) -> Dict:
    """-> {"mod" (on the CPU), "state", the inputs, "ref" (the float64 emulation with its slack), "ref64" (the same function
    without roundings), "cond" (`conditions`), "draw"}: the first of DRAWS seeded draws of the inputs on which the conditions
    hold — the suite's usual pattern; nothing of the code under test enters the choice.  The closing MLP's inputs are
    bottleneck_cases.closing_case's."""
    last = None
    for draw in range(DRAWS if case[0] != "closing" else 1):
        c = _draw(case, draw)
        c["ref"], c["ref64"] = _emulate(case, c, Arith()), _emulate(case, c, Arith(rounding=False, slack=False))
        c["cond"], c["draw"] = conditions(case, c["ref"], c["ref64"]), draw
        last = c
        if conditions_hold(case, c["cond"]):
            return c
    raise AssertionError(f"{case_id(case)}: no draw meets the conditions on the reference: {last['cond']}")


def allowance_share(o: Out, ref64: torch.Tensor) -> torch.Tensor:
    """(s + ulp_bf16(pre)) / (OLD_GATE max|ref64|) per element (an fp32 output: s alone)."""
    return (o.s + (ulp_bf16(o.pre) if o.fmt == "bf16" else 0)) / (OLD_GATE * float(ref64.abs().max()))


def emulate(case, A: Arith) -> Dict[str, Out]:
    """The outputs of a case under the arithmetic A, name -> Out."""
    e = _emulate(case, case_inputs(case), A)
    return {k: e[k] for k in OUTPUTS[case[0]]}


def reference(case) -> Dict[str, Out]:
    """The float64 emulation with its slack: what the rule is held against."""
    return {k: case_inputs(case)["ref"][k] for k in OUTPUTS[case[0]]}


def ref64(case) -> Dict[str, torch.Tensor]:
    """The same functions without any rounding, float64 (the oracle's)."""
    return {k: case_inputs(case)["ref64"][k].pre for k in OUTPUTS[case[0]]}


# ---------------------------------------------------------------------------------------------------------------------
# B. exact-arithmetic probes
# ---------------------------------------------------------------------------------------------------------------------
# Weights: every row a few nonzeros +-2^e whose columns cover every input; biases and inputs small integers; so every
# product and every partial sum is a small multiple of a power of two — an fp32 (and, where stored, a bf16) number — and
# the float64 result is the result of EVERY correct evaluation: bf16 storage, f16x3, bf16x6 and the fp32 cores, any order.
PROBE_QUANTUM = 2.0 ** -4         # every term of every sum is a multiple of this ...
PROBE_BITS = 24                   # ... and every sum of |terms| stays below 2^24 of them
SELECT = 2.0 ** 15                # the edge head's selector weight: logits of two types differ by at least SELECT less the rest


def probe_linear(g, out: int, din: int, mags=(1.0, 2.0), nnz: int = 3, bias: int = 2):
    """W (out, din): row r holds `nnz` (at least din / out: every column is covered) nonzeros +-m, m from `mags`, at the
    columns perm[(r nnz + i + wraps) mod din] (shifted by one with every wrap, so that no two rows hold the same columns);
    b: integers in [-bias, bias]."""
    nnz = max(nnz, -(-din // out))
    perm = torch.randperm(din, generator=g)
    W = torch.zeros(out, din, dtype=torch.float64)
    m = torch.tensor(mags, dtype=torch.float64)
    for r in range(out):
        cols = perm[(r * nnz + torch.arange(nnz) + (r * nnz) // din) % din]
        sign = torch.randint(0, 2, (nnz,), generator=g).double() * 2 - 1
        W[r, cols] = sign * m[torch.randint(0, len(mags), (nnz,), generator=g)]
    return W, torch.randint(-bias, bias + 1, (out,), generator=g).double()


def _ints(g, lo: int, hi: int, *shape) -> torch.Tensor:
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _load(mlp, W0, b0, W1, b1) -> None:
    with torch.no_grad():
        for layer, W, b in ((mlp.layers[0], W0, b0), (mlp.layers[1], W1, b1)):
            layer.weight.copy_(W)
            layer.bias.copy_(b)


def _type_weights(g, B: int, E: int, K: int) -> torch.Tensor:
    """(B, E, K): one-hot, or 1/2 on two types."""
    ef = torch.zeros(B, E, K)
    a = torch.randint(0, K, (B, E), generator=g)
    b = torch.randint(0, K, (B, E), generator=g)
    ef.scatter_add_(2, a[..., None], torch.full((B, E, 1), 0.5))
    ef.scatter_add_(2, b[..., None], torch.full((B, E, 1), 0.5))
    return ef


PROBE_NODE = (("node", 3, 23),)
PROBE_EDGE = (("edge", 6, 3, 23, 0), ("edge", 10, 3, 23, 0), ("edge", 6, 3, 15, 5), ("edge", 1, 3, 23, 0))
# typed aggregation: the twins' forms, and fp32 storage's ("pair" / "pair-node": PairSpec(A), the first layer per node)
PROBE_AGG_FORMS = (("eo", 3, 0, 23), ("gather", 3, 11, 3), ("gather", 3, 20, 5), ("twin-pair", 3, 5, 0), ("twin-pair", 3, 11, 0),
                   ("scene", 32, 1, 0), ("scene", 3, 33, 0), ("scene", 2, 50, 0), ("scene", 2, 64, 0),
                   ("pair", 3, 5, 0), ("pair", 3, 11, 0), ("pair-node", 3, 11, 0))
PROBE_AGG = tuple(("agg", K) + f for f in PROBE_AGG_FORMS for K in ((1, 6, 10, 16) if f[0] == "eo" else (6, 10)))
PROBE_SCATTER = ("hyper", 6, 8, 3)                      # N = 8: the division by N is exact
PROBE_CLOSING = tuple(("closing", d, f) for f, ds in ((X_FORM, (64, 33, 32)), (PROBE_SCATTER, (40,))) for d in ds)
PROBES = PROBE_NODE + PROBE_EDGE + PROBE_AGG + PROBE_CLOSING
TWIN_FORMS = ("eo", "gather", "twin-pair", "scene")
FP32_FORMS = ("eo", "gather", "pair", "pair-node")


def probe_id(case) -> str:
    if case[0] == "agg":
        _, K, form, B, N, x = case
        return f"probe-agg-{form}-K{K}-B{B}-" + (f"E{x}" if form == "eo" else f"N{N}" + (f"-s{x}" if x else ""))
    if case[0] == "edge":
        return f"probe-edge-K{case[1]}-{case[2]}x{case[3]}" + (f"-sym{case[4]}" if case[4] else "")
    return "probe-" + (f"node-B{case[1]}-N{case[2]}" if case[0] == "node" else f"closing-d{case[1]}-{form_id(case[2])}")


class Exact(Arith):
    """Float64 without roundings that RECORDS what the probe conditions speak about: every value a twin stores in bf16
    ("stored"), per sum the sum of |terms| and the terms' granularity ("sums"), and every hidden layer ("hidden")."""

    def __init__(self, flaw: Optional[str] = None):
        super().__init__(torch.float64, rounding=False, flaw=flaw, slack=False)
        self.stored, self.sums, self.hiddens, self.relus = [], [], [], []

    def note_relu(self, pre, weight):
        self.relus.append(pre[weight != 0])

    def w(self, t):
        self.stored.append(t.double())
        return t.double()

    def dot(self, x, W, b=None, xs=None):
        terms = x[..., None, :] * W
        mag = terms.abs().sum(-1) + (0 if b is None else b.abs())
        pre = terms.sum(-1) + (0 if b is None else b)
        gran = bool((terms / PROBE_QUANTUM == torch.round(terms / PROBE_QUANTUM)).all())
        self.sums.append((float(mag.max()), gran and (b is None or bool((b / PROBE_QUANTUM == torch.round(b / PROBE_QUANTUM)).all()))))
        return pre, torch.zeros_like(pre), mag

    def hidden(self, pre, s):
        v = torch.relu(pre)
        self.stored.append(v)
        self.hiddens.append(pre)
        return v, torch.zeros_like(v)

    def store(self, pre, s):
        self.stored.append(pre)
        return pre, torch.zeros_like(pre)


@functools.lru_cache(maxsize=None)
def probe_inputs(case) -> Dict:
    """The module (probe weights loaded into the product's own module, so that the product packs them) and inputs of a probe."""
    st = case[0]
    g = _gen(31, zlib.crc32(repr(case).encode()))          # (a seed of the case that does not depend on the process)
    if st == "closing":
        _, d, form = case
        mlp = closing_mlp(d)
        scat = form[0] != "x"
        _load(mlp, *probe_linear(g, 128, 128), *probe_linear(g, d, 128, mags=(1.0,) if scat else (1.0, 0.5)))
        if not scat:
            src = dict(x=_ints(g, -2, 2, ROWS, 128))
        else:
            _, B, N, s = form
            ori = 8 * _ints(g, -1, 1, B, N, 64)
            src = dict(ori=ori, feat=8 * _ints(g, -1, 1, B, N, 64), H=O.topk_incidence_ranked(O.affinity(_rnd16(g, B, N, 64)), s))
        return dict(mod=mlp, state=state_of(mlp), src=src, form=form)
    if st == "node":
        _, B, N = case
        mod = pair_module(6, 4200)
        _load(mod.node2edge_start_mlp[0], *probe_linear(g, 256, 64), *probe_linear(g, 64, 256, mags=(1.0,)))
        Wp, bp = probe_linear(g, 32, 64, mags=(1.0, 0.5), nnz=2)
        Wq, _ = probe_linear(g, 32, 64, mags=(1.0, 0.5), nnz=2)
        with torch.no_grad():
            mod.attention_mlp[0].layers[0].weight.copy_(torch.cat((Wp, Wq), dim=1))
            mod.attention_mlp[0].layers[0].bias.copy_(bp)
        return dict(mod=mod, state=state_of(mod), x=_ints(g, -2, 2, B, N, 64))
    if st == "agg":
        _, K, form, B, N, x = case
        mod = agg_module(K)
        scene = form in ("scene", "pair-node")
        for k in range(K):
            W1, b1 = probe_linear(g, 128, 64, mags=(1.0,) if scene else (1.0, 2.0))
            if form != "eo":
                b1 = 2 * torch.round(b1 / 2)            # (the per-node first layer adds b1 / 2 twice)
            _load(mod.agg_mlp[k], W1, b1, *probe_linear(g, 64, 128, mags=(1.0,) if scene else (1.0, 0.5)))
        if form == "eo":
            inp, E = dict(eo=_ints(g, -2, 2, B, x, 64)), x
        else:
            inp, E = dict(ori=_ints(g, -1, 1, B, N, 64)), pair_count(N)
            if form == "gather":
                inp["H"] = O.topk_incidence_ranked(O.affinity(_rnd16(g, B, N, 64)), x)
                E = inp["H"].shape[1]
        ef = _type_weights(g, B, E, K)
        if scene:
            # a node's type sum S adds over its partners: only the pairs (n, n) and (n, n + 1) carry weight, three per node
            ii, jj, _ = pair_index(N)
            ef = ef * ((jj - ii <= 1) | ((ii == 0) & (jj == N - 1))).float()[None, :, None]
        inp["ef"] = ef
        return dict(mod=mod, state=state_of(mod, "agg"), inp=inp, K=K)
    _, K, B, E, sym_N = case
    mod = edge_head(K)
    # init_MLP: z_40 = x_0 (hidden relu(x_0), relu(-x_0)): the factor's selector, in the SECOND output tile, where the first
    # tile's bias (b1[8] = 1) would show; z_1 = relu(x_1 + 2) + relu(x_2 + 2) in 0..8: the type's selector; the other 62
    # outputs and 124 hidden units generic (they move the logits by less than the selector's step: what the outputs show
    # of the head is its selectors' routes)
    W0, b0 = probe_linear(g, 128, 64)
    W1, b1 = probe_linear(g, 64, 128, mags=(1.0,))
    FZ = 40
    sel = [126, 127, 2, 3]            # hidden relu(x_0), relu(-x_0) (the LAST hidden column among them), relu(x_1 + 2), relu(x_2 + 2)
    W0[sel], b0[sel], W1[FZ], W1[1], b1[FZ], b1[1], b1[FZ - 32], W1[:, sel] = 0, 0, 0, 0, 0, 0, 1, 0
    W0[126, 0], W0[127, 0], W0[2, 1], W0[3, 2], b0[2], b0[3] = 1, -1, 1, 1, 2, 2
    W1[FZ, 126], W1[FZ, 127], W1[1, 2], W1[1, 3] = 1, -1, 1, 1
    for c in ((W1 != 0).sum(0) == 0).nonzero().reshape(-1).tolist():      # (a column only the two selector rows had held)
        W1[2 + c % 30, c] = 1
    _load(mod.init_MLP, W0, b0, W1, b1)
    # distribution head: hidden 2k, 2k + 1 = relu(z_1 - k), relu(k - z_1), logit_k = -SELECT |z_1 - k| + the generic rest
    Wd0, bd0 = probe_linear(g, 128, 64, mags=(1.0,))
    Wd1, bd1 = probe_linear(g, K, 128, mags=(1.0,), nnz=3)
    Wd0[:2 * K], Wd1[:, :2 * K] = 0, 0
    for k in range(K):
        Wd0[2 * k, 1], bd0[2 * k], Wd0[2 * k + 1, 1], bd0[2 * k + 1] = 1, -k, -1, k
        Wd1[k, 2 * k], Wd1[k, 2 * k + 1] = -SELECT, -SELECT
    _load(mod.MLP_distribution, Wd0, bd0, Wd1, bd1)
    # factor head: f = 1024 clamp(z_0, -1, 1) (hidden relu(z_0), relu(z_0 - 1), relu(-z_0), relu(-z_0 - 1)): 0 -> 1/2, 1024 -> 1,
    # -1024 -> 0 in float64 and in fp32 alike; the other hidden units in identical pairs of weight +64 / -64, which cancel
    # exactly in any order and still reach the output
    Wf0, bf0 = probe_linear(g, 128, 64, mags=(1.0,))
    Wf0[1::2], bf0[1::2] = Wf0[0::2].clone(), bf0[0::2].clone()
    Wf1 = torch.zeros(1, 128, dtype=torch.float64)
    Wf1[0, 0::2], Wf1[0, 1::2] = 64, -64
    Wf0[:4], bf0[:4] = 0, 0
    Wf0[0, FZ], Wf0[1, FZ], Wf0[2, FZ], Wf0[3, FZ], bf0[1], bf0[3] = 1, 1, -1, -1, -1, -1
    Wf1[0, :4] = torch.tensor([1024.0, -1024.0, -1024.0, 1024.0], dtype=torch.float64)
    _load(mod.MLP_factor, Wf0, bf0, Wf1, torch.zeros(1, dtype=torch.float64))
    edges, U = _ints(g, -2, 2, B, E, 64), torch.rand(B, sym_N * sym_N if sym_N else E, K, generator=g)
    return dict(mod=mod, state=state_of(mod, "head"), edges=edges, U=U, sym_N=sym_N, K=K)


def probe_eval(case, A: Arith, placement: str = "plain") -> Dict[str, torch.Tensor]:
    """The float64 result of a probe, name -> tensor (the typed aggregation's forms of fp32 storage are the same
    functions: "pair" is "twin-pair", "pair-node" is "scene").  placement "rb2": the two-row-blocks order of operations."""
    c = probe_inputs(case)
    with torch.no_grad():
        if case[0] == "node":
            e = node_emul(c["state"], c["x"], A)
        elif case[0] == "edge":
            e = edge_emul(c["state"], c["edges"], c["U"], c["sym_N"], A)
        elif case[0] == "agg":
            form = {"pair": "twin-pair", "pair-node": "scene"}.get(case[2], case[2])
            e = agg_emul(c["state"], (form,) + case[3:], c["inp"], c["K"], placement == "rb2", A)
        else:
            e = closing_emul(c["state"], c["form"], c["src"], A)
    return {k: e[k].pre for k in OUTPUTS[case[0]]}


@functools.lru_cache(maxsize=None)
def probe_reference(case) -> Dict[str, torch.Tensor]:
    return probe_eval(case, Arith(rounding=False, slack=False))
