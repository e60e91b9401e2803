"""Test helper: plain torch statements of every backward kernel of groupnet_amd/csrc/gn_backward.hip, the case tables of
tests/test_backward_kernels_gpu.py, and the one tolerance rule those tests use.

Every reference takes the dtype as a parameter: float64 is the reference, float32 (the same code on the CPU) is the
yardstick `e32` of the gate.  Nothing here imports groupnet_amd; tests/test_backward_kernels_cpu.py pins the references
to the golden-pinned oracle (oracle/ms_hgnn_oracle.py), checks the conditions on the inputs of every GPU case, that the
case tables reach every launcher form restated below, and that a reference with one of the named flaws is told apart.

Inputs of the pooling cases are built so that no ReLU decision depends on rounding: pq on the dyadic grid k/64 in
[-2, 2], H in {0, 1, 2, 0.5}; every pre-activation P_n[c] + sum_m h_m Qn_m[c] is then a multiple of 1/128 below 2^10,
exact in fp32 in any summation order, and either exactly 0 (derivative 0 in torch and in the kernel, `pre > 0`) or at
least 1/128 away from it.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

F64, F32 = torch.float64, torch.float32
FLOOR = 2.0 ** -22          # of `scale`: one rounding of the result (2^-24) with the gate's own factor 4
PROBE_REL = 2.0 ** -23      # split exactness probe: the split's stated 2^-24 plus one rounding
SPLITK_CEILING = 1e-4       # of `scale`, K >= 4096 split-K cases (as tests/test_backward_gpu.py's accumulate case)
FACTOR = 4.0                # margin of a correct fp32 path against float64, in units of the fp32 oracle's own distance


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def pair_count(N: int) -> int:
    return N * (N + 1) // 2


def gate(ref64: torch.Tensor, ref32: torch.Tensor, scale: float):
    """(bound on max|hip - ref64|, e32): max(4 * max|ref32 - ref64|, 2^-22 * scale).  The caller caps it at its ceiling."""
    e32 = float((ref32.double() - ref64).abs().max()) if ref64.numel() else 0.0
    return max(FACTOR * e32, FLOOR * float(scale)), e32


# ------------------------------------------------------------------------------------------------------------------
# attention pooling (gn_node2edge_bwd[_grouped]_f32)
# ------------------------------------------------------------------------------------------------------------------
N2E_FLAWS = ("nonmembers_dropped", "h_once", "selfloop_weight_1", "relu_derivative_1_at_0")


def pair_incidence(N: int, sym: bool, self_w: float = 2.0, dtype=F32) -> torch.Tensor:
    """(E, N) incidence of the implicit pairwise graph: ordered E = N*N (edge i*N + j), or with sym the N(N+1)/2 unordered
    pairs in gn_pair_decode order ((i, j >= i), row-major); weight 1 on i and j, `self_w` (2) on i when i == j."""
    pairs = [(i, j) for i in range(N) for j in range(i if sym else 0, N)]
    H = torch.zeros(len(pairs), N, dtype=dtype)
    for e, (i, j) in enumerate(pairs):
        if i == j:
            H[e, i] = self_w
        else:
            H[e, i] = H[e, j] = 1.0
    return H


def n2e_ref(xp, pq, H, w2, b2, flaw: Optional[str] = None, keep: Optional[dict] = None):
    """Pooled edges (B,E,64) as the oracle's decomposed node2edge computes them from its pieces.  b2: scalar or (B,E,N)."""
    P, Qn = pq[..., :32], pq[..., 32:]
    Q = H @ Qn
    pre = P[:, None, :, :] + Q[:, :, None, :]
    if flaw == "relu_derivative_1_at_0":
        act = torch.where(pre >= 0, pre, torch.zeros_like(pre))
    else:
        act = torch.relu(pre)
    att = act @ w2 + b2
    if keep is not None:
        keep["pre"], keep["act"] = pre.detach(), act.detach()
    member = (H != 0).to(H.dtype)
    if flaw == "nonmembers_dropped":
        z = (att * H).masked_fill(H == 0, float("-inf"))
        z = z - z.max(dim=2, keepdim=True).values.clamp_min(-1e300)
        e = torch.exp(z)
        p = e / e.sum(dim=2, keepdim=True).clamp_min(1e-300)
    else:
        p = torch.softmax(att * H, dim=2)
    return (p * (member if flaw == "h_once" else H)) @ xp


def n2e_grads(inp: Dict[str, torch.Tensor], dtype, flaw: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """Expected contents of the kernel's in-out buffers, start + gradient of <edges, dedges>, evaluated in `dtype`:
    dxp, dpq, dw2, db2, the scales of the two sums (absolute-term sums, the start value counted as one more term) and
    the ReLU pattern."""
    c = lambda k: inp[k].to(dtype)
    xp, pq = c("xp").requires_grad_(True), c("pq").requires_grad_(True)
    H, w2 = c("H"), c("w2")
    B, E, N = H.shape
    b2 = c("b2").reshape(1, 1, 1).expand(B, E, N).clone().requires_grad_(True)
    keep: dict = {}
    edges = n2e_ref(xp, pq, H, w2, b2, flaw, keep)
    dxp, dpq, datt = torch.autograd.grad((edges * c("dedges")).sum(), (xp, pq, b2))
    terms = datt[..., None] * keep["act"]                      # (B,E,N,32)
    return dict(dxp=c("dxp0") + dxp, dpq=c("dpq0") + dpq,
                dw2=c("dw20") + terms.sum(dim=(0, 1, 2)), db2=c("db20") + datt.sum().reshape(1),
                dw2_scale=float((c("dw20").abs() + terms.abs().sum(dim=(0, 1, 2))).max()),
                db2_scale=float(c("db20").abs().sum() + datt.abs().sum()),
                relu=keep["pre"] > 0, pre=keep["pre"])


@dataclass(frozen=True)
class N2ECase:
    name: str
    B: int
    N: int
    E: int
    kind: str            # "hyper" | "ordered" | "sym"
    members: int = 0
    zero_scene: int = -1     # this scene's dedges are 0: its dxp / dpq must come back bit-identical
    w2_scale: float = 0.25   # keeps the attention logits O(1), where the fp32 reference stays inside the ceiling
    seed: int = 0


# f: the table's B = 1 shapes carry one more scene, the one whose dedges are zero
N2E_CASES = [
    N2ECase("a", 3, 11, 11, "hyper", 5, zero_scene=1, seed=1),
    N2ECase("b", 2, 11, 1, "hyper", 11, seed=2),
    N2ECase("c_n1_ordered", 2, 1, 1, "ordered", seed=3),
    N2ECase("c_n1_sym", 2, 1, 1, "sym", seed=4),
    N2ECase("c_n2_ordered", 2, 2, 4, "ordered", seed=5),
    N2ECase("d_ordered", 3, 11, 121, "ordered", seed=6),
    N2ECase("d_sym", 3, 11, 66, "sym", seed=7),
    N2ECase("e_n60", 2, 60, 60, "hyper", 16, zero_scene=1, seed=8),
    N2ECase("e_n61", 2, 61, 61, "hyper", 16, zero_scene=1, seed=9),
    N2ECase("f_n140", 2, 140, 20, "hyper", 100, zero_scene=1, w2_scale=1 / 16, seed=10),
    N2ECase("f_n141", 2, 141, 37, "hyper", 100, zero_scene=1, w2_scale=1 / 16, seed=11),
    N2ECase("g", 2, 141, 5, "hyper", 141, w2_scale=1 / 16, seed=12),
]
# the four groups of the grouped launch at (B, N) = (3, 11); the ordered group's dedges are all zero
N2E_GROUPED = [
    N2ECase("grp_sym", 3, 11, 66, "sym", seed=21),
    N2ECase("grp_ordered", 3, 11, 121, "ordered", zero_scene=-2, seed=22),
    N2ECase("grp_hyper", 3, 11, 11, "hyper", 5, seed=23),
    N2ECase("grp_one", 3, 11, 1, "hyper", 11, seed=24),
]


def n2e_form(N: int, explicit_H: bool) -> str:
    """gn_node2edge_bwd_f32's choice: one workgroup per scene while x', pq, their gradients and the four waves' lists
    fit in LDS (64 KiB, or 150 KiB with the opt-in), else one wave per hyperedge."""
    scene_lds = (4 * N * 64 + 64 + 4 * 4 * N) * 4
    if scene_lds <= 64 * 1024:
        return "scene"
    if scene_lds <= 150 * 1024:
        return "scene_big_lds"
    return "wave" if explicit_H else "error"


def _hyper_H(case: N2ECase, g: torch.Generator) -> torch.Tensor:
    B, N, E = case.B, case.N, case.E
    H = torch.zeros(B, E, N)
    wts = torch.tensor([1.0, 2.0, 0.5])
    for b in range(B):
        for e in range(E):
            cnt = case.members
            if E >= 3 and case.members < N:     # one empty (a) or one-member (f) row, one full row
                if e == 0:
                    cnt = 0 if case.N == 11 else 1
                elif e == 1:
                    cnt = N
            idx = torch.randperm(N, generator=g)[:cnt]
            H[b, e, idx] = wts[torch.randint(0, 3, (cnt,), generator=g)] if case.members < N or case.name == "g" \
                else 1.0
    return H


@functools.lru_cache(maxsize=None)
def n2e_inputs(case: N2ECase, self_w: float = 2.0) -> Dict[str, torch.Tensor]:
    """fp32 CPU tensors of a pooling case (H is the explicit incidence also where the kernel gets H == NULL)."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    B, N, E = case.B, case.N, case.E
    R = lambda *s: torch.randn(*s, generator=g)
    if case.kind == "hyper":
        H = _hyper_H(case, g)
    else:
        H = pair_incidence(N, case.kind == "sym", self_w)[None].repeat(B, 1, 1)
    assert tuple(H.shape) == (B, E, N)
    pq = torch.randint(-128, 129, (B, N, 64), generator=g).float() / 64
    dedges = R(B, E, 64)
    if case.zero_scene >= 0:
        dedges[case.zero_scene] = 0
    elif case.zero_scene == -2:
        dedges.zero_()
    return dict(xp=R(B, N, 64), pq=pq, H=H, w2=R(32) * case.w2_scale, b2=R(1), dedges=dedges,
                dxp0=R(B, N, 64), dpq0=R(B, N, 64), dw20=R(32), db20=R(1))


@functools.lru_cache(maxsize=None)
def n2e_expected(case: N2ECase):
    inp = n2e_inputs(case)
    return n2e_grads(inp, F64), n2e_grads(inp, F32)


N2E_OUTPUTS = ("dxp", "dpq", "dw2", "db2")


def n2e_scale(r64: dict, out: str) -> float:
    return r64[out + "_scale"] if out in ("dw2", "db2") else float(r64[out].abs().max())


# ------------------------------------------------------------------------------------------------------------------
# Gumbel stages (gn_gumbel_ef_f32, gn_gumbel_bwd[_grouped]_f32)
# ------------------------------------------------------------------------------------------------------------------
GUMBEL_FLAWS = ("diagonal_twice", "gdist_ignored", "no_inverse_tau")


def sym_edge_rows(B: int, N: int):
    """Pair row r = (b, i, j >= i) -> its ordered dist rows e0 = (b, i, j), e1 = (b, j, i) (e1 = -1 on the diagonal)."""
    ii, jj = torch.triu_indices(N, N)           # row-major upper triangle = gn_pair_decode order
    b = torch.arange(B)[:, None]
    e0 = ((b * N + ii) * N + jj).reshape(-1)
    e1 = ((b * N + jj) * N + ii).reshape(-1)
    return e0, torch.where(e0 == e1, torch.full_like(e1, -1), e1)


def gumbel_ref(logits, f, g, tau, sym_N=0, diag_w=1.0, flaw=None):
    """dist (ordered rows, K) and ef (rows, K).  logits (rows, K), f (rows,), noise g (ordered rows, K)."""
    if flaw == "no_inverse_tau":        # the same values, d y / d logits = 1
        inv = lambda x: x + (x.detach() / tau - x.detach())
    else:
        inv = lambda x: x / tau
    sig = torch.sigmoid(f)[:, None]
    if sym_N <= 0:
        dist = torch.softmax(inv(logits) + g / tau, dim=-1)
        return dist, sig * dist
    P = pair_count(sym_N)
    e0, e1 = sym_edge_rows(logits.shape[0] // P, sym_N)
    off = e1 >= 0
    row_of = torch.empty(g.shape[0], dtype=torch.long)
    row_of[e0] = torch.arange(e0.numel())
    row_of[e1[off]] = torch.arange(e0.numel())[off]
    dist = torch.softmax(inv(logits)[row_of] + g / tau, dim=-1)
    second = torch.where(off[:, None], dist[e1.clamp_min(0)], torch.zeros_like(dist[e0]))
    if flaw == "diagonal_twice":
        second = torch.where(off[:, None], second, dist[e0])
    w = torch.where(off, torch.ones_like(f), torch.full_like(f, diag_w))[:, None]
    return dist, sig * (dist[e0] + second) * w


def gumbel_grads(inp, dtype, flaw=None, with_gdist=True):
    """ef (with the case's diag_w), dist, and dlgf (rows, K+1) = [d logits | d f] of <ef, def> + <dist, gdist> at
    diag_w = 1 (the backward kernel has no such argument)."""
    c = lambda k: inp[k].to(dtype)
    logits, f = c("logits").requires_grad_(True), c("f").requires_grad_(True)
    tau, sym_N = inp["tau"], inp["sym_N"]
    dist, ef = gumbel_ref(logits, f, c("g"), tau, sym_N, 1.0, flaw)
    loss = (ef * c("def")).sum()
    if with_gdist and flaw != "gdist_ignored":
        loss = loss + (dist * c("gdist")).sum()
        if flaw == "diagonal_twice" and sym_N > 0:
            e0, e1 = sym_edge_rows(logits.shape[0] // pair_count(sym_N), sym_N)
            loss = loss + (dist[e0[e1 < 0]] * c("gdist")[e0[e1 < 0]]).sum()
    dl, df = torch.autograd.grad(loss, (logits, f))
    with torch.no_grad():
        _, ef_w = gumbel_ref(logits, f, c("g"), tau, sym_N, inp["diag_w"], None)
    return dict(dist=dist.detach(), ef=ef_w, dlgf=torch.cat((dl, df[:, None]), dim=1))


@dataclass(frozen=True)
class GumbelCase:
    name: str
    rows: int            # rows of lgf / def / dlgf / ef (B * P with sym_N)
    K: int
    sym_N: int = 0
    diag_w: float = 1.0
    ld_ef: int = 0       # 0: K
    logit_scale: float = 1.0
    seed: int = 0
    saturated: bool = True   # the first rows carry f = +-30, +-100


LDL, TAU = 32, 0.5
GUMBEL_CASES = [
    GumbelCase("k6", 37, 6, seed=1),
    GumbelCase("k10_ld12_x8", 37, 10, ld_ef=12, logit_scale=8.0, seed=2),
    GumbelCase("k6_sym1_w2", 7, 6, sym_N=1, diag_w=2.0, ld_ef=12, seed=3),
    GumbelCase("k10_sym5_w2_x8", 3 * 15, 10, sym_N=5, diag_w=2.0, logit_scale=8.0, seed=4),
    GumbelCase("k6_sym5", 3 * 15, 6, sym_N=5, ld_ef=12, seed=5),
]
GUMBEL_STRIDE_CASES = [      # past 4096 workgroups x 256 rows
    GumbelCase("k6_stride", 1_048_876, 6, seed=6, saturated=False),
    GumbelCase("k6_sym11_stride", 15_889 * 66, 6, sym_N=11, seed=7, saturated=False),
]
GUMBEL_GROUPED = [GUMBEL_CASES[0], GUMBEL_CASES[3], GUMBEL_CASES[4]]     # different rows, K, sym_N


def grid_stride(items: int, per_block: int, cap: int = 4096) -> bool:
    """cap_grid of gn_backward.hip: is the launch's grid-stride loop taken a second time?"""
    return cdiv(items, per_block) > cap


@functools.lru_cache(maxsize=None)
def gumbel_inputs(case: GumbelCase):
    g = torch.Generator().manual_seed(2000 + case.seed)
    rows, K, N = case.rows, case.K, case.sym_N
    orows = rows if N <= 0 else rows // pair_count(N) * N * N
    logits = torch.randn(rows, K, generator=g) * case.logit_scale
    f = torch.randn(rows, generator=g)
    if case.saturated:
        f[:4] = torch.tensor([30.0, -30.0, 100.0, -100.0])
    U = torch.rand(orows, K, generator=g)
    noise = -torch.log(1e-10 - torch.log(U + 1e-10))
    return dict(logits=logits, f=f, g=noise, tau=TAU, sym_N=N, diag_w=case.diag_w,
                gdist=torch.randn(orows, K, generator=g), **{"def": torch.randn(rows, K, generator=g)})


@functools.lru_cache(maxsize=None)
def gumbel_expected(case: GumbelCase, with_gdist: bool = True):
    inp = gumbel_inputs(case)
    return gumbel_grads(inp, F64, None, with_gdist), gumbel_grads(inp, F32, None, with_gdist)


# ------------------------------------------------------------------------------------------------------------------
# typed-MLP middle (gn_typed_bwd_f32)
# ------------------------------------------------------------------------------------------------------------------
TYPED_FLAWS = ("b2_term_missing", "mask_from_T")
TYPED_CASES = [(37, 10, 128, 12), (66, 6, 128, 8), (5, 1, 64, 1), (32_773, 2, 64, 4)]     # rows, K, hid, ld_ef


@functools.lru_cache(maxsize=None)
def typed_inputs(case):
    rows, K, hid, ld_ef = case
    g = torch.Generator().manual_seed(3000 + rows)
    R = lambda *s: torch.randn(*s, generator=g)
    pre, W2, dfeat = R(rows, K, hid), R(K, 64, hid) / hid ** 0.5, R(rows, 64)
    T = torch.einsum("ro,koh->rkh", dfeat.double(), W2.double()).float()
    return dict(ef=R(rows, K), pre=pre, W2=W2, b2=R(K, 64), dfeat=dfeat, Hc=torch.relu(pre), T=T)


def typed_grads(inp, dtype, flaw=None):
    """def (rows, K) and the gradient of the pre-activations (rows, K, hid) of <feat, dfeat>,
    feat = sum_k ef_k (relu(pre_k) W2_k^T + b2_k)."""
    c = lambda k: inp[k].to(dtype)
    ef, pre = c("ef").requires_grad_(True), c("pre").requires_grad_(True)
    y = torch.einsum("rkh,koh->rko", torch.relu(pre), c("W2"))
    if flaw != "b2_term_missing":
        y = y + c("b2")
    feat = (ef[:, :, None] * y).sum(dim=1)
    d_ef, d_pre = torch.autograd.grad((feat * c("dfeat")).sum(), (ef, pre))
    if flaw == "mask_from_T":
        T = torch.einsum("ro,koh->rkh", c("dfeat"), c("W2"))
        d_pre = ef.detach()[:, :, None] * T * (T > 0)
    return {"def": d_ef, "T": d_pre}


@functools.lru_cache(maxsize=None)
def typed_expected(case):
    inp = typed_inputs(case)
    return typed_grads(inp, F64), typed_grads(inp, F32)


# ------------------------------------------------------------------------------------------------------------------
# gn_axpby2d_f32
# ------------------------------------------------------------------------------------------------------------------
AXPBY_CASES = [(rows, cols, ab) for rows, cols in ((37, 5), (4100, 260))
               for ab in ((1.0, 1.0), (0.5, 0.0), (-2.0, 0.25))]      # 185 and 1 066 000 elements (grid cap: 1 048 576)


def axpby_ref(out0, a, alpha, beta):
    """alpha*a + beta*out, each operation rounded in the tensors' dtype (beta = 0: out is not read)."""
    v = alpha * a
    return v if beta == 0 else v + beta * out0


# ------------------------------------------------------------------------------------------------------------------
# GEMM (gn_gemm_grouped_f32, gn_gemm_f32)
# ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GemmCase:
    name: str
    M: int
    N: int
    K: int
    tA: bool = False
    tB: bool = False
    pad: int = 4             # leading dimension = width + pad for A, B
    ldc: int = 0             # 0: width + 4
    offA: int = 0            # floats between the 16-byte-aligned buffer start and the operand
    offC: int = 0
    bias: bool = False
    relu: bool = False
    mask: bool = False       # ldmask = N + 4
    alpha: float = 1.0
    beta: float = 0.0
    rs: int = 0              # 0: none, else rs_ld (rs = column 1 of a (stored rows, rs_ld) tensor; 1: a vector)
    colsum: bool = False
    accum: bool = False
    tC: bool = False
    select: str = ""         # "A" | "B": that operand is a selection matrix (exactness probe), C starts at 0
    seed: int = 0

    @property
    def a_shape(self):
        return (self.K, self.M) if self.tA else (self.M, self.K)

    @property
    def b_shape(self):
        return (self.N, self.K) if self.tB else (self.K, self.N)

    @property
    def c_shape(self):
        return (self.N, self.M) if self.tC else (self.M, self.N)

    @property
    def lda(self):
        return self.a_shape[1] + self.pad

    @property
    def ldb(self):
        return self.b_shape[1] + self.pad

    @property
    def ldc_(self):
        return self.ldc or self.c_shape[1] + 4


def gemm_vec(c: GemmCase) -> bool:
    """gn_gemm_grouped_f32's `vec` rule (buffers start 16-byte aligned; B and C never start off it here)."""
    return (c.offA % 4 == 0 and c.lda % 4 == 0 and c.ldb % 4 == 0 and c.K % 32 == 0 and (not c.tA or c.M % 4 == 0)
            and (c.tB or c.N % 4 == 0))


def gemm_splits(M: int, N: int, K: int, accum: bool) -> int:
    tiles, s = cdiv(M, 128) * cdiv(N, 64), 1
    if accum:
        s = min(cdiv(512, tiles), cdiv(K, 256))
    kchunk = cdiv(cdiv(K, s), 32) * 32
    return cdiv(K, kchunk)


def gemm_f32_accum(M, N, K, plain_epilogue: bool) -> bool:
    """gn_gemm_f32's own rule for the weight-gradient route (scale_kernel, then split-K atomics)."""
    return cdiv(M, 128) * cdiv(N, 64) < 128 and K >= 4096 and plain_epilogue


_EPI = [dict(), dict(bias=True, relu=True), dict(mask=True), dict(alpha=0.5, beta=0.25, ldc=136, offC=64)]
_VEC_SHAPES = [(4, 4, 32), (128, 64, 32), (132, 68, 64), (260, 200, 256)]
_RAGGED = [(1, 1, 1), (130, 70, 33), (64, 200, 5), (33, 7, 40)]


def _epi(i, N):
    e = dict(_EPI[i % 4])
    if "ldc" in e:
        e["ldc"] = N + 72
    return e


# one GemmBatch: 16 vector-path problems ((tA, tB) x shape, the epilogue rotating so that every (tA, tB) meets every
# epilogue), 17 scalar-path ones, and the same (132, 68, 64) problem one float off alignment
GEMM_BATCH = (
    [GemmCase(f"vec{i}", *_VEC_SHAPES[i // 4], tA=bool(i & 1), tB=bool(i & 2), seed=i, **_epi(i + i // 4, _VEC_SHAPES[i // 4][1]))
     for i in range(16)]
    + [GemmCase(f"ragged{i}", *_RAGGED[i % 4], tA=bool(i & 1), tB=bool(i & 2), pad=3, seed=20 + i,
                **_epi(i // 4 + i, _RAGGED[i % 4][1])) for i in range(17)]
    + [GemmCase("vec_aligned", 132, 68, 64, seed=40), GemmCase("scalar_by_misalignment", 132, 68, 64, offA=1, seed=40)])
GEMM_ACCUM = (
    [GemmCase(f"dW_colsum_rs_K{K}", 96, 64, K, tA=True, accum=True, rs=3, colsum=True, seed=50 + i)
     for i, K in enumerate((256, 288, 300, 8224))]
    + [GemmCase("deo_rs_plain_A", 198, 64, 768, accum=True, rs=1, seed=60),
       GemmCase("dW2k_tC_production", 128, 64, 2080, tA=True, accum=True, tC=True, rs=12, seed=61),
       GemmCase("dW2k_tC_ragged", 192, 68, 2077, tA=True, accum=True, tC=True, rs=12, pad=1, seed=62),
       # A = dpq[:, :32], C = ga0[:, 64:]
       GemmCase("column_slices", 198, 64, 32, pad=32, ldc=128, offC=64, seed=63)])
GEMM_PROBES = [GemmCase(f"probe_select{s}{'_tC' if tC else ''}", 128, 64, 64, tA=tC, accum=tC, tC=tC, select=s, seed=70 + i)
               for i, (s, tC) in enumerate((("B", False), ("A", False), ("B", True), ("A", True)))]
GEMM_SINGLE = [GemmCase("single_plain", 100, 60, 40, pad=0, ldc=60, seed=80),
               GemmCase("single_dW_beta", 96, 64, 4096, tA=True, pad=0, ldc=68, beta=0.5, seed=81),
               GemmCase("single_dW_beta0", 96, 64, 4096, tA=True, pad=0, ldc=68, seed=82)]


def view2d(buf: torch.Tensor, rows: int, cols: int, ld: int, off: int = 0) -> torch.Tensor:
    return buf.as_strided((rows, cols), (ld, 1), off)


def _buf(rows, ld, off, g, fill=None):
    n = off + rows * ld
    return torch.randn(n, generator=g) if fill is None else torch.full((n,), fill)


def _selection(shape, along_rows: bool, g) -> torch.Tensor:
    """One entry +-2^k per column (or per row), the rest 0."""
    S = torch.zeros(shape)
    n = shape[0] if along_rows else shape[1]
    depth = shape[1] if along_rows else shape[0]
    pos = torch.randint(0, depth, (n,), generator=g)
    val = torch.ldexp(torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0), torch.randint(-6, 7, (n,), generator=g))
    if along_rows:
        S[torch.arange(n), pos] = val
    else:
        S[pos, torch.arange(n)] = val
    return S


@functools.lru_cache(maxsize=None)
def gemm_inputs(c: GemmCase):
    """Flat fp32 buffers (as the device will hold them) of one problem; operands are views at (ld, offset)."""
    g = torch.Generator().manual_seed(4000 + c.seed)
    (ar, ac), (br, bc), (cr, cc) = c.a_shape, c.b_shape, c.c_shape
    A = torch.zeros(c.offA + ar * c.lda)
    A[c.offA:] = torch.randn(ar * c.lda, generator=g)        # the same values at every offset
    Bm = _buf(br, c.ldb, 0, g)
    fresh = not c.accum and c.beta == 0
    C0 = _buf(cr, c.ldc_, c.offC, g, float("nan") if fresh else None)
    d = dict(A=A, B=Bm, C0=C0)
    if c.select:
        C0.zero_()
        sel_is_a = c.select == "A"
        shape = c.a_shape if sel_is_a else c.b_shape
        # A: one entry per m; B: one entry per n (k is the other axis of the stored operand)
        along_rows = (not c.tA) if sel_is_a else c.tB
        view2d(A if sel_is_a else Bm, *shape, c.lda if sel_is_a else c.ldb,
               c.offA if sel_is_a else 0).copy_(_selection(shape, along_rows, g))
    if c.bias:
        d["bias"] = torch.randn(c.N, generator=g)
    if c.mask:
        d["mask"] = torch.randn(c.M * (c.N + 4), generator=g)
    if c.rs:
        d["rs"] = torch.rand(ar * c.rs, generator=g) + 0.25
    if c.colsum:
        d["colsum0"] = torch.randn(c.M, generator=g)
    return d


def gemm_ref(c: GemmCase, d, dtype):
    """(C buffer as it must be afterwards, flat; colsum or None; colsum scale) evaluated in `dtype`."""
    A = view2d(d["A"], *c.a_shape, c.lda, c.offA).to(dtype)
    Bm = view2d(d["B"], *c.b_shape, c.ldb).to(dtype)
    if c.rs:
        A = A * view2d(d["rs"], c.a_shape[0], 1, c.rs, 1 if c.rs > 1 else 0).to(dtype)
    P = c.alpha * ((A.t() if c.tA else A) @ (Bm.t() if c.tB else Bm))
    out = d["C0"].to(dtype).clone()
    Cv = view2d(out, *c.c_shape, c.ldc_, c.offC)
    if c.accum:
        Cv += P.t() if c.tC else P
    else:
        if c.bias:
            P = P + d["bias"].to(dtype)
        if c.beta != 0:
            P = P + c.beta * Cv
        if c.relu:
            P = P.clamp_min(0)
        if c.mask:
            P = torch.where(view2d(d["mask"], c.M, c.N, c.N + 4) > 0, P, torch.zeros_like(P))
        Cv.copy_(P)
    cs = cs_scale = None
    if c.colsum:
        cs = d["colsum0"].to(dtype) + A.sum(0)
        cs_scale = float((d["colsum0"].to(dtype).abs() + A.abs().sum(0)).max())
    return out, cs, cs_scale


@functools.lru_cache(maxsize=None)
def gemm_expected(c: GemmCase):
    d = gemm_inputs(c)
    return gemm_ref(c, d, F64), gemm_ref(c, d, F32)


def gemm_ceiling(c: GemmCase, single: bool = False) -> float:
    from test_backward_gpu import TOL_CLEAN
    split = c.accum or (single and gemm_f32_accum(c.M, c.N, c.K, not (c.bias or c.mask or c.relu)))
    return SPLITK_CEILING if split and c.K >= 4096 else TOL_CLEAN


def c_scale(c: GemmCase, ref64_buf: torch.Tensor) -> float:
    return float(view2d(ref64_buf, *c.c_shape, c.ldc_, c.offC).abs().max())
