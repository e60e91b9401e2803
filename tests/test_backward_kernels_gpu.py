"""Every backward kernel of gn_backward.hip alone, through the C ABI, against a float64 statement of the same operation
(tests/backward_kernel_refs.py) at the smallest shapes that reach each launcher form and edge.

Gate (backward_kernel_refs.gate): max|hip - ref64| <= max(4 * max|ref32 - ref64|, 2^-22 * scale), never above TOL_CLEAN
(1e-4 on the K >= 4096 split-K cases) of scale; ref32 is the same reference in float32 on the CPU.  In-out buffers start
from random values (the kernels ADD), write-only buffers start NaN-filled.  Every test prints measured / e32 / gate."""
import math

import pytest
import torch

import backward_kernel_refs as R
from test_backward_gpu import TOL_CLEAN

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _api():
    from groupnet_amd import _lib
    return _lib, _lib.load(), torch.device("cuda:0")


def _within(bad, tag, out, hip, r64, r32, scale, ceiling=TOL_CLEAN):
    bound, e32 = R.gate(r64, r32, scale)
    bound = min(bound, ceiling * scale)
    err = float((hip.detach().double().cpu() - r64).abs().max()) if r64.numel() else 0.0
    print(f"\n{tag} {out}: measured {err:.2e} / e32 {e32:.2e} / gate {bound:.2e}  (scale {scale:.2e}, "
          f"measured/e32 {err / e32 if e32 > 0 else float('inf'):.2f})", end="")
    if not err <= bound:        # (NaN fails)
        bad.append((tag, out, err, e32, bound))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- attention pooling ----------------------------------------------------------------------------------------------
def _n2e_buffers(case, dev):
    d = {k: v.to(dev) for k, v in R.n2e_inputs(case).items()}
    out = {o: d[o + "0"].clone() for o in R.N2E_OUTPUTS}
    return d, out


def _n2e_verdict(bad, case, d, out):
    r64, r32 = R.n2e_expected(case)
    for o in R.N2E_OUTPUTS:
        _within(bad, f"n2e_bwd {case.name} (B={case.B} N={case.N} E={case.E} {case.kind})", o, out[o], r64[o], r32[o],
                R.n2e_scale(r64, o))
    scenes = [case.zero_scene] if case.zero_scene >= 0 else (list(range(case.B)) if case.zero_scene == -2 else [])
    for z in scenes:      # no write across scenes: a scene without gradient keeps its start values to the bit
        assert torch.equal(_bits(out["dxp"][z]), _bits(d["dxp0"][z])), (case.name, "dxp", z)
        assert torch.equal(_bits(out["dpq"][z]), _bits(d["dpq0"][z])), (case.name, "dpq", z)


@pytest.mark.parametrize("case", R.N2E_CASES, ids=lambda c: c.name)
def test_node2edge_bwd(case):
    L, lib, dev = _api()
    d, out = _n2e_buffers(case, dev)
    H = d["H"] if case.kind == "hyper" else None
    assert R.n2e_form(case.N, H is not None) != "error"
    with torch.cuda.device(dev):
        L.check(lib.gn_node2edge_bwd_f32(L.addr(d["xp"]), L.addr(d["pq"]), L.addr(H), L.addr(d["w2"]), L.addr(d["b2"]),
                                         L.addr(d["dedges"]), L.addr(out["dxp"]), L.addr(out["dpq"]), L.addr(out["dw2"]),
                                         L.addr(out["db2"]), case.B, case.N, case.E, int(case.kind == "sym"),
                                         L.stream_handle()), "gn_node2edge_bwd_f32")
    torch.cuda.synchronize()
    bad = []
    _n2e_verdict(bad, case, d, out)
    assert not bad, bad


def test_node2edge_bwd_grouped():
    """sym pairwise, ordered pairwise (all-zero dedges: its buffers come back unchanged), hyper E = N and hyper E = 1 in one
    launch, each group with its own inputs and outputs."""
    L, lib, dev = _api()
    bufs = [_n2e_buffers(c, dev) for c in R.N2E_GROUPED]
    groups = [L.N2EBwdGroup(xp=L.addr(d["xp"]), pq=L.addr(d["pq"]), H=L.addr(d["H"] if c.kind == "hyper" else None),
                            w2=L.addr(d["w2"]), b2=L.addr(d["b2"]), dedges=L.addr(d["dedges"]), dxp=L.addr(o["dxp"]),
                            dpq=L.addr(o["dpq"]), dw2=L.addr(o["dw2"]), db2=L.addr(o["db2"]), E=c.E,
                            sym=int(c.kind == "sym")) for c, (d, o) in zip(R.N2E_GROUPED, bufs)]
    arr = (L.N2EBwdGroup * len(groups))(*groups)
    with torch.cuda.device(dev):
        L.check(lib.gn_node2edge_bwd_grouped_f32(arr, len(groups), 3, 11, L.stream_handle()), "gn_node2edge_bwd_grouped_f32")
    torch.cuda.synchronize()
    bad = []
    for c, (d, o) in zip(R.N2E_GROUPED, bufs):
        _n2e_verdict(bad, c, d, o)
        if c.zero_scene == -2:
            assert torch.equal(_bits(o["dw2"]), _bits(d["dw20"])) and torch.equal(_bits(o["db2"]), _bits(d["db20"]))
    assert not bad, bad


# ---- Gumbel stages --------------------------------------------------------------------------------------------------
def _gumbel_device(case, dev, with_gdist=True):
    inp = R.gumbel_inputs(case)
    r64, r32 = R.gumbel_expected(case, with_gdist)
    g = torch.Generator().manual_seed(case.seed)
    lgf = torch.randn(case.rows, R.LDL, generator=g)
    lgf[:, :case.K], lgf[:, case.K] = inp["logits"], inp["f"]
    d = dict(dist=r64["dist"].float().to(dev), lgf=lgf.to(dev), gdist=inp["gdist"].to(dev) if with_gdist else None)
    d["def"] = inp["def"].to(dev)
    return d, r64, r32


def _gumbel_ef(case):
    L, lib, dev = _api()
    d, r64, r32 = _gumbel_device(case, dev)
    K, ld = case.K, case.ld_ef or case.K
    ef0 = torch.randn(case.rows, ld)
    ef0[:, :K] = NAN
    ef = ef0.to(dev)
    with torch.cuda.device(dev):
        L.check(lib.gn_gumbel_ef_f32(L.addr(d["dist"]), L.addr(d["lgf"]), L.addr(ef), case.rows, K, R.LDL, case.sym_N,
                                     case.diag_w, ld, L.stream_handle()), "gn_gumbel_ef_f32")
    torch.cuda.synchronize()
    assert torch.equal(_bits(ef[:, K:]), _bits(ef0[:, K:]))      # the padding columns keep their content
    bad = []
    _within(bad, f"gumbel_ef {case.name} (rows={case.rows} K={K} sym_N={case.sym_N} diag_w={case.diag_w:g} ld_ef={ld})", "ef",
            ef[:, :K], r64["ef"], r32["ef"], float(r64["ef"].abs().max()))
    assert not bad, bad


def _gumbel_bwd_launch(case, d):
    L, lib, dev = _api()
    dlgf = torch.full((case.rows, R.LDL), NAN, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.gn_gumbel_bwd_f32(L.addr(d["dist"]), L.addr(d["lgf"]), L.addr(d["def"]), L.addr(d["gdist"]),
                                      L.addr(dlgf), case.rows, case.K, R.LDL, R.TAU, case.sym_N, L.stream_handle()),
                "gn_gumbel_bwd_f32")
    torch.cuda.synchronize()
    return dlgf


def _gumbel_bwd(case, with_gdist):
    _, _, dev = _api()
    d, r64, r32 = _gumbel_device(case, dev, with_gdist)
    dlgf = _gumbel_bwd_launch(case, d)
    K = case.K
    assert bool(torch.isfinite(dlgf).all())
    assert not bool(dlgf[:, K + 1:].any())               # columns K+1 .. ldl-1 exactly 0
    bad = []
    _within(bad, f"gumbel_bwd {case.name} (rows={case.rows} K={K} sym_N={case.sym_N} x{case.logit_scale:g} "
                 f"gdist={'yes' if with_gdist else 'NULL'})", "dlgf", dlgf[:, :K + 1], r64["dlgf"], r32["dlgf"],
            float(r64["dlgf"].abs().max()))
    if case.saturated:      # f = +-30, +-100: the sigmoid saturates and d f goes to 0
        assert float(dlgf[:4, K].abs().max()) <= 1e-10 * float(r64["dlgf"].abs().max())
    assert not bad, bad


@pytest.mark.parametrize("case", R.GUMBEL_CASES + R.GUMBEL_STRIDE_CASES, ids=lambda c: c.name)
def test_gumbel_ef(case):
    _gumbel_ef(case)


@pytest.mark.parametrize("with_gdist", [True, False], ids=["gdist", "gdist_null"])
@pytest.mark.parametrize("case", R.GUMBEL_CASES, ids=lambda c: c.name)
def test_gumbel_bwd(case, with_gdist):
    _gumbel_bwd(case, with_gdist)


@pytest.mark.parametrize("case", R.GUMBEL_STRIDE_CASES, ids=lambda c: c.name)
def test_gumbel_bwd_grid_stride(case):
    _gumbel_bwd(case, True)


def test_gumbel_bwd_grouped_equals_the_single_launches():
    """Three groups with their own rows, K and sym_N, the last with gdist == NULL: bit-identical to the single launches
    (no atomics: the arithmetic is fixed), which the tests above gate against float64."""
    L, lib, dev = _api()
    cases = R.GUMBEL_GROUPED
    ds = [_gumbel_device(c, dev, with_gdist=i < 2)[0] for i, c in enumerate(cases)]
    singles = [_gumbel_bwd_launch(c, d) for c, d in zip(cases, ds)]
    outs = [torch.full((c.rows, R.LDL), NAN, device=dev) for c in cases]
    arr = (L.GumbelBwdGroup * len(cases))(*[
        L.GumbelBwdGroup(dist=L.addr(d["dist"]), lgf=L.addr(d["lgf"]), def_=L.addr(d["def"]), gdist=L.addr(d["gdist"]),
                         dlgf=L.addr(o), rows=c.rows, K=c.K, sym_N=c.sym_N) for c, d, o in zip(cases, ds, outs)])
    assert len({(c.rows, c.K, c.sym_N) for c in cases}) == 3
    with torch.cuda.device(dev):
        L.check(lib.gn_gumbel_bwd_grouped_f32(arr, len(cases), R.LDL, R.TAU, L.stream_handle()), "gn_gumbel_bwd_grouped_f32")
    torch.cuda.synchronize()
    for c, a, b in zip(cases, singles, outs):
        assert bool(torch.isfinite(b).all()) and torch.equal(_bits(a), _bits(b)), c.name


# ---- typed-MLP middle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.TYPED_CASES, ids=str)
def test_typed_bwd(case):
    L, lib, dev = _api()
    rows, K, hid, ld_ef = case
    inp = R.typed_inputs(case)
    r64, r32 = R.typed_expected(case)
    ef = torch.randn(rows, ld_ef)
    ef[:, :K] = inp["ef"]
    T = inp["T"].reshape(rows, K * hid).to(dev)
    Hc, ef, dfeat, b2 = (t.to(dev) for t in (inp["Hc"].reshape(rows, K * hid), ef, inp["dfeat"], inp["b2"]))
    d_ef = torch.full((rows, K), NAN, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.gn_typed_bwd_f32(L.addr(T), L.addr(Hc), L.addr(ef), ld_ef, L.addr(dfeat), L.addr(b2), L.addr(d_ef),
                                     rows, K, hid, L.stream_handle()), "gn_typed_bwd_f32")
    torch.cuda.synchronize()
    assert not bool(T[Hc == 0].any())                       # exactly 0 where the unit is off
    bad = []
    tag = f"typed_bwd (rows={rows} K={K} hid={hid} ld_ef={ld_ef})"
    _within(bad, tag, "def", d_ef, r64["def"], r32["def"], float(r64["def"].abs().max()))
    _within(bad, tag, "T", T.view(rows, K, hid), r64["T"], r32["T"], float(r64["T"].abs().max()))
    assert not bad, bad


# ---- axpby -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,ab", R.AXPBY_CASES, ids=lambda v: str(v))
def test_axpby2d(rows, cols, ab):
    """Column slices with ldo != lda != cols; alpha and beta are powers of two, so a fused multiply-add rounds as the
    per-operation fp32 expression does: exact equality, and nothing outside the slice moves."""
    L, lib, dev = _api()
    alpha, beta = ab
    g = torch.Generator().manual_seed(rows)
    ldo, lda = cols + 7, cols + 2
    out0, a = torch.randn(rows, ldo, generator=g), torch.randn(rows, lda, generator=g)
    if beta == 0:
        out0[:, 3:3 + cols] = NAN
    out, a_dev = out0.to(dev), a.to(dev)
    with torch.cuda.device(dev):
        L.check(lib.gn_axpby2d_f32(L.addr(out[:, 3:]), ldo, L.addr(a_dev[:, 1:]), lda, rows, cols, alpha, beta,
                                   L.stream_handle()), "gn_axpby2d_f32")
    torch.cuda.synchronize()
    want = out0.clone()
    want[:, 3:3 + cols] = R.axpby_ref(out0[:, 3:3 + cols], a[:, 1:1 + cols], alpha, beta)
    assert torch.equal(_bits(out), _bits(want))


# ---- GEMM -------------------------------------------------------------------------------------------------------------
def _gemm_add(gb, c, dev):
    """Adds case c to the batch; returns what the verdict needs."""
    d = {k: v.to(dev) for k, v in R.gemm_inputs(c).items()}
    A = R.view2d(d["A"], *c.a_shape, c.lda, c.offA)
    Bm = R.view2d(d["B"], *c.b_shape, c.ldb)
    Cbuf = d["C0"].clone()
    C = R.view2d(Cbuf, *c.c_shape, c.ldc_, c.offC)
    assert (A.data_ptr() % 16 == 0) == (c.offA % 4 == 0) and Bm.data_ptr() % 16 == 0     # what gemm_vec assumes
    mask = R.view2d(d["mask"], c.M, c.N, c.N + 4) if c.mask else None
    rs = d["rs"].as_strided((c.a_shape[0],), (c.rs,), 1 if c.rs > 1 else 0) if c.rs else None
    cs = d["colsum0"].clone() if c.colsum else None
    gb.add(A, Bm, C, c.tA, c.tB, d.get("bias"), mask, c.relu, c.alpha, c.beta, rs=rs, colsum=cs, accum=c.accum, tC=c.tC)
    return Cbuf, cs


def _gemm_verdict(bad, c, Cbuf, cs, single=False):
    (c64, cs64, cs_scale), (c32, cs32, _) = R.gemm_expected(c)
    inside = torch.zeros(c64.numel(), dtype=torch.bool)
    R.view2d(inside, *c.c_shape, c.ldc_, c.offC).fill_(True)
    hip = Cbuf.cpu()
    C0 = R.gemm_inputs(c)["C0"]
    assert torch.equal(_bits(hip[~inside]), _bits(C0[~inside])), (c.name, "wrote outside C")
    ceiling = R.gemm_ceiling(c, single)
    path = "vector" if R.gemm_vec(c) else "scalar"
    splits = R.gemm_splits(c.M, c.N, c.K, c.accum or (single and R.gemm_f32_accum(c.M, c.N, c.K, True)))
    tag = f"gemm {c.name} (M={c.M} N={c.N} K={c.K} tA={int(c.tA)} tB={int(c.tB)} tC={int(c.tC)} {path}, {splits} split)"
    _within(bad, tag, "C", hip[inside], c64[inside], c32[inside], R.c_scale(c, c64), ceiling)
    if c.colsum:
        _within(bad, tag, "colsum", cs, cs64, cs32, cs_scale, ceiling)


def _run_gemm_cases(cases):
    from groupnet_amd.backward import GemmBatch
    _, _, dev = _api()
    gb = GemmBatch()
    held = [_gemm_add(gb, c, dev) for c in cases]
    gb.run()
    torch.cuda.synchronize()
    bad = []
    for c, (Cbuf, cs) in zip(cases, held):
        _gemm_verdict(bad, c, Cbuf, cs)
    assert not bad, bad


def test_gemm_vector_and_scalar_kernels_in_one_batch():
    """The four (tA, tB) stagings of the vector kernel at (4,4,32) .. (260,200,256) with every epilogue (beta = 0 onto NaN,
    bias + ReLU, mask with ldmask > N, alpha/beta on a column-sliced C), 17 scalar-path problems in between so that both
    descriptor tables flush, and the (132,68,64) problem aligned and one float off alignment (same values, same
    reference)."""
    order = [c for pair in zip(R.GEMM_BATCH[:16], R.GEMM_BATCH[16:32]) for c in pair] + R.GEMM_BATCH[32:]
    assert len(order) == len(R.GEMM_BATCH)
    _run_gemm_cases(order)


def test_gemm_accumulate_modes():
    """tA + colsum + rs at K = 256 (no split), 288 / 300 (two uneven splits, vector / scalar), 8224 (33 splits); rs on a
    plain A; tC with rs a column of a (rows, 12) tensor at the production shape and a ragged one; column-slice operands."""
    _run_gemm_cases(R.GEMM_ACCUM)


def test_gemm_three_part_products_are_exact_to_one_rounding():
    """Selection-matrix probe of the vector kernel's bf16 three-part split: every output is ONE product a * (+-2^k), all
    other terms exact zeros.  |C - ref| <= 2^-23 |ref| element-wise; a lost part-product shows as about 2^-17.  Either
    operand as the selection matrix, without and with GN_GEMM_TRANS_C (operands swapped in the MFMA call)."""
    from groupnet_amd.backward import GemmBatch
    _, _, dev = _api()
    gb = GemmBatch()
    held = [_gemm_add(gb, c, dev) for c in R.GEMM_PROBES]
    gb.run()
    torch.cuda.synchronize()
    for c, (Cbuf, _) in zip(R.GEMM_PROBES, held):
        ref = R.gemm_expected(c)[0][0]
        err = (Cbuf.cpu().double() - ref).abs()
        worst = float((err / ref.abs().clamp_min(1e-300))[ref != 0].max())
        print(f"\ngemm {c.name}: worst relative error {worst:.2e} (2^{math.log2(max(worst, 1e-30)):.1f}), gate 2^-23",
              end="")
        assert bool((err <= R.PROBE_REL * ref.abs()).all()), (c.name, worst)


@pytest.mark.parametrize("case", R.GEMM_SINGLE, ids=lambda c: c.name)
def test_gemm_f32_entry_point(case):
    """gn_gemm_f32 itself: a plain problem, and its own weight-gradient route (K >= 4096 over few tiles: scale_kernel, then
    split-K atomics) with beta = 0.5 on a random C and beta = 0 on a NaN-filled one; ldc > N stays untouched."""
    L, lib, dev = _api()
    c = case
    d = {k: v.to(dev) for k, v in R.gemm_inputs(c).items()}
    Cbuf = d["C0"].clone()
    with torch.cuda.device(dev):
        L.check(lib.gn_gemm_f32(L.addr(d["A"]), L.addr(d["B"]), L.addr(Cbuf), c.M, c.N, c.K, c.lda, c.ldb, c.ldc_,
                                int(c.tA), int(c.tB), None, None, 0, 0, c.alpha, c.beta, L.stream_handle()), "gn_gemm_f32")
    torch.cuda.synchronize()
    bad = []
    _gemm_verdict(bad, c, Cbuf, None, single=True)
    assert not bad, bad
