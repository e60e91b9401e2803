"""CPU checks of tests/backward_kernel_refs.py: the references equal autograd through the golden-pinned oracle, the
inputs of every GPU case meet the conditions the gate rests on, the case tables reach every launcher form, and every
named flaw moves some output of some case by more than 10 gates."""
import pytest
import torch

import backward_kernel_refs as R
from oracle import ms_hgnn_oracle as O
from test_backward_gpu import TOL_CLEAN

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ---- the references are the oracle's -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [R.N2E_CASES[0], R.N2E_GROUPED[0]], ids=lambda c: c.name)
def test_pooling_reference_equals_oracle_autograd(case):
    """oracle node2edge(decomposed=True) with an identity start layer (x' = x): its gradients w.r.t. x, the attention
    layer 0 (W1, b1) and layer 1 (w2, b2) against the helper's dxp / dpq / dw2 / db2 chained through pq = [P | Qn]."""
    g = torch.Generator().manual_seed(7)
    inp = R.n2e_inputs(case)
    H, x, dedges = inp["H"].double(), inp["xp"].double(), inp["dedges"].double()
    W1 = torch.randn(32, 128, generator=g, dtype=F64)
    b1 = torch.randn(32, generator=g, dtype=F64)
    state = {"node2edge_start_mlp.0.layers.0.weight": torch.eye(64, dtype=F64),
             "node2edge_start_mlp.0.layers.0.bias": torch.zeros(64, dtype=F64),
             "attention_mlp.0.layers.0.weight": W1, "attention_mlp.0.layers.0.bias": b1,
             "attention_mlp.0.layers.1.weight": inp["w2"].double()[None],
             "attention_mlp.0.layers.1.bias": inp["b2"].double()}
    leaves = [x, W1, b1, state["attention_mlp.0.layers.1.weight"], state["attention_mlp.0.layers.1.bias"]]
    for t in leaves:
        t.requires_grad_(True)
    edges, _ = O.node2edge(state, x, H, decomposed=True)
    gx, gW1, gb1, gw2, gb2 = torch.autograd.grad((edges * dedges).sum(), leaves)
    pq = torch.cat((x.detach() @ W1.detach()[:, :64].t() + b1.detach(), x.detach() @ W1.detach()[:, 64:].t()), dim=-1)
    zero = {k: torch.zeros_like(inp[k]) for k in ("dxp0", "dpq0", "dw20", "db20")}
    r = R.n2e_grads({**inp, **zero, "pq": pq}, F64)
    dP, dQn, xd = r["dpq"][..., :32], r["dpq"][..., 32:], x.detach()
    assert _rel(r["dxp"] + dP @ W1.detach()[:, :64] + dQn @ W1.detach()[:, 64:], gx) <= 1e-12
    assert _rel(torch.cat((torch.einsum("bnc,bnd->cd", dP, xd), torch.einsum("bnc,bnd->cd", dQn, xd)), dim=1), gW1) <= 1e-12
    assert _rel(dP.sum(dim=(0, 1)), gb1) <= 1e-12
    assert _rel(r["dw2"], gw2[0]) <= 1e-12 and _rel(r["db2"], gb2) <= 1e-12


@pytest.mark.parametrize("K,rows", [(6, 9), (10, 14)])
def test_gumbel_reference_equals_oracle_autograd(K, rows):
    g = torch.Generator().manual_seed(K)
    D = 16
    Rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    z, Wd, bd, Wf, bf = Rn(1, rows, D), Rn(K, D), Rn(K), Rn(1, D), Rn(1)
    U = torch.rand(1, rows, K, generator=g, dtype=F64)
    de, gd = Rn(1, rows, K), Rn(1, rows, K)
    state = {"m.init_MLP.layers.0.weight": torch.eye(D, dtype=F64), "m.init_MLP.layers.0.bias": torch.zeros(D, dtype=F64),
             "m.MLP_distribution.layers.0.weight": Wd, "m.MLP_distribution.layers.0.bias": bd,
             "m.MLP_factor.layers.0.weight": Wf, "m.MLP_factor.layers.0.bias": bf}
    leaves = [z, Wd, bd, Wf, bf]
    for t in leaves:
        t.requires_grad_(True)
    ef, dist = O.edge_mlp_gumbel(state, "m", z, U)
    gz, gWd, gbd, gWf, gbf = torch.autograd.grad((ef * de).sum() + (dist * gd).sum(), leaves)
    zd = z.detach()[0]
    inp = dict(logits=zd @ Wd.detach().t() + bd.detach(), f=(zd @ Wf.detach().t() + bf.detach())[:, 0],
               g=-torch.log(O.GUMBEL_EPS - torch.log(U[0] + O.GUMBEL_EPS)), tau=O.GUMBEL_TAU, sym_N=0, diag_w=1.0,
               gdist=gd[0], **{"def": de[0]})
    r = R.gumbel_grads(inp, F64)
    dl, df = r["dlgf"][:, :K], r["dlgf"][:, K:]
    assert _rel(r["ef"], ef.detach()[0]) <= 1e-12 and _rel(r["dist"], dist.detach()[0]) <= 1e-12
    assert _rel(dl.t() @ zd, gWd) <= 1e-12 and _rel(dl.sum(0), gbd) <= 1e-12
    assert _rel(df.t() @ zd, gWf) <= 1e-12 and _rel(df.sum(0), gbf) <= 1e-12
    assert _rel(dl @ Wd.detach() + df @ Wf.detach(), gz[0]) <= 1e-12


def test_gumbel_pair_rows_are_the_sum_of_their_ordered_rows():
    """sym_N: the pair-row reference equals the ordered-row reference fed the replicated logits, summed per pair."""
    case = R.GUMBEL_CASES[4]
    inp = {k: (v.double() if torch.is_tensor(v) else v) for k, v in R.gumbel_inputs(case).items()}
    N, P = case.sym_N, R.pair_count(case.sym_N)
    e0, e1 = R.sym_edge_rows(case.rows // P, N)
    row_of = torch.empty(inp["g"].shape[0], dtype=torch.long)
    row_of[e0] = torch.arange(case.rows)
    row_of[e1[e1 >= 0]] = torch.arange(case.rows)[e1 >= 0]
    flat = dict(inp, logits=inp["logits"][row_of], f=inp["f"][row_of], sym_N=0, **{"def": inp["def"][row_of]})
    a, b = R.gumbel_grads(inp, F64), R.gumbel_grads(flat, F64)
    summed = torch.zeros_like(a["dlgf"]).index_add_(0, row_of, b["dlgf"])
    assert _rel(a["dist"], b["dist"]) <= 1e-12 and _rel(a["dlgf"], summed) <= 1e-12


@pytest.mark.parametrize("case", R.TYPED_CASES[:2])
def test_typed_reference_equals_oracle_autograd(case):
    rows, K, hid, _ = case
    g = torch.Generator().manual_seed(rows)
    inp = {k: v.double() for k, v in R.typed_inputs(case).items()}
    eo = torch.randn(1, rows, 64, generator=g, dtype=F64)
    W1 = torch.randn(K, hid, 64, generator=g, dtype=F64)
    b1 = torch.randn(K, hid, generator=g, dtype=F64)
    state = {}
    for k in range(K):
        state[f"a.agg_mlp.{k}.layers.0.weight"], state[f"a.agg_mlp.{k}.layers.0.bias"] = W1[k], b1[k]
        state[f"a.agg_mlp.{k}.layers.1.weight"], state[f"a.agg_mlp.{k}.layers.1.bias"] = inp["W2"][k], inp["b2"][k]
    ef = inp["ef"][None].clone().requires_grad_(True)
    b1s = [state[f"a.agg_mlp.{k}.layers.0.bias"].requires_grad_(True) for k in range(K)]
    feat = O.aggregate_typed_mlp(state, "a", ef, eo)
    got = torch.autograd.grad((feat[0] * inp["dfeat"]).sum(), [ef] + b1s)
    pre = torch.einsum("rd,khd->rkh", eo[0], W1) + b1.detach()
    r = R.typed_grads(dict(inp, pre=pre), F64)
    assert _rel(r["def"], got[0][0]) <= 1e-12
    assert _rel(r["T"].sum(0), torch.stack(got[1:])) <= 1e-12


# ---- conditions on the inputs of every GPU case -------------------------------------------------------------------
def _within_ceiling(tag, r64, r32, scale, ceiling=TOL_CLEAN):
    bound, e32 = R.gate(r64, r32, scale)
    assert bound <= ceiling * scale, (tag, e32, scale, ceiling)
    return bound


@pytest.mark.parametrize("case", R.N2E_CASES + R.N2E_GROUPED, ids=lambda c: c.name)
def test_pooling_inputs(case):
    r64, r32 = R.n2e_expected(case)
    assert torch.equal(r64["relu"], r32["relu"])
    pre = r64["pre"]
    assert torch.equal(pre.float().double(), pre) and torch.equal(r32["pre"].double(), pre)
    nz = pre[pre != 0].abs()
    assert nz.numel() == 0 or float(nz.min()) >= 1 / 128
    for out in R.N2E_OUTPUTS:
        _within_ceiling((case.name, out), r64[out], r32[out], R.n2e_scale(r64, out))


def test_pooling_table_exercises_the_convention_at_zero():
    zeros = sum(int((R.n2e_expected(c)[0]["pre"] == 0).sum()) for c in R.N2E_CASES)
    assert zeros >= 15


@pytest.mark.parametrize("case", R.GUMBEL_CASES + R.GUMBEL_STRIDE_CASES, ids=lambda c: c.name)
def test_gumbel_inputs(case):
    for with_gdist in ((True, False) if case in R.GUMBEL_CASES else (True,)):
        r64, r32 = R.gumbel_expected(case, with_gdist)
        assert bool(torch.isfinite(r64["dlgf"]).all())
        for out in ("ef", "dlgf"):
            _within_ceiling((case.name, out), r64[out], r32[out], float(r64[out].abs().max()))
    if case.saturated:       # df -> 0 on the saturated rows
        assert float(r64["dlgf"][:4, case.K].abs().max()) <= 1e-10 * float(r64["dlgf"].abs().max())
    if case.logit_scale > 1:
        assert float(r64["dist"].min()) < 1e-19


@pytest.mark.parametrize("case", R.TYPED_CASES, ids=str)
def test_typed_inputs(case):
    r64, r32 = R.typed_expected(case)
    inp = R.typed_inputs(case)
    assert bool((inp["Hc"] == 0).any()) and torch.equal(inp["Hc"] > 0, inp["pre"] > 0)
    for out in ("def", "T"):
        _within_ceiling((case, out), r64[out], r32[out], float(r64[out].abs().max()))


@pytest.mark.parametrize("case", R.GEMM_BATCH + R.GEMM_ACCUM + R.GEMM_SINGLE, ids=lambda c: c.name)
def test_gemm_inputs(case):
    (c64, cs64, cs_scale), (c32, cs32, _) = R.gemm_expected(case)
    ceiling = R.gemm_ceiling(case, single=case in R.GEMM_SINGLE)
    inside = torch.isfinite(c64)
    _within_ceiling(case.name, c64[inside], c32[inside], R.c_scale(case, c64), ceiling)
    if case.colsum:
        _within_ceiling((case.name, "colsum"), cs64, cs32, cs_scale, ceiling)


def test_probe_products_are_exact():
    """Every output of a probe is one product by a power of two: float64 and fp32 evaluations agree to the bit."""
    for case in R.GEMM_PROBES:
        (c64, _, _), (c32, _, _) = R.gemm_expected(case)
        assert torch.equal(c64, c32.double()) and int((c64 != 0).sum()) == case.M * case.N
        assert R.gemm_vec(case) and R.gemm_splits(case.M, case.N, case.K, case.accum) == 1


# ---- the tables reach every form ------------------------------------------------------------------------------------
def test_case_tables_reach_every_form():
    forms = {R.n2e_form(c.N, c.kind == "hyper") for c in R.N2E_CASES}
    assert forms == {"scene", "scene_big_lds", "wave"}
    by_n = {c.N: R.n2e_form(c.N, True) for c in R.N2E_CASES}
    assert (by_n[60], by_n[61], by_n[140], by_n[141]) == ("scene", "scene_big_lds", "scene_big_lds", "wave")
    assert any(c.B * c.E % 4 for c in R.N2E_CASES if R.n2e_form(c.N, True) == "wave")      # a dead tail wave
    assert all(R.n2e_form(c.N, c.kind == "hyper") != "wave" for c in R.N2E_GROUPED)
    # GEMM staging, from the launcher's `vec` rule, in one batch with more than a table's worth of each
    staging = [R.gemm_vec(c) for c in R.GEMM_BATCH]
    assert staging.count(True) >= 17 and staging.count(False) >= 17
    assert {(c.tA, c.tB) for c in R.GEMM_BATCH if R.gemm_vec(c) and c.name.startswith("vec")} == \
        {(a, b) for a in (False, True) for b in (False, True)}
    mis = [c for c in R.GEMM_BATCH if c.offA % 4]
    assert mis and all(R.gemm_vec(R.GemmCase(**{**c.__dict__, "offA": 0})) and not R.gemm_vec(c) for c in mis)
    # split-K: none, two uneven chunks on either staging, many
    splits = {(R.gemm_vec(c), R.gemm_splits(c.M, c.N, c.K, c.accum)) for c in R.GEMM_ACCUM}
    assert {(True, 1), (True, 2), (False, 2)} <= splits and max(s for _, s in splits) >= 33
    assert {R.gemm_vec(c) for c in R.GEMM_ACCUM if c.tC} == {True, False}
    # gn_gemm_f32's own split rule
    assert {R.gemm_f32_accum(c.M, c.N, c.K, True) for c in R.GEMM_SINGLE} == {True, False}
    # grid-stride loops
    gum = {R.grid_stride(c.rows, 256) for c in R.GUMBEL_CASES + R.GUMBEL_STRIDE_CASES}
    ef = {R.grid_stride(c.rows * c.K, 256) for c in R.GUMBEL_CASES + R.GUMBEL_STRIDE_CASES}
    typed = {R.grid_stride(rows, 4, 8192) for rows, _, _, _ in R.TYPED_CASES}
    ax = {R.grid_stride(rows * cols, 256) for rows, cols, _ in R.AXPBY_CASES}
    assert gum == ef == typed == ax == {True, False}
    assert {c.sym_N > 0 for c in R.GUMBEL_STRIDE_CASES} == {True, False}


# ---- sensitivity: every named flaw is told apart ------------------------------------------------------------------
def _gates_moved(flawed, r64, r32, scale):
    bound, _ = R.gate(r64, r32, scale)
    return float((flawed - r64).abs().max()) / bound


@pytest.mark.parametrize("flaw", R.N2E_FLAWS)
def test_pooling_flaws_are_detected(flaw):
    worst = 0.0
    for case in R.N2E_CASES[:7]:
        if flaw == "selfloop_weight_1":
            if case.kind == "hyper":
                continue
            bad = R.n2e_grads(R.n2e_inputs(case, 1.0), F64)
        else:
            bad = R.n2e_grads(R.n2e_inputs(case), F64, flaw)
        r64, r32 = R.n2e_expected(case)
        worst = max([worst] + [_gates_moved(bad[o], r64[o], r32[o], R.n2e_scale(r64, o)) for o in R.N2E_OUTPUTS])
    assert worst > 10, (flaw, worst)


def test_two_pooling_flaws_need_partial_membership_and_non_unit_weights():
    """Dropping the non-members is invisible under full membership, H-once under 0/1 weights: why case a has both."""
    full, pairwise = R.N2E_CASES[1], R.N2E_CASES[5]
    assert _rel(R.n2e_grads(R.n2e_inputs(full), F64, "nonmembers_dropped")["dxp"], R.n2e_expected(full)[0]["dxp"]) <= 1e-12
    ones = dict(R.n2e_inputs(pairwise))
    ones["H"] = (ones["H"] != 0).float()
    assert _rel(R.n2e_grads(ones, F64, "h_once")["dxp"], R.n2e_grads(ones, F64)["dxp"]) <= 1e-12


@pytest.mark.parametrize("flaw", R.GUMBEL_FLAWS)
def test_gumbel_flaws_are_detected(flaw):
    worst = 0.0
    for case in R.GUMBEL_CASES:
        r64, r32 = R.gumbel_expected(case)
        bad = R.gumbel_grads(R.gumbel_inputs(case), F64, flaw)
        worst = max(worst, _gates_moved(bad["dlgf"], r64["dlgf"], r32["dlgf"], float(r64["dlgf"].abs().max())))
    assert worst > 10, (flaw, worst)


@pytest.mark.parametrize("flaw", R.TYPED_FLAWS)
def test_typed_flaws_are_detected(flaw):
    worst = 0.0
    for case in R.TYPED_CASES[:3]:
        r64, r32 = R.typed_expected(case)
        bad = R.typed_grads(R.typed_inputs(case), F64, flaw)
        worst = max([worst] + [_gates_moved(bad[o], r64[o], r32[o], float(r64[o].abs().max())) for o in ("def", "T")])
    assert worst > 10, (flaw, worst)


def test_a_two_part_split_would_miss_the_probe_gate():
    """A product formed from two bf16 parts of one operand is off by about 2^-17 of itself — far outside 2^-23."""
    case = R.GEMM_PROBES[0]
    d = R.gemm_inputs(case)
    A = R.view2d(d["A"], *case.a_shape, case.lda, case.offA)
    p1 = A.bfloat16().float()
    two = p1 + (A - p1).bfloat16().float()
    rel = ((two - A).abs() / A.abs()).max()
    assert float(rel) > 32 * R.PROBE_REL
