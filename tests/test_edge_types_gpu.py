"""The edge head and the typed aggregation at every edge-type count K, against float64.

The reference runs K = 6 (pairwise) and K = 10 (hyper), and so did every comparison with a reference in this suite; the
kernels take 1..15 (edge head) and 1..16 (aggregation) and branch on K (tests/edge_type_cases.py lists where).  Four
parts, each against the float64 oracle on inputs drawn on the CPU (tests/test_edge_types_cpu.py holds the fp32 oracle on
the same inputs within a third of every gate):

  1. every edge kernel at K = 1..15, rows ragged against the 32-row block and the pairwise unordered form;
  2. one typed-aggregation launch per source form, launch size and matrix path at K = 1..16, the launcher's plan of that
     very launch (waves per row block, node form, kernel) held against the rules;
  3. whole modules built by `with_edge_types` through `run_message_passing`: the latency form on both sides of the K
     at which the aggregation launch takes the closing stage, the pair form beyond the node form's K = 12, the group order
     by cost in K, the stand-alone gather / scatter, bf16 storage in the scene form, two rounds;
  4. training: every gradient against float64 autograd of the oracle, parameters whose gradient is identically zero
     (the whole distribution head at K = 1) included.

Gates: those the suite applies at K = 6 / 10 — TOL_FEAT of max|ref| and TOL_FAC absolute on fp32 results, TOL_ORACLE on
bf16 storage, TOL_CLEAN / TOL_ANY on gradients.  Every test prints its measured errors.
"""
import pytest
import torch

from device_noise_cases import KERNELS, select_kernel
from edge_type_cases import (EDGE_SHAPES, K_AGG, K_AGG_EDGES, K_ALL, LATENCY_CASES, N17_CASES, NMP2_CASES, NODE_FORM_MAX_K,
                             ORDER_CASE, ORDER_POS, PAIR_FORM_CASES, SCENE_CASES, BACKWARD_K, BACKWARD_KINDS, BACKWARD_SIZES, abs_err,
                             agg_cases, agg_inputs, backward_case, backward_reference, live_parameters,
                             agg_launch_forms, agg_module, agg_ref, edge_head, edge_inputs, edge_ref, engine_case, engine_forms,
                             engine_ref, rel_err, state_of)
from relu_probe import WINDOW
from test_backward_gpu import TOL_ANY, TOL_CLEAN, _check
from test_bf16_gpu import TOL_ORACLE
from test_device_noise_gpu import _assert_kernel, _spy_edge_plans
from test_launch_forms_gpu import TOL_FAC, TOL_FEAT, _spy_plans
from test_route_gpu import carried, check_follows, engine_route, record

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _name(kernel):
    from groupnet_amd import _lib
    return (_lib.load().gn_kernel_name(kernel) or b"").decode()


def _set_precision(mode, monkeypatch):
    from groupnet_amd import ops
    monkeypatch.setattr(ops, "BF16X6", ops.BF16X6)      # (restored after the test)
    monkeypatch.setattr(ops, "F16X3", ops.F16X3)
    ops.set_precision(mode)


# ---- 1. the edge head ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", K_ALL)
@pytest.mark.parametrize("kernel", KERNELS, ids=[k.id for k in KERNELS])
def test_edge_head_matches_float64(kernel, K, monkeypatch):
    """factor * dist and dist of every edge kernel against O.edge_mlp_gumbel in float64: 69 rows (two full row blocks and
    a ragged one) and the unordered pairs of N = 5 with the ordered dist, one launch each.  K = 1: dist is exactly 1."""
    from groupnet_amd import ops
    dtype = select_kernel(kernel, monkeypatch)
    twin = dtype == torch.bfloat16
    plans = []
    _spy_edge_plans(monkeypatch, plans)
    mod = edge_head(K)
    st = state_of(mod, "head")
    pk = mod.to(dev())._packed()
    gate = TOL_ORACLE if twin else TOL_FAC
    errs = []
    for shape in EDGE_SHAPES:
        tag, B, E, sym_N = shape
        edges, U = edge_inputs(K, shape, bf16=twin)
        (ef, dist), = ops.edge_mlp_gumbel_grouped([(edges.to(dev()).to(dtype), U.to(dev()), pk, K, sym_N, True)])
        with torch.no_grad():
            ref_ef, ref_dist = edge_ref(st, edges, U, sym_N)
        assert ef.dtype == torch.float32 and dist.dtype == dtype
        errs.append((tag, abs_err(ef, ref_ef), abs_err(dist, ref_dist)))
        if K == 1:
            assert bool((dist == 1).all()), "a one-type softmax is exactly 1"
    print(f"\nedge head {kernel.name} K={K}: " + ", ".join(f"{t} factor*dist {a:.2e} dist {b:.2e}" for t, a, b in errs)
          + f" (gate {gate:g})", end="")
    _assert_kernel(plans, kernel, len(EDGE_SHAPES))
    assert max(max(a, b) for _, a, b in errs) <= gate, (kernel.id, K, errs)


# ---- 2. the typed aggregation stage --------------------------------------------------------------------------------------
AGG_MODES = ([("f16x3", "fp32", K) for K in K_AGG]
             + [(p, d, K) for p, d in (("bf16x6", "fp32"), ("fp32", "fp32"), ("f16x3", "bf16")) for K in K_AGG_EDGES])


def _agg_source(case, inp, K, pk, dtype):
    from groupnet_amd import ops
    form = case[0]
    t = lambda x: x.to(dev()).to(dtype)
    if form == "eo":
        return t(inp["eo"])
    if form == "gather":
        return ops.GatherSpec(t(inp["ori"]), inp["H"].to(dev()))
    if form in ("twin-pair", "scene"):
        return ops.GatherSpec(t(inp["ori"]), None, True, node=form == "scene")
    A = ops.node_linear(t(inp["ori"]), pk["W1cat"], pk["b1half"], K * 128)
    return ops.PairSpec(A, node=form == "pair-node")


@pytest.mark.parametrize("precision,dtype,K", AGG_MODES, ids=[f"{p if d == 'fp32' else d}-K{K}" for p, d, K in AGG_MODES])
def test_typed_aggregation_matches_float64(precision, dtype, K, monkeypatch):
    """One ops.agg_mlp_grouped launch per source form and launch size against O.aggregate_typed_mlp in float64 (the node
    and scene forms: H^T of it over the pairwise incidence), and the plan of that launch against the rules: waves per
    row block by K and launch size, node form, kernel.  The node form beyond K = 12 is refused."""
    from groupnet_amd import ops
    _set_precision(precision, monkeypatch)
    twin = dtype == "bf16"
    tdt = torch.bfloat16 if twin else torch.float32
    plans = []
    _spy_plans(monkeypatch, plans)
    mod = agg_module(K)
    st = state_of(mod, "agg")
    pk = mod.to(dev())._packed()
    gate = TOL_ORACLE if twin else TOL_FEAT
    lines, worst = [], 0.0
    for case in agg_cases(precision, dtype):
        inp = agg_inputs(K, case, bf16=twin)
        ef = inp["ef"].to(dev())
        if case[0] == "pair-node" and K > NODE_FORM_MAX_K:
            with pytest.raises(ValueError):
                ops.agg_mlp_grouped([(_agg_source(case, inp, K, pk, tdt), ef, pk, K)])
            continue
        with torch.no_grad():
            ref = agg_ref(st, case, inp)
        for rb2 in (("0", "1") if twin else (None,)):
            if rb2 is None:
                monkeypatch.delenv("GN_AGG_RB2", raising=False)
            else:
                monkeypatch.setenv("GN_AGG_RB2", rb2)
            n0 = len(plans)
            (got,) = ops.agg_mlp_grouped([(_agg_source(case, inp, K, pk, tdt), ef, pk, K)])
            assert got.dtype == tdt and got.shape == ref.shape
            (stem, rc, plan), = plans[n0:]
            want = agg_launch_forms(case, K, precision, dtype, rb2)
            assert rc == 0 and plan.n_groups == 1, (case, rc)
            assert (plan.wpr[0], bool(plan.node_form[0])) == (want["wpr"], want["node_form"]), (case, K, plan.wpr[0])
            if want["scene_grid"] is not None:
                assert (_name(plan.pre_kernel[0]), plan.pre_grid[0]) == ("agg_scene_kernel", want["scene_grid"]), case
            else:
                assert _name(plan.kernel) == want["kernel"] and plan.pre_grid[0] == 0, (case, _name(plan.kernel))
            err = rel_err(got, ref)
            worst = max(worst, err)
            lines.append(f"{case[0]} B{case[1]} {'E' if case[0] == 'eo' else 'N'}{case[3] if case[0] == 'eo' else case[2]}"
                         f"{'' if rb2 is None else ' rb2=' + rb2} wpr{want['wpr']}: {err:.2e}")
            assert err <= gate, (precision, dtype, K, case, rb2, err)
    print(f"\ntyped aggregation {precision if not twin else 'bf16'} K={K} (gate {gate:g}, worst {worst:.2e}): " + "; ".join(lines),
          end="")


def test_node_form_beyond_twelve_types_is_refused():
    from groupnet_amd import ops
    K = 13
    mod = agg_module(K).to(dev())
    pk = mod._packed()
    ori = torch.randn(2, 5, 64, device=dev())
    A = ops.node_linear(ori, pk["W1cat"], pk["b1half"], K * 128)
    ef = torch.rand(2, 15, K, device=dev())
    with pytest.raises(ValueError):
        ops.agg_mlp_grouped([(ops.PairSpec(A, node=True), ef, pk, K)])
    (feat,) = ops.agg_mlp_grouped([(ops.PairSpec(A), ef, pk, K)])       # the pair form takes it
    assert feat.shape == (2, 15, 64) and bool(torch.isfinite(feat).all())


# ---- 3. whole modules through the engine ---------------------------------------------------------------------------------
def _run(case, monkeypatch, fuse_closing=True, spy=True):
    """One forward of the case through run_message_passing -> (results on the sampled scenes, float64 references,
    recorded calls, plans of the aggregation launches, the modules)."""
    from groupnet_amd.MS_HGNN_batch import run_message_passing
    _set_precision("f16x3", monkeypatch)
    mods, states, h, Hs, U, scenes = engine_case(case)
    tdt = torch.bfloat16 if case["dtype"] == "bf16" else torch.float32
    for m in mods:
        m.to(dev()).eval()
    hd = h.to(dev()).to(tdt)
    Hd = [None if H is None else H.to(dev()) for H in Hs]
    Ud = [[u.to(dev()) for u in per] for per in U]
    plans = []
    _spy_plans(monkeypatch, plans)
    calls = record(monkeypatch)

    def forward(fuse):
        with torch.no_grad():
            res = run_message_passing(mods, [hd] * len(mods), Hd, Ud, [None] * len(mods), fuse_closing=fuse)
        torch.cuda.synchronize()
        return res
    res = forward(fuse_closing)
    kept = list(calls), [p for s, rc, p in plans if s == "gn_agg_mlp"]
    assert all(rc == 0 for _, rc, _ in plans)
    with torch.no_grad():
        ref = engine_ref(states, h, Hs, U, scenes, case["nmp"])
    return dict(res=res, ref=ref, calls=kept[0], agg_plans=kept[1], mods=mods, scenes=scenes, forward=forward)


def _compare(case, res, ref, scenes, what=""):
    twin = case["dtype"] == "bf16"
    sel = scenes.to(dev())
    fe = [rel_err(r[0][sel], w[0]) for r, w in zip(res, ref)]
    ce = [abs_err(r[1][sel], w[1]) for r, w in zip(res, ref)]
    print(f"\nengine {case['id']}{what}: {len(scenes)} scenes, features {['%.2e' % e for e in fe]} of max|ref| "
          f"(gate {TOL_ORACLE if twin else TOL_FEAT:g}), factors {['%.2e' % e for e in ce]} (gate {TOL_ORACLE if twin else TOL_FAC:g})",
          end="")
    assert max(fe) <= (TOL_ORACLE if twin else TOL_FEAT), (case["id"], fe)
    assert max(ce) <= (TOL_ORACLE if twin else TOL_FAC), (case["id"], ce)
    for (nf, fac), K in zip(res, case["types"]):
        assert fac.shape[-1] == K and (K > 1 or bool((fac == 1).all()))


def _follows(case, run, fused):
    tdt = torch.bfloat16 if case["dtype"] == "bf16" else torch.float32
    N = case["N"]
    rt = engine_route(N, [(s is None, K) for s, K in zip(case["scales"], case["types"])], tdt, False, closing_asked=True)
    names = ["pair" if s is None else (1 if s == N else N) for s in case["scales"]]
    check_follows(run["calls"], rt, names, N, nmp=case["nmp"], fused=fused)
    return rt


@pytest.mark.parametrize("case", LATENCY_CASES, ids=[c["id"] for c in LATENCY_CASES])
def test_latency_form_takes_or_declines_the_closing_stage(case, monkeypatch):
    """fuse_closing=True at N = 11: `ops.agg_mlp_closing` accepts exactly when the rules say so for these K (a hyper group
    at one wave per row block — K < 4 below 128 row blocks, K = 1 from there on — declines); where it declines the forward
    completes through the separate closing launch, bit-identical with the forward that never asked."""
    forms = engine_forms(case)
    run = _run(case, monkeypatch)
    taken = [c[3] is not None for c in run["calls"] if c[0] == "agg_mlp_closing"]
    assert taken == [forms["fused_closing"]], (case["id"], taken)
    rt = _follows(case, run, forms["fused_closing"])
    assert rt.ask_closing and [m.node_form for m in rt.modules] == [g["node_form"] for g in forms["groups"]]
    names = [c[0] for c in run["calls"]]
    assert ("mlp2_grouped" in names) == (not forms["fused_closing"]) and names.count("agg_mlp_grouped") == int(not forms["fused_closing"])
    (plan,) = run["agg_plans"]
    assert plan.closing == int(forms["fused_closing"])
    for i, g in enumerate(forms["groups"]):
        assert (plan.wpr[i], plan.spw[i], bool(plan.node_form[i])) == (g["wpr"], g["spw"], g["node_form"]), (case["id"], g)
    assert [plan.pos[i] for i in range(len(forms["groups"]))] == forms["agg_pos"]
    _compare(case, run["res"], run["ref"], run["scenes"], " closing " + ("fused" if forms["fused_closing"] else "declined"))
    plain = run["forward"](False)
    same = all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(run["res"], plain))
    if not forms["fused_closing"]:
        assert same, "a declined closing stage must leave the forward that never asked"
    else:
        _compare(case, plain, run["ref"], run["scenes"], " closing not asked")


@pytest.mark.parametrize("case", PAIR_FORM_CASES, ids=[c["id"] for c in PAIR_FORM_CASES])
def test_pairwise_module_beyond_the_node_form_takes_the_pair_form(case, monkeypatch):
    from groupnet_amd import ops, route as R
    run = _run(case, monkeypatch)
    rt = _follows(case, run, False)
    pair = rt.modules[0]
    assert (pair.source, pair.first_layer, pair.node_form, pair.closing_input) == (R.PAIR, True, False, R.SCATTER_SPEC)
    agg = [carried(c, case["N"]) for c in run["calls"] if c[0] == "agg_mlp_grouped"]
    mlp2 = [carried(c, case["N"]) for c in run["calls"] if c[0] == "mlp2_grouped"]
    assert agg == [("agg_mlp_grouped", [(ops.PairSpec, False), (ops.GatherSpec, False)])]
    assert mlp2 == [("mlp2_grouped", [ops.ScatterSpec, ops.ScatterSpec])]
    _compare(case, run["res"], run["ref"], run["scenes"])


def test_group_order_follows_the_cost_in_edge_types(monkeypatch):
    """[pair K = 6 (node form), hyper K = 1, hyper K = 15, hyper K = 4] in one aggregation launch: the longest waves first."""
    run = _run(ORDER_CASE, monkeypatch)
    (plan,) = run["agg_plans"]
    assert [plan.pos[i] for i in range(4)] == ORDER_POS == engine_forms(ORDER_CASE)["agg_pos"]
    assert [plan.wpr[i] for i in range(4)] == [1, 1, 4, 4] and plan.closing == 0
    _follows(ORDER_CASE, run, False)
    _compare(ORDER_CASE, run["res"], run["ref"], run["scenes"])


@pytest.mark.parametrize("case", N17_CASES + SCENE_CASES + NMP2_CASES, ids=[c["id"] for c in N17_CASES + SCENE_CASES + NMP2_CASES])
def test_modules_at_other_edge_type_counts_match_float64(case, monkeypatch):
    """N = 17: stand-alone gather and scatter; N = 33 on bf16 storage: the scene form; two rounds at N = 11."""
    from groupnet_amd import route as R
    forms = engine_forms(case)
    run = _run(case, monkeypatch)
    rt = _follows(case, run, forms["fused_closing"] if case["N"] <= 16 else None)
    if case["N"] == 17:
        assert (rt.gather, rt.scatter) == ((1, 2), (0, 1, 2)) and rt.modules[0].source == R.PAIR
    elif case["dtype"] == "bf16":
        assert rt.modules[0].source == R.SCENE and rt.scatter == (1,)
    else:
        assert len(run["agg_plans"]) == 2 and case["nmp"] == 2
    _compare(case, run["res"], run["ref"], run["scenes"])


# ---- 4. backward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N", BACKWARD_SIZES)
@pytest.mark.parametrize("K", BACKWARD_K)
@pytest.mark.parametrize("kind", BACKWARD_KINDS)
def test_gradients_match_float64_autograd(kind, K, B, N):
    """L = <node_feat, R1> + <factors, R2>: dL/dh and every parameter gradient of the HIP training path against float64
    autograd of the oracle — the whole batch within TOL_ANY, its clean scenes alone (relu_probe) within TOL_CLEAN, as
    tests/test_backward_gpu.py (the inputs: `backward_case`, chosen on the oracle alone so that at least one scene is
    clean).  A parameter whose float64 gradient is identically zero (never touched, or — K = 1 — the whole distribution
    head: a one-type softmax is constant) gets None or exact zeros.  K = 5 and 13 are padded to 8 and 16 rows in the
    backward: a pad row that leaked would show in the K-row gradients of the heads."""
    c = backward_case(kind, K, B, N)
    mod, h, U, R1, R2 = c["mod"], c["h"], c["U"], c["R1"], c["R2"]
    mod.to(dev()).train()
    tag = f"{kind} K={K} B={B} N={N} (draw {c['shift']})"

    def both(rows, tol):
        r = backward_reference(kind, c, rows)
        for p in mod.parameters():
            p.grad = None
        x = h[rows].clone().to(dev()).requires_grad_(True)
        if kind == "pair":
            nf2, fac2 = mod(x, noise_u=[U[rows].to(dev())])
        else:
            nf2, fac2, _ = mod(x, None, noise_u=[U[rows].to(dev())], H=r["H"].to(dev()))
        assert abs_err(nf2, r["nf"]) <= 1e-5 and abs_err(fac2, r["fac"]) <= 1e-5
        ((nf2 * R1[rows].to(dev())).sum() + (fac2 * R2[rows].to(dev())).sum()).backward()
        eh = rel_err(x.grad, r["dh"])
        assert eh <= tol, (tag, "dL/dh", eh, tol)
        ref = r["grads"]
        hip = {k: p.grad for k, p in mod.named_parameters()}
        used = [k for k in ref if k not in r["dead"]]
        assert len(used) == live_parameters(kind, K), (tag, len(used))
        ew, where = _check(hip, ref, used, tol)
        for k in r["dead"]:
            assert hip[k] is None or not bool(hip[k].any()), (tag, k, "gradient of a parameter the loss does not depend on")
        return r["probe"], eh, ew, where, ref, hip

    rows_all = torch.arange(B)
    probe, eh, ew, where, ref, hip = both(rows_all, TOL_ANY)
    if K == 1:
        dead = [k for k in ref if "MLP_distribution" in k]
        assert len(dead) == 4 and all(not bool(ref[k].any()) for k in dead)
        assert all(hip[k] is None or not bool(hip[k].any()) for k in dead)
    for k in hip:
        if "MLP_distribution.layers.1" in k:
            assert hip[k] is None or hip[k].shape[0] == K
    clean = probe.clean()
    assert bool(clean.any()), tag
    msg = (f"\nbackward {tag}: whole batch dL/dh {eh:.1e}, worst parameter {ew:.1e} ({where}), gate {TOL_ANY:g}; "
           f"{int(clean.sum())}/{B} scenes clean (window {WINDOW:g})")
    if bool(clean.all()):
        print(msg + f"; all clean: gated at {TOL_CLEAN:g}", end="")
        assert eh <= TOL_CLEAN and ew <= TOL_CLEAN, (tag, eh, ew, where)
        return
    _, eh2, ew2, where2, _, _ = both(rows_all[clean], TOL_CLEAN)
    print(msg + f"; clean scenes alone dL/dh {eh2:.1e}, worst parameter {ew2:.1e} ({where2}), gate {TOL_CLEAN:g}", end="")
