"""The edge-type count K on the host (no GPU): the launchers' plans at every K against tests/launch_forms.py, the
launchers' and the modules' refusals outside the supported range, the route's K branch points, and the float64
references of tests/test_edge_types_gpu.py against the fp32 oracle on the same inputs."""
import ctypes
import itertools

import pytest
import torch

from edge_type_cases import (AGG_CASES_FP32, EDGE_SHAPES, K_AGG, K_ALL, K_EDGES, abs_err, agg_inputs, agg_launch_forms,
                             agg_module, agg_ref, agg_rows, edge_head, edge_inputs, edge_ref, engine_case, engine_forms,
                             engine_ref, rel_err, state_of, with_edge_types, ENGINE_CASES, LATENCY_CASES, ORDER_CASE,
                             ORDER_POS)
from launch_forms import PLACEHOLDER, agg_wpr, expected_forms, launch_descriptors
from test_bf16_gpu import TOL_ORACLE
from test_launch_forms_gpu import TOL_FAC, TOL_FEAT      # (the gates; importing them needs no GPU)
from test_launch_plan_cpu import MODES, _ask, _lib, _name, check_plans

# (B, N); B = 63: the pairwise group's 4158 pair rows are 130 row blocks, between the two points of the waves' rule
SIZES = [(3, 11), (63, 11), (400, 11), (2232, 11), (3, 17)]


# ---- the launchers' plans ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,dtype", MODES, ids=[p if d == "fp32" else d for p, d in MODES])
def test_plans_at_every_edge_type_count(precision, dtype):
    """gn_agg_mlp_plan_* / gn_mlp2_plan_* / gn_node2edge_plan_* / gn_agg_gather_plan_* / gn_agg_scatter_plan_* of a forward
    whose modules have K types against `expected_forms(..., types=)`: K in every module, in the pairwise module alone
    and in the hyper modules alone."""
    seen = set()
    for (B, N), K in itertools.product(SIZES, K_AGG):
        scales = [2, 5, N]
        for types in ((K, K, K, K), (K, 10, 10, 10), (6, K, K, K), (6, K, 10, 1 + (K + 7) % 16)):
            kw = dict(B=B, N=N, scales=scales, precision=precision, dtype=dtype, types=types)
            forms = expected_forms(**kw)
            check_plans(forms, launch_descriptors(**kw), True, kw)
            assert [g["K"] for g in forms["groups"]] == list(types)
            seen |= {(g["name"] == "pair", g["node_form"], g["wpr"]) for g in forms["groups"]}
            seen.add(("fused", forms["fused_closing"], min(g["K"] for g in forms["groups"][1:]) >= 4))
    # the sweep reaches both node-form answers and every number of waves per row block, and the closing stage is refused
    # for want of types as well as taken
    twin, x16 = dtype == "bf16", precision != "fp32"
    assert {(False, False, w) for w in (1, 2, 4)} <= seen
    assert twin or {(True, False, w) for w in (1, 2, 4)} <= seen      # (the twins' pairwise group: the scene form up to N = 64)
    assert ((True, True, 1) in seen) == (twin or x16)
    if x16 and not twin:
        assert {("fused", True, True), ("fused", False, False), ("fused", True, False)} <= seen


def test_waves_per_row_block_by_edge_types():
    """The rule itself, on both sides of each of its points: K = 1 never splits, K = 2, 3 split only from 128 row blocks
    on, K >= 4 always below 768."""
    for K in K_AGG:
        small, mid, large = agg_wpr(127 * 32, K), agg_wpr(127 * 32 + 1, K), agg_wpr(767 * 32 + 1, K)
        assert (small, mid, large) == (4 if K >= 4 else 1, 2 if K >= 2 else 1, 1), K
        assert agg_wpr(767 * 32, K) == mid
        for rows, want in ((127 * 32, small), (127 * 32 + 1, mid), (767 * 32 + 1, large)):
            L, _ = _lib()
            P = PLACEHOLDER
            for twin, fields in ((False, dict(W=P)), (False, dict(W12x=P, W12h=P)), (True, dict(W12x=P))):
                arr = (L.AggGroup * 1)(L.AggGroup(eo=P, edge_feat=P, b1=P, b2=P, feat=P, rows=rows, K=K, **fields))
                rc, plan = _ask("agg_mlp", twin, arr)
                assert rc == 0 and plan.wpr[0] == want, (K, rows, twin, rc, plan.wpr[0])


def test_single_group_launch_forms_of_the_gpu_cases():
    """`agg_launch_forms`, which tests/test_edge_types_gpu.py holds every launch's plan against, reaches every number of
    waves per row block in the eo and the pair form, and stays within the launch sizes the cases name."""
    got = {(c[0], agg_launch_forms(c, K, "f16x3")["wpr"]) for c in AGG_CASES_FP32 for K in K_AGG if c[0] != "pair-node"}
    assert {("eo", 1), ("eo", 2), ("eo", 4), ("pair", 1), ("pair", 2), ("pair", 4), ("gather", 1), ("gather", 4)} <= got
    blocks = {c: (agg_rows(c) + 31) // 32 for c in AGG_CASES_FP32}
    assert all(b < 128 for c, b in blocks.items() if c[1] == 3) and blocks[("eo", 37, 0, 111)] == 129
    assert 128 <= blocks[("pair", 63, 11, 0)] < 768 and agg_rows(("eo", 37, 0, 111)) % 32 != 0


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_launchers_refuse_edge_type_counts_outside_their_range():
    """The launcher and its plan query return the same code (-2, GN_ERR_SHAPE) and launch nothing: aggregation K = 0 and
    17 (every source form), edge head K = 0 and 16, the node form beyond K = 12."""
    L, lib = _lib()
    P = ctypes.c_void_p
    plan = ctypes.byref(L.LaunchPlan())

    def both(stem, arr, *args, tail=(), twin=False):
        sfx = "bf16" if twin else "f32"
        a = getattr(lib, f"gn_{stem}_{sfx}")(arr, *args, P(0))
        b = getattr(lib, f"gn_{stem}_plan_{sfx}")(arr, *args, *tail, plan)
        assert a == b, (stem, a, b)
        return a
    for K in (0, 17, -1):
        for fields in (dict(eo=16, W=16), dict(eo=16, W12x=16, W12h=16), dict(ori=16, H=16, E=5, N=5, W12x=16),
                       dict(A=16, E=15, N=5, sym=1, W2x=16, W2h=16), dict(A=16, E=15, N=5, sym=1, W2x=16, node_form=1)):
            a = (L.AggGroup * 1)(L.AggGroup(edge_feat=16, b1=16, b2=16, feat=16, rows=15, K=K, **fields))
            assert both("agg_mlp", a, 1) == -2, (K, fields)
        a = (L.AggGroup * 1)(L.AggGroup(ori=16, E=15, N=5, sym=1, W12x=16, node_form=1, edge_feat=16, b1=16, b2=16, feat=16,
                                        rows=15, K=K))
        assert both("agg_mlp", a, 1, twin=True) == -2, K            # the twins' scene form
    for K, want in ((12, 0), (13, -2), (16, -2)):
        a = (L.AggGroup * 1)(L.AggGroup(A=16, E=15, N=5, sym=1, W2x=16, W2h=16, node_form=1, edge_feat=16, b1=16, b2=16,
                                        feat=16, rows=15, K=K))
        rc, _ = _ask("agg_mlp", False, a)
        assert rc == want, (K, rc)
        a[0].node_form = 0
        assert _ask("agg_mlp", False, a)[0] == 0, K                 # the pair form takes every K
    for K, want in ((0, -2), (16, -2), (-3, -2)):
        e = (L.EdgeGroup * 1)(L.EdgeGroup(edges=16, W=16, bias=16, edge_feat=16, dist=16, rows=10, K=K))
        assert both("edge_mlp_gumbel", e, 1, 0.5, 0, P(0), tail=(0,)) == want, K
    for K in (1, 15):
        e = (L.EdgeGroup * 1)(L.EdgeGroup(edges=16, W=16, bias=16, edge_feat=16, dist=16, rows=10, K=K))
        rc, p = _ask("edge_mlp_gumbel", False, e, ctypes.c_float(0.5), 0, None, ctypes.c_longlong(0))
        assert rc == 0 and _name(p) == "edge_mlp_gumbel_kernel", K
    for K in (1, 16):
        a = (L.AggGroup * 1)(L.AggGroup(eo=16, W=16, edge_feat=16, b1=16, b2=16, feat=16, rows=15, K=K))
        rc, p = _ask("agg_mlp", False, a)
        assert rc == 0 and _name(p) == "agg_mlp_kernel", K


def test_modules_refuse_edge_type_counts_at_construction():
    import groupnet_amd as G
    from groupnet_amd.MS_HGNN_batch import MLP_dict_softmax, edge_aggregation
    for K in (0, 17, -1):
        with pytest.raises(NotImplementedError):
            edge_aggregation(64, 64, (128,), edge_types=K)
    for K in (0, 16):
        with pytest.raises(NotImplementedError):
            MLP_dict_softmax(64, 64, (128,), edge_types=K)
    assert edge_aggregation(64, 64, (128,), edge_types=16).edge_types == 16
    assert len(edge_aggregation(64, 64, (128,), edge_types=1).agg_mlp) == 1
    kw = dict(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=2)
    for cls in (G.MS_HGNN_oridinary, G.MS_HGNN_hyper):
        with pytest.raises(NotImplementedError):
            with_edge_types(cls, 16)(**kw)                          # (the edge head stops at 15)
        for K in (1, 15):
            m = with_edge_types(cls, K)(**kw)
            assert isinstance(m, cls) and m.edge_types == K and with_edge_types(cls, K) is type(m)
            assert m.nmp_mlp_start.bottleneck_dim == K and m.nmp_mlps[1].bottleneck_dim == K
            assert all(a.edge_types == K and len(a.agg_mlp) == K for a in m.edge_aggregation_list)
            assert m.state_dict()["nmp_mlp_start.MLP_distribution.layers.1.weight"].shape == (K, 128)
    assert G.MS_HGNN_oridinary(**kw).edge_types == 6 and G.MS_HGNN_hyper(**kw).edge_types == 10


def test_noise_shapes_follow_each_modules_edge_types():
    """MultiScaleHGNN.noise_shapes (and with it the graphs' draws per step and the shards' offsets) reads every module's
    own K."""
    import groupnet_amd as G
    from groupnet_amd.multiscale import MultiScaleHGNN
    blk = MultiScaleHGNN([2, 5, 11])
    assert blk.noise_shapes(4, 11) == [(4, 121, 6), (4, 11, 10), (4, 11, 10), (4, 1, 10)]
    kw = dict(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=1)
    blk.interaction = with_edge_types(G.MS_HGNN_oridinary, 3)(**kw)
    blk.interaction_hyper[0] = with_edge_types(G.MS_HGNN_hyper, 15)(scale=2, **kw)
    blk.interaction_hyper[2] = with_edge_types(G.MS_HGNN_hyper, 1)(scale=11, **kw)
    assert blk.noise_shapes(4, 11) == [(4, 121, 3), (4, 11, 15), (4, 11, 10), (4, 1, 1)]
    from oracle import ms_hgnn_oracle as O
    assert [O.noise_shapes(4, 11, s, 1, m.edge_types)[0] for s, m in zip([None, 2, 5, 11], [blk.interaction, *blk.interaction_hyper])
            ] == blk.noise_shapes(4, 11)
    assert O.noise_shapes(4, 11, None, 2) == [(4, 121, 6)] * 2 and O.noise_shapes(4, 11, 11) == [(4, 1, 10)]


# ---- the route ----------------------------------------------------------------------------------------------------------
def test_route_at_every_edge_type_count():
    """K enters the route in one place — the pairwise module's node form on fp32 storage stops at K = 12 — and the route's
    answer is `expected_forms`' at every K; the twins' scene form, the fp32 cores' pair form, the hyper modules and the
    launches of the forward do not move with K."""
    from groupnet_amd import route as R
    knobs = R.Knobs(fuse_pool=True, pool_max_n=16, node_form=True, masked=False)
    base = {}
    for (precision, dtype), N, K in itertools.product(MODES, (11, 16, 17, 64), K_AGG):
        rt = R.message_passing_route(N, ((True, K), (False, K), (False, K)), twin=dtype == "bf16", training=False,
                                     matrix16=precision != "fp32", knobs=knobs, closing_asked=True)
        forms = expected_forms(3, N, [2, N], precision, dtype, types=(K, K, K))
        assert [m.node_form for m in rt.modules] == [g["node_form"] for g in forms["groups"]], (precision, dtype, N, K)
        pair = rt.modules[0]
        if dtype == "bf16":
            assert pair.source == R.SCENE
        elif precision == "fp32" or N > 16:
            assert pair.source == R.PAIR
        else:
            assert pair.source == (R.PAIR_NODE if K <= 12 else R.PAIR)
            assert pair.closing_input == (R.NODE_AGG if K <= 12 else R.SCATTER_SPEC)
        rest = (rt.modules[1:], rt.node2edge, rt.gather, rt.scatter, rt.ask_closing, rt.masks)
        assert base.setdefault((precision, dtype, N), rest) == rest, (precision, dtype, N, K)


# ---- the references ------------------------------------------------------------------------------------------------------
def test_fp32_oracle_stays_within_a_third_of_every_gate():
    """The inputs tests/test_edge_types_gpu.py uses (drawn on the CPU from the seeds of tests/edge_type_cases.py): the fp32
    CPU oracle against the float64 one at every K — edge head (TOL_FAC absolute), typed stage (TOL_FEAT of max|ref|) and
    every whole-module case (both) — so that a kernel as accurate as plain fp32 torch has a margin of 3x."""
    worst = dict(edge=0.0, agg=0.0, feat=0.0, fac=0.0)
    with torch.no_grad():
        for K in K_ALL:
            st = state_of(edge_head(K), "head")
            for shape in EDGE_SHAPES:
                edges, U = edge_inputs(K, shape)
                r64, r32 = edge_ref(st, edges, U, shape[3]), edge_ref(st, edges, U, shape[3], torch.float32)
                e = max(abs_err(r32[0], r64[0]), abs_err(r32[1], r64[1]))
                assert e <= TOL_FAC / 3, ("edge head", K, shape, e)
                worst["edge"] = max(worst["edge"], e)
                if K == 1:
                    assert bool((r64[1] == 1).all()) and bool((r32[1] == 1).all())
        for K in K_AGG:
            st = state_of(agg_module(K), "agg")
            for case in AGG_CASES_FP32:
                inp = agg_inputs(K, case)
                e = rel_err(agg_ref(st, case, inp, torch.float32), agg_ref(st, case, inp))
                assert e <= TOL_FEAT / 3, ("typed stage", K, case, e)
                worst["agg"] = max(worst["agg"], e)
        for case in ENGINE_CASES:
            _, states, h, Hs, U, scenes = engine_case(case)
            twin = case["dtype"] == "bf16"
            for (f64, c64), (f32, c32) in zip(engine_ref(states, h, Hs, U, scenes, case["nmp"]),
                                              engine_ref(states, h, Hs, U, scenes, case["nmp"], dtype=torch.float32)):
                ef, ec = rel_err(f32, f64), abs_err(c32, c64)
                assert ef <= (TOL_ORACLE if twin else TOL_FEAT) / 3 and ec <= (TOL_ORACLE if twin else TOL_FAC) / 3, (case["id"], ef, ec)
                worst["feat"], worst["fac"] = max(worst["feat"], ef), max(worst["fac"], ec)
    print(f"\nfp32 oracle against float64: edge head {worst['edge']:.2e} (gate / 3 = {TOL_FAC / 3:.2e}), typed stage "
          f"{worst['agg']:.2e} of max|ref| (gate / 3 = {TOL_FEAT / 3:.2e}), modules {worst['feat']:.2e} / {worst['fac']:.2e}")


def test_references_of_the_pairwise_forms_agree():
    """The node and scene forms' reference (ordered edges through the oracle's pairwise incidence) is H^T of the pair
    form's reference with weight 1 on both nodes of a pair row and on a self-loop's node — what the stand-alone scatter of
    unordered pairs forms — and the edge head's pair rows are the sums of their two ordered edges."""
    from edge_type_cases import pair_index
    K, N = 5, 5
    st = state_of(agg_module(K), "agg")
    inp = agg_inputs(K, ("pair", 3, N, 0))
    ii, jj, row = pair_index(N)
    Hs = torch.zeros(ii.numel(), N, dtype=torch.float64)
    Hs[torch.arange(ii.numel()), ii] = 1
    Hs[torch.arange(ii.numel()), jj] = 1
    with torch.no_grad():
        per_pair = agg_ref(st, ("pair", 3, N, 0), inp)
        per_node = agg_ref(st, ("pair-node", 3, N, 0), inp)
    assert rel_err(torch.matmul(Hs.t(), per_pair), per_node) <= 1e-14
    assert row.tolist()[:6] == [0, 1, 2, 3, 4, 1] and (ii[:6].tolist(), jj[:6].tolist()) == ([0, 0, 0, 0, 0, 1], [0, 1, 2, 3, 4, 1])


def test_engine_cases_reach_the_forms_they_name():
    """The latency cases take the closing stage exactly from K = 4 on (B = 7: fewer than 128 row blocks per hyper group)
    and from K = 2 on (B = 400: 138), with unequal shares at K = 3, 5 and 15; the order case's positions are the rule's."""
    for case in LATENCY_CASES:
        forms, kh = engine_forms(case), case["types"][1]
        assert forms["groups"][0]["node_form"] and forms["fused_closing"] == (kh >= (4 if case["B"] == 7 else 2)), case["id"]
        b32 = [(g["rows"] + 31) // 32 for g in forms["groups"][1:]]
        assert all(b < 128 for b in b32) if case["B"] == 7 else all(128 <= b < 768 for b in b32), (case["id"], b32)
        assert [g["wpr"] for g in forms["groups"][1:]] == [agg_wpr(g["rows"], kh) for g in forms["groups"][1:]]
    assert {(c["B"], c["types"][1] % agg_wpr(c["B"] * 11, c["types"][1]) != 0) for c in LATENCY_CASES} == {
        (7, False), (7, True), (400, False), (400, True)}
    assert engine_forms(ORDER_CASE)["agg_pos"] == ORDER_POS and not engine_forms(ORDER_CASE)["fused_closing"]


def test_backward_cases_find_inputs_on_the_oracle_alone():
    """Every case of the GPU backward test finds, among its 16 seeded draws, inputs on which the float64 oracle keeps every
    ReLU input beyond RELU_MARGIN of zero and has a clean scene — decided here, without the code under test."""
    from edge_type_cases import BACKWARD_K, BACKWARD_KINDS, BACKWARD_SIZES, backward_case, backward_reference, live_parameters
    shifts = {}
    for kind, K, (B, N) in itertools.product(BACKWARD_KINDS, BACKWARD_K, BACKWARD_SIZES):
        c = backward_case(kind, K, B, N)
        assert c["h"].shape == (B, N, 64) and c["U"].shape[-1] == K and c["mod"].edge_types == K
        shifts[kind, K, B, N] = c["shift"]
        # the parameters whose gradient is zero as a function: those the forward never reaches and, at K = 1, the
        # distribution head — on the whole batch and on its clean scenes alone
        for rows in (torch.arange(B), torch.arange(B)[backward_reference(kind, c, torch.arange(B))["probe"].clean()]):
            r = backward_reference(kind, c, rows)
            assert len(r["grads"]) - len(r["dead"]) == live_parameters(kind, K), (kind, K, B, N, r["dead"])
            assert all(("MLP_distribution" in k) == (K == 1) or "nmp_mlp_start" not in k for k in r["dead"])
            assert not any("attention_mlp" in k or "agg_mlp" in k or "nmp_mlp_end" in k for k in r["dead"])
    print(f"\nbackward cases: draws used {sorted(set(shifts.values()))}, the latest for "
          f"{max(shifts, key=shifts.get)} ({max(shifts.values())})")
