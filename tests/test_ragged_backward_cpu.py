"""CPU checks of ragged training (tests/ragged_backward_cases.py): the routes with and without the opt-in, the kernel
reference pinned to the golden-pinned oracle, the seeded flaws, the module oracle's plumbing, and the switch itself."""
import itertools

import pytest
import torch

import backward_kernel_refs as R
import ragged_backward_cases as RB
import ragged_cases as C
from oracle import ms_hgnn_oracle as O
from test_backward_gpu import TOL_CLEAN, _modules

F64 = torch.float64
MIXES = [((True, 6),), ((False, 10),), ((True, 6), (False, 10), (False, 10)), ((True, 3), (False, 16))]
SIZES = [1, 5, 11, 16, 17, 50, 64, 65, 140, 141, 200]


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


# ---- 1. the routes -------------------------------------------------------------------------------------------------
def _knobs(route, masked=False):
    return route.Knobs(fuse_pool=True, pool_max_n=16, node_form=True, masked=masked)


@pytest.mark.parametrize("matrix16", [True, False])
def test_forward_route_with_and_without_the_opt_in(matrix16):
    from groupnet_amd import route as RT
    for N, mods, masked in itertools.product(SIZES, MIXES, (False, True)):
        kw = dict(twin=False, training=True, matrix16=matrix16, knobs=_knobs(RT, masked), closing_asked=True, ragged=True)
        with pytest.raises(NotImplementedError, match="inference-only"):
            RT.message_passing_route(N, mods, **kw)
        with pytest.raises(NotImplementedError, match="inference-only"):
            RT.message_passing_route(N, mods, ragged_training=False, **kw)
        r = RT.message_passing_route(N, mods, ragged_training=True, **kw)
        every = tuple(range(len(mods)))
        assert r.node2edge == every and r.scatter == every and not r.masks and not r.ask_closing
        assert r.gather == tuple(i for i, (pw, _) in enumerate(mods) if not pw and N > 16)
        for (pw, _), m in zip(mods, r.modules):
            assert not m.pool_in_edge_kernel and not m.node_form and m.closing_input == RT.SCATTER
            assert m.first_layer == pw
            assert m.source == (RT.PAIR if pw else RT.FUSED_GATHER if N <= 16 else RT.EO)
        # it is the ragged inference route: that one already keeps what the backward reads
        assert r == RT.message_passing_route(N, mods, **{**kw, "training": False})
        # the opt-in changes nothing else: full-batch training, and the twins under training
        full = {**kw, "ragged": False}
        assert RT.message_passing_route(N, mods, ragged_training=True, **full) == RT.message_passing_route(N, mods, **full)
        with pytest.raises(NotImplementedError, match="forward-only"):
            RT.message_passing_route(N, mods, ragged_training=True, **{**kw, "twin": True})


def test_graph_stage_route_with_and_without_the_opt_in():
    from groupnet_amd import route as RT
    training = RT.StageFacts(grouped=True, latency_form=False, capturing=False, embed=False, may_defer=False)
    eager = RT.StageFacts(grouped=True, latency_form=True, capturing=True, embed=False, may_defer=True)
    for S, form, rows, masked, facts in itertools.product((0, 1, 3), ("tail", "fused", "banded"), (77, 1 << 16),
                                                          (False, True), (training, eager)):
        kw = dict(masked=masked, ragged=True, training=True, facts=facts)
        with pytest.raises(NotImplementedError, match="inference-only"):
            RT.graph_stage_route(S, form, rows, **kw)
        g = RT.graph_stage_route(S, form, rows, ragged_training=True, **kw)
        kind = RT.NONE if S == 0 else RT.BANDED if form == "banded" else RT.FUSED
        # the training stage: launched at once, no final and no counter of its own, nothing asked of the closing stage
        assert g == RT.GraphStage(kind=kind, masks=False, fork=False, deferred=False, own_copy=False, ask_closing=False,
                                  H_cat=S >= 1)
        full = {**kw, "ragged": False}
        assert RT.graph_stage_route(S, form, rows, ragged_training=True, **full) == RT.graph_stage_route(S, form, rows, **full)


def test_backward_round_route_with_counts():
    from groupnet_amd import route as RT
    assert RT.N2E_BWD_SCENE_MAX_N == RB.LDS_LIMIT_N
    assert RB.scene_lds(RB.LDS_LIMIT_N) <= 150 * 1024 < RB.scene_lds(RB.LDS_LIMIT_N + 1)
    for N, pairwise in itertools.product(SIZES, ((True,), (False,), (True, False, False))):
        if N <= RB.LDS_LIMIT_N:
            assert RT.backward_round_route(N, pairwise, True) == RT.BackwardRound(pair_rows=True, kept=True, n2e_grouped=True)
            assert RT.backward_round_route(N, pairwise, True) == RT.backward_round_route(N, pairwise)
        else:
            with pytest.raises(NotImplementedError, match=str(RB.LDS_LIMIT_N)):
                RT.backward_round_route(N, pairwise, True)
            assert not RT.backward_round_route(N, pairwise).n2e_grouped        # the full-batch answer stands
        assert RT.backward_round_route(N, pairwise, False) == RT.backward_round_route(N, pairwise)


# ---- 2. the kernel reference is the oracle's --------------------------------------------------------------------------
@pytest.mark.parametrize("case", [RB.KERNEL_CASES[0], RB.KERNEL_CASES[3], RB.GROUPED[2]], ids=lambda c: c.name)
def test_kernel_reference_equals_per_scene_oracle_autograd(case):
    """Per scene, the oracle's node2edge(decomposed=True) on the scene ALONE (identity start layer, x' = x): its
    gradients w.r.t. x, attention layer 0 (W1, b1) and layer 1 (w2, b2), summed over the scenes, against the helper's
    dxp / dpq / dw2 / db2 chained through pq = [P | Qn]."""
    g = torch.Generator().manual_seed(7)
    inp = RB.kernel_inputs(case)
    x = inp["xp"].double()
    W1 = torch.randn(32, 128, generator=g, dtype=F64)
    b1 = torch.randn(32, generator=g, dtype=F64)
    w2, b2 = inp["w2"].double()[None].clone(), inp["b2"].double().clone()
    state = {"node2edge_start_mlp.0.layers.0.weight": torch.eye(64, dtype=F64),
             "node2edge_start_mlp.0.layers.0.bias": torch.zeros(64, dtype=F64),
             "attention_mlp.0.layers.0.weight": W1, "attention_mlp.0.layers.0.bias": b1,
             "attention_mlp.0.layers.1.weight": w2, "attention_mlp.0.layers.1.bias": b2}
    for t in (W1, b1, w2, b2):
        t.requires_grad_(True)
    gx = torch.zeros_like(x)
    gpar = [torch.zeros_like(t) for t in (W1, b1, w2, b2)]
    for b, n in enumerate(case.counts):
        if n == 0:
            continue
        sl = RB.scene_slice(case, inp, b)
        xb = x[b:b + 1, :n].clone().requires_grad_(True)
        edges, _ = O.node2edge(state, xb, sl["H"].double(), decomposed=True)
        got = torch.autograd.grad((edges * sl["dedges"].double()).sum(), (xb, W1, b1, w2, b2))
        gx[b, :n] = got[0][0]
        for acc, t in zip(gpar, got[1:]):
            acc += t
    Wd, bd = W1.detach(), b1.detach()
    pq = torch.cat((x @ Wd[:, :64].t() + bd, x @ Wd[:, 64:].t()), dim=-1)
    zero = {k: torch.zeros_like(inp[k]) for k in ("dxp0", "dpq0", "dw20", "db20")}
    r = RB.kernel_grads(case, F64, {**inp, **zero, "pq": pq})
    dP, dQn = r["dpq"][..., :32], r["dpq"][..., 32:]
    assert _rel(r["dxp"] + dP @ Wd[:, :64] + dQn @ Wd[:, 64:], gx) <= 1e-12
    assert _rel(torch.cat((torch.einsum("bnc,bnd->cd", dP, x), torch.einsum("bnc,bnd->cd", dQn, x)), dim=1), gpar[0]) <= 1e-12
    assert _rel(dP.sum(dim=(0, 1)), gpar[1]) <= 1e-12
    assert _rel(r["dw2"], gpar[2][0]) <= 1e-12
    # (db2 of all-member rows is an exact zero sum — the softmax is shift-invariant: relative to its absolute terms)
    assert float((r["db2"] - gpar[3]).abs().max()) <= 1e-12 * r["db2_scale"]
    # padded rows: nothing flows into them
    for b, n in enumerate(case.counts):
        assert not bool(r["dxp"][b, n:].any()) and not bool(r["dpq"][b, n:].any())


@pytest.mark.parametrize("case", RB.KERNEL_CASES[:4] + RB.GROUPED, ids=lambda c: c.name)
def test_second_statement_of_the_counted_softmax_agrees(case):
    """`counted_pool` (the statement the flaws are seeded into) without a flaw gives the reference's buffers, and its
    forward is `ragged_size_cases.node2edge_counted`'s."""
    a, b = RB.counted_grads(case, F64), RB.kernel_grads(case, F64)
    for o in R.N2E_OUTPUTS:
        assert _rel(a[o], b[o]) <= 1e-12, o
    inp = RB.kernel_inputs(case)
    scene = next(i for i, n in enumerate(case.counts) if 0 < n < case.N)
    n = case.counts[scene]
    g = torch.Generator().manual_seed(3)
    W1, b1 = torch.randn(32, 128, generator=g, dtype=F64), torch.randn(32, generator=g, dtype=F64)
    state = {"node2edge_start_mlp.0.layers.0.weight": torch.eye(64, dtype=F64),
             "node2edge_start_mlp.0.layers.0.bias": torch.zeros(64, dtype=F64),
             "attention_mlp.0.layers.0.weight": W1, "attention_mlp.0.layers.0.bias": b1,
             "attention_mlp.0.layers.1.weight": inp["w2"].double()[None], "attention_mlp.0.layers.1.bias": inp["b2"].double()}
    x, H = inp["xp"][scene].double(), inp["H"][scene].double()
    pq = torch.cat((x @ W1[:, :64].t() + b1, x @ W1[:, 64:].t()), dim=-1)
    mine = RB.counted_pool(x, pq, H, inp["w2"].double(), inp["b2"].double(), n)
    theirs = RB.node2edge_counted(state, x[None], H[None], torch.tensor([n]))[0]
    assert _rel(mine, theirs) <= 1e-12


@pytest.mark.parametrize("case", RB.KERNEL_CASES + RB.GROUPED, ids=lambda c: c.name)
def test_kernel_case_inputs(case):
    """What the gate rests on: exact ReLU decisions (dyadic grid), the cases' count edges, a reference whose own fp32
    distance stays inside the ceiling."""
    inp = RB.kernel_inputs(case)
    assert bool(((inp["pq"] * 64) == (inp["pq"] * 64).round()).all())
    assert set(inp["H"].unique().tolist()) <= {0.0, 0.5, 1.0, 2.0}
    for b, n in enumerate(case.counts):
        assert not bool(inp["H"][b, :, n:].any())
        if case.kind == "hyper" and case.E == case.N:
            assert not bool(inp["H"][b, n:].any())
    r64, r32 = RB.kernel_expected(case)
    for o in R.N2E_OUTPUTS:
        bound, e32, scale, _ = RB.kernel_gate(case, o, TOL_CLEAN)
        print(f"\n{case.name} {o}: e32 {e32:.2e} gate {bound:.2e} scale {scale:.2e}", end="")
        assert 4 * e32 <= TOL_CLEAN * scale, (case.name, o, e32, scale)
    if case.name == "hyper_e11":
        H = inp["H"]
        n = case.counts[1]
        members = (H[1] != 0).sum(-1)
        assert int(members[0]) == n and int(members[1]) == 1 and bool((members[2:n] < n).all()) and 0 in case.counts
    if case.name == "big_lds":
        assert 64 * 1024 < RB.scene_lds(case.N) <= 150 * 1024


# ---- 3. the seeded flaws ----------------------------------------------------------------------------------------------
SEES = {"N_for_nb": [c.name for c in RB.KERNEL_CASES + RB.GROUPED],
        "zero_in_max": ["one_allones", "grp_one"],
        "invalid_pair": ["ordered", "sym", "grp_sym"]}


@pytest.mark.parametrize("flaw", RB.FLAWS)
def test_seeded_flaws_are_detected(flaw):
    by_name = {c.name: c for c in RB.KERNEL_CASES + RB.GROUPED}
    for name in SEES[flaw]:
        moves = RB.flaw_moves(by_name[name], flaw, TOL_CLEAN)
        print(f"\n{flaw} on {name}: " + ", ".join(f"{o} {m:.1e}" for o, m in moves.items()), end="")
        assert max(moves.values()) > RB.FLAW_FACTOR, (flaw, name, moves)


# ---- 4. the module oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,N,counts,scale,min_used", [("pair", 5, (5, 3, 2, 1), None, 30), ("hyper", 7, (7, 4, 3, 2, 1), 3, 40),
                                                          ("hyper", 7, (7, 4, 3, 2, 1), 7, 40)])
def test_module_oracle_plumbing(kind, N, counts, scale, min_used):
    case = RB.settled_case(N, counts, [scale] if scale else [], seed=N)
    h, U = C.inputs(case)
    h = C.with_garbage(case, h)
    assert C.min_gap(case, h) >= C.MIN_GAP
    pair, hyper = _modules(300 + N)
    mod = pair if kind == "pair" else hyper
    state = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    E = N * N if kind == "pair" else (1 if scale == N else N)
    R1, R2 = torch.randn(case["B"], N, 64, generator=g), torch.randn(case["B"], E, mod.edge_types, generator=g)
    ref = RB.module_oracle(state, kind == "pair", scale, case, h, U[0] if kind == "pair" else U[1], R1, R2)
    for b, n in enumerate(counts):
        assert not bool(ref["g_h"][b, n:].any()) and bool(ref["g_h"][b, :n].any())
        assert not bool(ref["node_feat"][b, n:].any())
    used = [k for k, v in ref["grads"].items() if v is not None and float(v.abs().max()) > 0]
    assert len(used) >= min_used, len(used)
    # garbage in the padded rows does not reach the oracle: the same batch with clean padding gives the same gradients
    ref2 = RB.module_oracle(state, kind == "pair", scale, case, C.inputs(case)[0], U[0] if kind == "pair" else U[1], R1, R2)
    assert torch.equal(ref["g_h"], ref2["g_h"])
    # the sum over scenes is a sum: two halves of the batch add up
    half = RB.module_oracle(state, kind == "pair", scale, case, h, U[0] if kind == "pair" else U[1], R1, R2, scenes=[0, 1])
    rest = RB.module_oracle(state, kind == "pair", scale, case, h, U[0] if kind == "pair" else U[1], R1, R2,
                            scenes=range(2, case["B"]))
    for k in used:
        assert _rel(half["grads"][k] + rest["grads"][k], ref["grads"][k]) <= 1e-12, k


# ---- 5. the switch ---------------------------------------------------------------------------------------------------
def test_ragged_training_switch(monkeypatch):
    import groupnet_amd as G
    from groupnet_amd import MS_HGNN_batch as M
    monkeypatch.delenv("GN_RAGGED_TRAINING", raising=False)
    monkeypatch.setattr(M, "_RAGGED_TRAINING", None)
    assert G.ragged_training() is False                      # default off
    monkeypatch.setenv("GN_RAGGED_TRAINING", "1")
    assert G.ragged_training() is True                       # read per call
    G.set_ragged_training(False)
    assert G.ragged_training() is False                      # the setter wins
    monkeypatch.setenv("GN_RAGGED_TRAINING", "0")
    G.set_ragged_training(True)
    assert G.ragged_training() is True
    G.set_ragged_training(None)                              # back to the environment
    assert G.ragged_training() is False
    # the refusals a forward asks for: everything without the opt-in, a size beyond the per-scene backward with it
    assert M.ragged_grad_refusals(True, 11) == dict(grad=True, large=False)
    assert M.ragged_grad_refusals(False, 500) == dict(grad=False, large=False)
    G.set_ragged_training(True)
    assert M.ragged_grad_refusals(True, 140) == dict(grad=False, large=False)
    assert M.ragged_grad_refusals(True, 141) == dict(grad=False, large=True)
    assert M.ragged_grad_refusals(False, 141) == dict(grad=False, large=False)
    with pytest.raises(NotImplementedError, match="140"):
        M.refuse_ragged(**M.ragged_grad_refusals(True, 141))
    G.set_ragged_training(None)
