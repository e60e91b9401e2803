"""The deterministic training mode on the GPU ("Deterministic training").

Kernels alone: the ordered split-K GEMM (gn_gemm_grouped_det_f32) and the ordered node->edge backward
(gn_node2edge_bwd_det_grouped_f32) against the float64 references under the gates their default forms are held to
(backward_kernel_refs.gate, TOL_CLEAN / SPLITK_CEILING, ragged_backward_cases.kernel_gate) — and the ORDER of their sums,
bit for bit: the partial of every K slice / every scene is produced on its own and added in the stated order with
elementwise fp32 torch adds; the result must be `torch.equal`.
Modules: the gradient gates of tests/test_backward_gpu.py and tests/test_ragged_backward_gpu.py with the mode on (restated in
tests/deterministic_cases.py), two backward passes bit-equal, a graphed training step bit-equal to its eager twin in the
updated weights, the encoder, and the two incidence forms."""
import copy
import os

import numpy as np
import pytest
import torch

import backward_kernel_refs as R
import deterministic_cases as D
import ragged_backward_cases as RB
import ragged_cases as C
import test_backward_gpu as TB
import test_backward_kernels_gpu as TK
import test_ragged_backward_gpu as TRB

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def mode_on():
    import groupnet_amd as G
    G.set_deterministic(True)
    G.set_ragged_training(True)
    yield
    G.set_deterministic(None)
    G.set_ragged_training(None)


def _api():
    from groupnet_amd import _lib
    return _lib, _lib.load(), dev()


_bits = TK._bits


# ---- 1. the ordered GEMM: accuracy ----------------------------------------------------------------------------------
def _run_cases(cases):
    """One GemmBatch over the cases with the current mode -> [(Cbuf, colsum)]."""
    from groupnet_amd.backward import GemmBatch
    gb = GemmBatch()
    held = [TK._gemm_add(gb, c, dev()) for c in cases]
    gb.run()
    torch.cuda.synchronize()
    return held


def test_gemm_det_accuracy_on_the_accumulate_cases():
    cases = R.GEMM_ACCUM + D.ORDER_CASES
    bad = []
    for c, (Cbuf, cs) in zip(cases, _run_cases(cases)):
        TK._gemm_verdict(bad, c, Cbuf, cs)
    assert not bad, bad


def test_gemm_det_runs_other_problems_as_the_default_entry_does():
    import groupnet_amd as G
    order = [c for pair in zip(R.GEMM_BATCH[:16], R.GEMM_BATCH[16:32]) for c in pair] + R.GEMM_BATCH[32:]
    on = _run_cases(order)
    G.set_deterministic(False)
    off = _run_cases(order)
    bad = []
    for c, (a, _), (b, _) in zip(order, on, off):
        assert torch.equal(_bits(a), _bits(b)), c.name
        TK._gemm_verdict(bad, c, a, None)
    assert not bad, bad


# ---- 2. the ordered GEMM: the order of the sum ------------------------------------------------------------------------
def _det(problems):
    """gn_gemm_grouped_det_f32 through `GemmBatch` on [(case, operands, C or None, colsum or None)]."""
    from groupnet_amd.backward import GemmBatch
    gb = GemmBatch()
    for c, o, C_, cs in problems:
        D.add(gb, c, o, C_, cs)
    gb.run()
    torch.cuda.synchronize()


def _partials(c, o):
    """[(partial tile in C's orientation, partial column sums or None)] of the K slices, each from a launch of its own: a
    plain one-split problem (beta = 0 onto NaN; colsum onto zeros), or for GN_GEMM_TRANS_C — which has no plain form — the
    ordered entry on the slice with a zeroed destination."""
    import groupnet_amd as G
    from groupnet_amd.backward import GemmBatch
    out = []
    for s in D.k_slices(c, o):
        gb = GemmBatch()
        cs = torch.zeros(c.M, device=dev()) if c.colsum else None
        if c.tC:
            P = torch.zeros(c.N, c.M, device=dev())
            gb.add(s["A"], s["B"], P, tA=c.tA, tB=c.tB, rs=s["rs"], alpha=c.alpha, accum=True, tC=True)
            gb.run()
        else:
            P = torch.full((c.M, c.N), float("nan"), device=dev())
            gb.add(s["A"], s["B"], P, tA=c.tA, tB=c.tB, rs=s["rs"], alpha=c.alpha, colsum=cs)
            G.set_deterministic(False)
            gb.run()
            G.set_deterministic(True)
        out.append((P, cs))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", D.ORDER_CASES, ids=lambda c: c.name)
def test_gemm_det_adds_its_splits_in_ascending_order(case):
    c, o = case, D.operands(case, dev())
    C_old = o["C"].clone()
    cs_old = o["colsum"].clone() if c.colsum else None
    _det([(c, o, None, None)])
    v, vs = C_old, cs_old
    for P, cs in _partials(c, o):
        v = v + P
        if c.colsum:
            vs = vs + cs
    assert torch.equal(o["C"], v), c.name
    if c.colsum:
        assert torch.equal(o["colsum"], vs), c.name


def test_gemm_det_chains_identical_destinations_in_descriptor_order():
    c1, c2 = D.ORDER_CASES[0], D.CHAIN_SECOND
    o1, o2 = D.operands(c1, dev()), D.operands(c2, dev())
    C_old, cs_old = o1["C"].clone(), o1["colsum"].clone()
    _det([(c1, o1, None, None), (c2, o2, o1["C"], o1["colsum"])])
    v, vs = C_old, cs_old
    for c, o in ((c1, o1), (c2, o2)):
        for P, cs in _partials(c, o):
            v, vs = v + P, vs + cs
    assert torch.equal(o1["C"], v) and torch.equal(o1["colsum"], vs)
    # ... and the other order is another sum: the chain follows the descriptors, not the addresses
    o1b, o2b = D.operands(c1, dev()), D.operands(c2, dev())
    _det([(c2, o2b, o1b["C"], o1b["colsum"]), (c1, o1b, None, None)])
    w, ws = C_old, cs_old
    for c, o in ((c2, o2b), (c1, o1b)):
        for P, cs in _partials(c, o):
            w, ws = w + P, ws + cs
    assert torch.equal(o1b["C"], w) and torch.equal(o1b["colsum"], ws)


def test_gemm_det_problem_alone_and_among_others():
    """Alone, among 3 and among 17 others (a second table's worth: the batch is cut) at a middle position: the same bits."""
    others = (R.GEMM_ACCUM + R.GEMM_BATCH[:4] + D.ORDER_CASES[1:] + R.GEMM_BATCH[16:20])[:17]
    assert len(others) == 17 and sum(c.accum for c in others) >= 9
    for c in (D.ORDER_CASES[0], R.GEMM_ACCUM[6]):       # vector path with colsum; scalar path written transposed
        alone = D.operands(c, dev())
        _det([(c, alone, None, None)])
        for n in (3, 17):
            mine = D.operands(c, dev())
            probs = [(k, D.operands(k, dev()), None, None) for k in others[:n]]
            probs.insert(n // 2, (c, mine, None, None))
            _det(probs)
            assert torch.equal(_bits(mine["Cbuf"]), _bits(alone["Cbuf"])), (c.name, n)
            if c.colsum:
                assert torch.equal(mine["colsum"], alone["colsum"]), (c.name, n)


def test_gemm_det_three_launches_are_bit_equal():
    cases = R.GEMM_ACCUM + D.ORDER_CASES
    runs = [_run_cases(cases) for _ in range(3)]
    for i, c in enumerate(cases):
        for r in runs[1:]:
            assert torch.equal(_bits(r[i][0]), _bits(runs[0][i][0])), c.name
            if c.colsum:
                assert torch.equal(r[i][1], runs[0][i][1]), c.name


# ---- 3. the ordered node->edge backward --------------------------------------------------------------------------------
def _n2e_group(L, d, o, E, sym, explicit):
    return L.N2EBwdGroup(xp=L.addr(d["xp"]), pq=L.addr(d["pq"]), H=L.addr(d["H"] if explicit else None), w2=L.addr(d["w2"]),
                         b2=L.addr(d["b2"]), dedges=L.addr(d["dedges"]), dxp=L.addr(o["dxp"]), dpq=L.addr(o["dpq"]),
                         dw2=L.addr(o["dw2"]), db2=L.addr(o["db2"]), E=E, sym=int(sym))


def _n2e_det(groups, B, N, nv=None, expect=0):
    L, lib, _ = _api()
    arr = (L.N2EBwdGroup * len(groups))(*groups)
    part = torch.full((len(groups) * B * 33,), float("nan"), device=dev())
    with torch.cuda.device(dev()):
        rc = lib.gn_node2edge_bwd_det_grouped_f32(arr, len(groups), B, N, L.addr(nv), L.addr(part), L.stream_handle())
    torch.cuda.synchronize()
    assert rc == expect, rc
    return part


def _full(case):
    """(d, out, group) of a full-batch case of backward_kernel_refs."""
    L, _, _ = _api()
    d, out = TK._n2e_buffers(case, dev())
    return d, out, _n2e_group(L, d, out, case.E, case.kind == "sym", case.kind == "hyper")


def _ragged(case):
    L, _, _ = _api()
    d, out, nv = TRB._buffers(case)
    return d, out, nv, _n2e_group(L, d, out, case.E, case.kind == "sym", case.kind in ("hyper", "one"))


@pytest.mark.parametrize("case", [c for c in R.N2E_CASES if c.N <= D.N2E_MAX_N], ids=lambda c: c.name)
def test_node2edge_bwd_det(case):
    d, out, g = _full(case)
    _n2e_det([g], case.B, case.N)
    bad = []
    TK._n2e_verdict(bad, case, d, out)
    assert not bad, bad


def test_node2edge_bwd_det_grouped():
    held = [_full(c) for c in R.N2E_GROUPED]
    _n2e_det([g for _, _, g in held], 3, 11)
    bad = []
    for c, (d, o, _) in zip(R.N2E_GROUPED, held):
        TK._n2e_verdict(bad, c, d, o)
        if c.zero_scene == -2:
            assert torch.equal(_bits(o["dw2"]), _bits(d["dw20"])) and torch.equal(_bits(o["db2"]), _bits(d["db20"]))
    assert not bad, bad


@pytest.mark.parametrize("case", RB.KERNEL_CASES, ids=lambda c: c.name)
def test_node2edge_bwd_det_ragged(case):
    d, out, nv, g = _ragged(case)
    _n2e_det([g], case.B, case.N, nv)
    bad = []
    TRB._verdict(bad, case, d, out)
    assert not bad, bad


def test_node2edge_bwd_det_ragged_grouped():
    held = [_ragged(c) for c in RB.GROUPED]
    _n2e_det([g for _, _, _, g in held], 3, 11, held[0][2])
    bad = []
    for c, (d, o, _, _) in zip(RB.GROUPED, held):
        TRB._verdict(bad, c, d, o)
    assert not bad, bad


def test_node2edge_bwd_det_beyond_the_scene_form_touches_nothing():
    L, _, _ = _api()
    for case in (c for c in R.N2E_CASES if c.N > D.N2E_MAX_N):
        d, out, g = _full(case)
        nv = torch.full((case.B,), 3, dtype=torch.int32, device=dev())
        for counts in (None, nv):
            part = _n2e_det([g], case.B, case.N, counts, expect=L.GN_ERR_LDS)
            assert bool(torch.isnan(part).all())
        for o in R.N2E_OUTPUTS:
            assert torch.equal(_bits(out[o]), _bits(d[o + "0"])), (case.name, o)


def _solo_scene(L, d, start, b, E, sym, explicit, N, count):
    """Scene b alone (B = 1) from the batch's start rows, dw2 / db2 zeroed -> (dxp row block, dpq row block, dw2, db2)."""
    one = {k: (v[b:b + 1].contiguous() if k in ("xp", "pq", "H", "dedges") else v) for k, v in d.items()}
    o = dict(dxp=start["dxp"][b:b + 1].clone(), dpq=start["dpq"][b:b + 1].clone(), dw2=torch.zeros(32, device=dev()),
             db2=torch.zeros(1, device=dev()))
    nv = None if count is None else torch.tensor([count], dtype=torch.int32, device=dev())
    _n2e_det([_n2e_group(L, one, o, E, sym, explicit)], 1, N, nv)
    return o


def _scene_order_check(cases, held, B, N, nv, counts):
    """The batched launch of `held` against every scene alone: a scene's rows bit-equal, dw2 / db2 = the start value plus
    the scenes' partials in ascending scene order (elementwise fp32 adds)."""
    L, _, _ = _api()
    start = [{o: out[o].clone() for o in R.N2E_OUTPUTS} for _, out, _ in held]
    _n2e_det([g for _, _, g in held], B, N, nv)
    for c, (d, out, _), st in zip(cases, held, start):
        dw2, db2 = st["dw2"], st["db2"]
        for b in range(B):
            solo = _solo_scene(L, d, st, b, c.E, c.kind == "sym", c.kind in ("hyper", "one"), N,
                               None if counts is None else counts[b])
            assert torch.equal(_bits(out["dxp"][b]), _bits(solo["dxp"][0])), (c.name, "dxp", b)
            assert torch.equal(_bits(out["dpq"][b]), _bits(solo["dpq"][0])), (c.name, "dpq", b)
            dw2, db2 = dw2 + solo["dw2"], db2 + solo["db2"]
        assert torch.equal(out["dw2"], dw2) and torch.equal(out["db2"], db2), c.name


@pytest.mark.parametrize("name", ["a", "d_sym", "d_ordered", "e_n61"])
def test_node2edge_bwd_det_adds_scenes_in_order(name):
    case = next(c for c in R.N2E_CASES if c.name == name)
    _scene_order_check([case], [_full(case)], case.B, case.N, None, None)


@pytest.mark.parametrize("name", ["hyper_e11", "sym", "ordered"])
def test_node2edge_bwd_det_ragged_adds_scenes_in_order(name):
    case = next(c for c in RB.KERNEL_CASES if c.name == name)       # hyper_e11: the counts (11, 5, 1, 0)
    d, out, nv, g = _ragged(case)
    _scene_order_check([case], [(d, out, g)], case.B, case.N, nv, case.counts)


def test_node2edge_bwd_det_grouped_adds_scenes_in_order():
    _scene_order_check(R.N2E_GROUPED, [_full(c) for c in R.N2E_GROUPED], 3, 11, None, None)
    held = [_ragged(c) for c in RB.GROUPED]
    _scene_order_check(RB.GROUPED, [(d, o, g) for d, o, _, g in held], 3, 11, held[0][2], RB.GROUPED[0].counts)


def test_node2edge_bwd_det_three_launches_are_bit_equal():
    for cases, ragged in ((R.N2E_GROUPED, False), (RB.GROUPED, True)):
        runs = []
        for _ in range(3):
            if ragged:
                held = [_ragged(c) for c in cases]
                _n2e_det([h[3] for h in held], 3, 11, held[0][2])
            else:
                held = [_full(c) for c in cases]
                _n2e_det([h[2] for h in held], 3, 11)
            runs.append([h[1] for h in held])
        for r in runs[1:]:
            for a, b in zip(r, runs[0]):
                assert all(torch.equal(_bits(a[o]), _bits(b[o])) for o in R.N2E_OUTPUTS)


# ---- 4. modules: the gates of the default mode, with the mode on ---------------------------------------------------------
@pytest.mark.parametrize("name", ["n11_b5", "n7_b3_nmp2"])
def test_module_gradients_meet_the_golden_gates(name, monkeypatch):
    """tests/test_backward_gpu.py's comparison with the reference's own gradients (grad_*.npz: MS_HGNN_oridinary and
    MS_HGNN_hyper at every scale), its gates (deterministic_cases.TOL_CLEAN / TOL_ANY), with the mode on."""
    import groupnet_amd as G
    assert G.deterministic()
    TB.test_hip_backward_matches_reference_gradients(name, "1", monkeypatch)


@pytest.mark.parametrize("kind,N,counts,scale,nmp", [("pair", 5, (5, 3, 2, 1), None, 1), ("hyper", 7, (7, 4, 3, 2, 1), 3, 1),
                                                     ("hyper", 6, (6, 4, 2, 1), 3, 2)])
def test_ragged_module_gradients_meet_the_gates(kind, N, counts, scale, nmp):
    """tests/test_ragged_backward_gpu.py's per-scene oracle and gates, both opt-ins on."""
    TRB._module_case(kind, N, counts, scale, nmp, 30 if kind == "pair" else 40)


def _block_gradients(case, ragged):
    """A MultiScaleHGNN of the case's scales against the per-scene float64 oracle (as
    tests/test_ragged_backward_gpu.py:233's block test): dL/df and every used parameter at TOL_CLEAN where every scene is
    clean, else TOL_ANY; forward within FORWARD_ABS."""
    B, N, counts, scales = case["B"], case["N"], case["counts"], case["scales"]
    blk, sp, shs = C.cpu_block(case)
    h, U = C.inputs(case)
    if ragged:
        h = C.with_garbage(case, h)
    S = len(scales)
    g = torch.Generator().manual_seed(6)
    Rm = torch.randn(B, N, 64 * (1 + S), generator=g)
    refs = []
    for i, (state, s) in enumerate(zip([sp, *shs], [None, *scales])):
        E = N * N if s is None else (1 if s == N else N)
        K = C.K_PAIR if s is None else C.K_HYPER
        refs.append(RB.module_oracle(state, s is None, s, case, h, U[i], Rm[..., 64 * i:64 * (i + 1)], torch.zeros(B, E, K)))
    g_f = sum(r["g_h"] for r in refs)
    clean = torch.stack([r["clean"] for r in refs]).all(dim=0)
    blk.to(dev()).train()
    x = h.to(dev()).requires_grad_(True)
    noise = [[u.to(dev()) for u in Um] for Um in U]
    final, _ = blk(x, noise_u=noise, **(dict(n_agents=counts) if ragged else {}))
    want = torch.cat([r["node_feat"] for r in refs], dim=-1)
    assert float((final[..., 64:].detach().double().cpu() - want).abs().max()) <= D.FORWARD_ABS
    (final[..., 64:] * Rm.to(dev())).sum().backward()
    tol = D.TOL_CLEAN if bool(clean.all()) else D.TOL_ANY
    eh = float((x.grad.double().cpu() - g_f).abs().max()) / float(g_f.abs().max())
    assert eh <= tol, ("dL/df", eh, tol)
    worst = []
    for prefix, r in zip(["interaction."] + [f"interaction_hyper.{i}." for i in range(S)], refs):
        used = [k for k, v in r["grads"].items() if v is not None and float(v.abs().max()) > 0]
        hip = {k[len(prefix):]: p.grad for k, p in blk.named_parameters() if k.startswith(prefix)}
        worst.append(TB._check(hip, r["grads"], used, tol))
    print(f"\ndeterministic block {case['id']} ragged={ragged}: dL/df {eh:.1e}, worst per module {worst}; "
          f"{int(clean.sum())}/{B} scenes clean, gate {tol:g}")


def test_block_gradients_meet_the_gates():
    _block_gradients(RB.settled_case(11, (11, 11, 11), [2, 5, 11], seed=11), ragged=False)     # MultiScaleHGNN([2, 5, 11])
    _block_gradients(C.BY_ID["n7"], ragged=True)


# ---- 5. modules: repeatability ----------------------------------------------------------------------------------------
def _grads_twice(loss_of, params, x):
    """Two forward + backward passes from the same state -> per pass [dL/dx, every parameter gradient]."""
    out = []
    for _ in range(2):
        for p in params:
            p.grad = None
        x.grad = None
        loss_of(x).backward()
        out.append([x.grad.clone()] + [p.grad.clone() for p in params if p.grad is not None])
    torch.cuda.synchronize()
    return out


def _assert_repeat(tag, a, b, min_grads):
    assert len(a) == len(b) >= min_grads, (tag, len(a))
    for i, (u, v) in enumerate(zip(a, b)):
        assert bool(torch.isfinite(u).all()) and bool(u.any()), (tag, i)
        assert torch.equal(u, v), (tag, i, float((u - v).abs().max()))


@pytest.mark.parametrize("what", ["block", "nmp2", "ragged", "agent_subset"])
def test_two_backward_passes_are_bit_equal(what):
    import groupnet_amd as G
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(21)
    B, N, nmp = 6, 11, 2 if what == "nmp2" else 1
    blk = MultiScaleHGNN([2, 5, 11], nmp_layers=nmp).to(dev()).train()
    f = torch.randn(B, N, 64, device=dev())
    Rm = torch.randn(B, N, blk.out_features, device=dev())
    noise = [[torch.rand(s, device=dev()) for _ in range(nmp)] for s in blk.noise_shapes(B, N)]
    kw = {}
    if what == "ragged":
        kw = dict(n_agents=[11, 7, 1, 4, 11, 2])
    elif what == "agent_subset":        # a host mask with holes ("Agents missing anywhere")
        mask = torch.ones(B, N, dtype=torch.bool)
        mask[1, 3], mask[2, :5], mask[4, 10], mask[5, ::2] = False, False, False, False
        kw = dict(n_agents=G.agent_subset(mask, dev()))
    a, b = _grads_twice(lambda x: (blk(x, noise_u=noise, **kw)[0] * Rm).sum(), list(blk.parameters()),
                        f.clone().requires_grad_(True))
    _assert_repeat(what, a, b, 100)


def test_graphed_train_step_equals_its_eager_twin_bit_for_bit():
    """The twin of tests/test_backward_gpu.py:219 — same weights, same seed, SGD — captured and run with the mode on, three
    steps: the loss bit-equal and every updated weight `torch.equal` after every step (with the mode off the weights agree
    to fp32 rounding only).  Replay k draws from Philox position k * draws_per_step: the twin's counter is set there."""
    import groupnet_amd as G
    from groupnet_amd.graphs import GraphedTrainStep
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(3)
    B, N = 16, 11
    blk = MultiScaleHGNN([2, 5, 11]).to(dev()).train()
    ref = copy.deepcopy(blk)
    f = torch.randn(B, N, 64, device=dev())
    tgt = torch.randn(B, N, blk.out_features, device=dev())
    loss_fn = lambda out, H, t: ((out - t) ** 2).mean()
    step = GraphedTrainStep(blk, torch.optim.SGD(blk.parameters(), lr=0.05), loss_fn, B, N,
                            target_shapes=[tuple(tgt.shape)], seed=11, warmup=2)
    blk.load_state_dict(ref.state_dict())       # the warm-up steps trained `blk`: restart both from the same weights
    G.MS_HGNN_batch.invalidate_weight_caches(blk)
    opt = torch.optim.SGD(ref.parameters(), lr=0.05)
    counter = torch.zeros(1, dtype=torch.int64, device=dev())
    losses = []
    for k in range(3):
        lg = float(step(f, tgt))
        counter.fill_(k * step.draws_per_step)
        G.set_noise_mode("device", seed=11, offset=0, counter=counter)
        try:
            opt.zero_grad()
            out, _ = ref(f)
            loss = loss_fn(out, None, tgt)
            loss.backward()
            opt.step()
        finally:
            G.set_noise_mode("host")
        assert float(loss.detach()) == lg, (k, float(loss.detach()), lg)
        for (n1, p1), (_, p2) in zip(blk.named_parameters(), ref.named_parameters()):
            assert torch.equal(p1, p2), (k, n1, float((p1 - p2).abs().max()))
        losses.append(lg)
    assert losses[2] < losses[0] and len(set(losses)) == 3


def test_past_encoder_training_step_repeats():
    """One `PastEncoder` training step on the reference's training-mode case (dropout probability 0, the host noise seeded
    per pass): the dense layers around the modules go through `GemmBatch` and follow the mode."""
    import types
    from groupnet_amd.past_encoder import PastEncoder
    with np.load(os.path.join(os.path.dirname(__file__), "golden", "past_encoder_train_s5_11_b6.npz")) as z:
        c = {k: z[k].copy() for k in z.files}
    sd = {k[3:]: torch.from_numpy(v) for k, v in c.items() if k.startswith("sd/")}
    B, scales = int(c["B"]), [int(s) for s in c["scales"]]
    enc = PastEncoder(types.SimpleNamespace(hidden_dim=64, hyper_scales=scales, past_length=5))
    enc.load_state_dict(sd, strict=True)
    enc.to(dev()).train()
    enc.pos_encoder.dropout.p = 0.0
    x0 = torch.from_numpy(c["x"]).to(dev())
    Rm = torch.randn(torch.Size(c["output_feature"].shape), generator=torch.Generator().manual_seed(2)).to(dev())

    def loss_of(x):
        torch.manual_seed(int(c["seed"]))
        out, _ = enc(x, B, 11)
        return (out * Rm).sum()
    a, b = _grads_twice(loss_of, list(enc.parameters()), x0.clone().requires_grad_(True))
    _assert_repeat("past encoder", a, b, 100)


def test_dense_and_mask_incidence_forms_give_the_same_gradients():
    """16 < N <= 64: the dense and the bit-mask form of the incidence differ, as stated, only in the order of the atomics of
    the backward — so with the mode on their gradients are the same bits."""
    from groupnet_amd import ops
    from oracle import ms_hgnn_oracle as O
    B, N, scale = 3, 20, 2
    _, hyper = TB._modules(100 + N, 1)
    hyper.scale = scale
    hyper.to(dev()).train()
    g = torch.Generator().manual_seed(N)
    h = torch.randn(B, N, 64, generator=g)
    corr = O.affinity(h).to(dev())
    U = [torch.rand(s, generator=g).to(dev()) for s in O.noise_shapes(B, N, scale, 1)]
    R1, R2 = torch.randn(B, N, 64, generator=g).to(dev()), torch.randn(B, N, hyper.edge_types, generator=g).to(dev())

    def loss_of(x):
        nf, fac, _ = hyper(x, corr, noise_u=U)
        return (nf * R1).sum() + (fac * R2).sum()
    got = {}
    try:
        for form in ("dense", "mask"):
            ops.set_incidence_form(form)
            got[form] = _grads_twice(loss_of, list(hyper.parameters()), h.to(dev()).requires_grad_(True))[0]
    finally:
        ops.set_incidence_form(None)
    _assert_repeat("dense vs mask", got["dense"], got["mask"], 40)
