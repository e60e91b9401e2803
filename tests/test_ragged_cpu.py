"""Ragged batches ("Ragged batches") without a device: the route a ragged forward takes, the plan
queries of every ragged entry point, the validated holder of the counts, and the test suite's own per-scene oracle
(tests/ragged_cases.py), which tests/test_ragged_gpu.py holds the kernels against."""
import ctypes

import pytest
import torch

import ragged_cases as C
from oracle import ms_hgnn_oracle as O

P = 4096            # an aligned non-NULL "device address": a plan query tests addresses, it never reads through them


def lib():
    from groupnet_amd import _lib
    return _lib, _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# the route
# ---------------------------------------------------------------------------------------------------------------------
def _route(N, twin, matrix16=True, **kw):
    from groupnet_amd import route as R
    knobs = R.Knobs(True, R.POOL_KERNEL_MAX_N, True, True)
    mods = ((True, C.K_PAIR), (False, C.K_HYPER), (False, C.K_HYPER))
    return R.message_passing_route(N, mods, twin=twin, training=False, matrix16=matrix16, knobs=knobs,
                                   closing_asked=True, **kw)


@pytest.mark.parametrize("twin", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [11, 16, 17, 50, 65])
def test_ragged_route_table(N, twin):
    """Every module pools in the node->edge launch and closes through the scatter launch; the pairwise module takes the
    pair form (fp32 storage, never the node form) or the twins' per-pair gather (never the scene form); hyper modules
    keep the fused gather / the gather launch by N; no masks, no closing stage asked."""
    from groupnet_amd import route as R
    rt = _route(N, twin, ragged=True)
    pair, hyper = rt.modules[0], rt.modules[1:]
    assert all(not m.pool_in_edge_kernel and not m.node_form and m.closing_input == R.SCATTER for m in rt.modules)
    assert pair.source == (R.TWIN_PAIR if twin else R.PAIR) and pair.first_layer == (not twin)
    assert all(m.source == (R.FUSED_GATHER if N <= 16 else R.EO) and not m.first_layer for m in hyper)
    assert rt.node2edge == (0, 1, 2) and rt.scatter == (0, 1, 2)
    assert rt.gather == (() if N <= 16 else (1, 2))
    assert rt.masks is False and rt.ask_closing is False


@pytest.mark.parametrize("twin", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N", [11, 16, 17, 50, 65])
def test_ragged_false_is_the_call_without_the_argument(N, twin):
    for matrix16 in (True, False):
        assert _route(N, twin, matrix16, ragged=False) == _route(N, twin, matrix16)


def test_ragged_route_is_keyword_only_and_inference_only():
    from groupnet_amd import route as R
    knobs = R.Knobs(True, 16, True, False)
    with pytest.raises(TypeError):
        R.message_passing_route(11, ((True, 6),), False, False, True, knobs, True, True)
    with pytest.raises(NotImplementedError):
        R.message_passing_route(11, ((True, 6),), twin=False, training=True, matrix16=True, knobs=knobs,
                                closing_asked=False, ragged=True)


# ---------------------------------------------------------------------------------------------------------------------
# plan queries
# ---------------------------------------------------------------------------------------------------------------------
def _scales(n=2):
    return (ctypes.c_void_p * n)(*[P] * n), (ctypes.c_int * n)(*[2] * n)


@pytest.mark.parametrize("stem", ["f32", "bf16"])
def test_affinity_topk_ragged_plan(stem):
    L, lb = lib()
    fn = getattr(lb, "gn_affinity_topk_ragged_plan_" + stem)
    Hl, kl = _scales()
    plan = L.LaunchPlan()
    q = lambda N=11, ex=None, counts=P: fn(P, None, Hl, kl, 2, 5, N, 64, ex, counts, ctypes.byref(plan))
    assert q(counts=None) == L.GN_ERR_NULL
    assert q(counts=P + 2) == L.GN_ERR_ALIGN
    ex = L.BlockExtras(x_raw=P, x_dim=20, M=P, c=P, f_contig=P)
    assert q(ex=ctypes.byref(ex)) == L.GN_ERR_SHAPE                 # the embedding front-end has no ragged form
    assert q(N=113) == L.GN_ERR_LDS                                  # beyond the fused tile: affinity + the banded top-k
    assert q(N=112) == L.GN_OK
    assert q() == L.GN_OK
    assert lb.gn_kernel_name(plan.kernel) == b"affinity_topk_ragged_kernel" and plan.kernel == L.K_AFFINITY_TOPK_RAGGED
    assert list(plan.grid) == [5, 1, 1] and plan.precision == (stem == "bf16")
    # the tile is the full-batch launch's
    full = L.LaunchPlan()
    assert getattr(lb, "gn_affinity_topk_plan_" + stem)(P, None, Hl, kl, 2, 5, 11, 64, None, None, None,
                                                         ctypes.byref(full)) == L.GN_OK
    assert plan.dyn_lds == full.dyn_lds
    assert fn(P, None, Hl, kl, 2, 5, 11, 64, None, P, None) == L.GN_ERR_NULL


def test_topk_incidence_ragged_plan():
    L, lb = lib()
    Hl, kl = _scales()
    plan, full = L.LaunchPlan(), L.LaunchPlan()
    q = lambda counts=P, N=113: lb.gn_topk_incidence_ragged_plan_f32(P, Hl, kl, 2, 2, N, counts, ctypes.byref(plan))
    assert q(counts=None) == L.GN_ERR_NULL
    assert q(counts=P + 1) == L.GN_ERR_ALIGN
    assert q(N=1) == -3                                              # k > N, as the full-batch launch
    assert q() == L.GN_OK
    assert lb.gn_kernel_name(plan.kernel) == b"topk_incidence_ragged_kernel"
    assert lb.gn_topk_incidence_plan_f32(P, Hl, kl, 2, 2, 113, ctypes.byref(full)) == L.GN_OK
    assert (list(plan.grid), plan.TE, plan.dyn_lds) == (list(full.grid), full.TE, full.dyn_lds)


@pytest.mark.parametrize("stem", ["f32", "bf16"])
def test_node2edge_ragged_plan(stem, monkeypatch):
    L, lb = lib()
    fn = getattr(lb, "gn_node2edge_ragged_plan_" + stem)
    N, B = 17, 5
    g = (L.N2EGroup * 3)(L.N2EGroup(xp=P, pq=P, w2=P, edges=P, b2=P, E=N * (N + 1) // 2, sym=1),
                         L.N2EGroup(xp=P, pq=P, H=P, w2=P, edges=P, b2=P, E=N),
                         L.N2EGroup(xp=P, pq=P, H=P, w2=P, edges=P, b2=P, E=1))
    plan, full = L.LaunchPlan(), L.LaunchPlan()
    assert fn(g, 3, B, N, None, ctypes.byref(plan)) == L.GN_ERR_NULL
    assert fn(g, 3, B, N, P + 2, ctypes.byref(plan)) == L.GN_ERR_ALIGN
    assert fn(g, 3, B, N, P, None) == L.GN_ERR_NULL
    for rows in ("0", "1"):
        monkeypatch.setenv("GN_N2E_ROWS", rows)
        assert fn(g, 3, B, N, P, ctypes.byref(plan)) == L.GN_OK
        assert lb.gn_kernel_name(plan.kernel) == b"node2edge_ragged_kernel" and plan.variant == int(rows)
        assert getattr(lb, "gn_node2edge_plan_" + stem)(g, 3, B, N, ctypes.byref(full)) == L.GN_OK
        full.kernel = plan.kernel
        assert bytes(plan) == bytes(full)                            # the work shape is the full-batch launch's
    g[0].E = 7
    assert fn(g, 3, B, N, P, ctypes.byref(plan)) == L.GN_ERR_SHAPE


@pytest.mark.parametrize("stem", ["f32", "bf16"])
def test_agg_scatter_ragged_plan(stem):
    L, lb = lib()
    fn = getattr(lb, "gn_agg_scatter_ragged_plan_" + stem)
    N, B = 17, 5
    g = (L.ScatterGroup * 3)(L.ScatterGroup(feat=P, ori=P, out=P, E=N * (N + 1) // 2, sym=1),
                             L.ScatterGroup(feat=P, ori=P, out=P, E=N * N),
                             L.ScatterGroup(feat=P, H=P, ori=P, out=P, E=N))
    plan = L.LaunchPlan()
    assert fn(g, 3, B, N, 0.0, None, ctypes.byref(plan)) == L.GN_ERR_NULL
    assert fn(g, 3, B, N, 0.0, P + 2, ctypes.byref(plan)) == L.GN_ERR_ALIGN
    assert fn(g, 3, B, N, -1.0, P, ctypes.byref(plan)) == L.GN_ERR_SHAPE
    for divisor in (0.0, 1.0):                                       # 0: each scene by its own count
        assert fn(g, 3, B, N, divisor, P, ctypes.byref(plan)) == L.GN_OK
        assert lb.gn_kernel_name(plan.kernel) == b"agg_scatter_ragged_kernel"
        assert list(plan.grid) == [(B * N * 32 + 255) // 256, 3, 1] and list(plan.pos)[:3] == [0, 1, 2]
    g[2].colmask = P
    assert fn(g, 3, B, N, 0.0, P, ctypes.byref(plan)) == L.GN_ERR_SHAPE      # dense H only
    g[2].colmask, g[2].out = None, None
    assert fn(g, 3, B, N, 0.0, P, ctypes.byref(plan)) == L.GN_ERR_NULL


def test_zero_padding_plan():
    L, lb = lib()
    N, B = 17, 5
    it = (L.ZeroItem * 3)(L.ZeroItem(ptr=P, pitch=4 * 64 * 5, width=4 * 64, kind=L.ZERO_NODE_ROWS),
                          L.ZeroItem(ptr=P, pitch=2 * 10, width=2 * 10, kind=L.ZERO_EDGE_ROWS),
                          L.ZeroItem(ptr=P, pitch=4 * 6, width=4 * 6, kind=L.ZERO_PAIR_ROWS))
    plan = L.LaunchPlan()
    q = lambda n=3, counts=P: lb.gn_zero_padding_plan(it, n, B, N, counts, ctypes.byref(plan))
    assert q(counts=None) == L.GN_ERR_NULL
    assert q(counts=P + 2) == L.GN_ERR_ALIGN
    assert q(n=0) == L.GN_ERR_SHAPE and q(n=L.MAX_ZERO_ITEMS + 1) == L.GN_ERR_SHAPE
    assert q() == L.GN_OK
    assert lb.gn_kernel_name(plan.kernel) == b"zero_padding_kernel" and plan.kernel == L.K_LAST
    assert plan.grid[1] == 3 and plan.grid[0] == (B * N * N * 6 + 1023) // 1024
    it[1].width = it[1].pitch = 2 * 5                                # a bf16 row of 5 types: written as 2-byte words
    assert q() == L.GN_OK
    it[1].width = 9                                                  # ... but never as bytes
    assert q() == L.GN_ERR_ALIGN
    it[1].width, it[1].pitch = 20, 16
    assert q() == L.GN_ERR_SHAPE
    it[1].pitch, it[1].kind = 20, 3
    assert q() == L.GN_ERR_SHAPE
    it[1].kind, it[1].ptr = 1, None
    assert q() == L.GN_ERR_NULL
    assert lb.gn_kernel_name(L.K_LAST + 1) is None


def _fields_but_kernel(plan):
    L, _ = lib()
    vals = {name: getattr(plan, name) for name, _ in L.LaunchPlan._fields_ if name != "kernel"}
    return {name: list(v) if isinstance(v, ctypes.Array) else v for name, v in vals.items()}


@pytest.mark.parametrize("stem", ["f32", "bf16"])
def test_ragged_plan_is_the_plain_plan_but_for_the_kernel(stem, monkeypatch):
    """One plan function per stage decides the plain and the ragged launch: for the same arguments the two plans agree in
    EVERY field except ``kernel``, which names the ragged kernel and its plain twin.  gn_topk_incidence (fp32 only: it
    ranks corr) on either side of one band, gn_affinity_topk at both ends of its tile, gn_node2edge in its banded form
    (by switch at N <= 64, by size beyond) and its row form.  Placeholder addresses: nothing is launched."""
    L, lb = lib()
    Hl, kl = _scales()
    plan, full = L.LaunchPlan(), L.LaunchPlan()

    def same(kernel, twin):
        assert lb.gn_kernel_name(plan.kernel) == kernel and lb.gn_kernel_name(full.kernel) == twin
        assert _fields_but_kernel(plan) == _fields_but_kernel(full)

    for B, N in ((2, 11), (1030, 11), (2, 113), (3, 400)):
        assert lb.gn_topk_incidence_ragged_plan_f32(P, Hl, kl, 2, B, N, P, ctypes.byref(plan)) == L.GN_OK
        assert lb.gn_topk_incidence_plan_f32(P, Hl, kl, 2, B, N, ctypes.byref(full)) == L.GN_OK
        same(b"topk_incidence_ragged_kernel", b"topk_incidence_kernel")
    for B, N, D in ((5, 11, 64), (1, 2, 4), (3, 112, 64)):
        assert getattr(lb, "gn_affinity_topk_ragged_plan_" + stem)(P, None, Hl, kl, 2, B, N, D, None, P,
                                                                   ctypes.byref(plan)) == L.GN_OK
        assert getattr(lb, "gn_affinity_topk_plan_" + stem)(P, None, Hl, kl, 2, B, N, D, None, None, None,
                                                            ctypes.byref(full)) == L.GN_OK
        same(b"affinity_topk_ragged_kernel", b"affinity_topk_kernel")
    for B, N, rows in ((5, 17, "0"), (5, 17, "1"), (300, 50, None), (2, 65, None), (2, 65, "1")):
        if rows is None:
            monkeypatch.delenv("GN_N2E_ROWS", raising=False)
        else:
            monkeypatch.setenv("GN_N2E_ROWS", rows)
        g = (L.N2EGroup * 3)(L.N2EGroup(xp=P, pq=P, w2=P, edges=P, b2=P, E=N * N),
                             L.N2EGroup(xp=P, pq=P, H=P, w2=P, edges=P, b2=P, E=N),
                             L.N2EGroup(xp=P, pq=P, H=P, w2=P, edges=P, b2=P, E=1))
        assert getattr(lb, "gn_node2edge_ragged_plan_" + stem)(g, 3, B, N, P, ctypes.byref(plan)) == L.GN_OK
        assert getattr(lb, "gn_node2edge_plan_" + stem)(g, 3, B, N, ctypes.byref(full)) == L.GN_OK
        same(b"node2edge_ragged_kernel", b"node2edge_kernel")
        assert plan.variant == (1 if N <= 64 and rows != "0" else 0)      # both forms were planned


# ---------------------------------------------------------------------------------------------------------------------
# the holder of the counts
# ---------------------------------------------------------------------------------------------------------------------
def test_agent_counts_refusals_and_the_all_n_rule():
    from groupnet_amd import ops
    dev = torch.device("cpu")       # (nothing below reaches the upload)
    assert ops.agent_counts(None, 3, 7, dev) is None
    assert ops.agent_counts([7, 7, 7], 3, 7, dev) is None                    # no scene is padded: today's path
    assert ops.agent_counts(torch.tensor([7, 7, 7]), 3, 7, dev) is None
    assert ops.agent_counts(torch.tensor([7, 7, 7], dtype=torch.int32), 3, 7, dev) is None
    for bad in ([7, 7], [7, 7, 7, 7], [0, 7, 7], [7, 8, 7], [7, -1, 7], [7.0, 7, 7], [True, 7, 7], 5,
                torch.tensor([7.0, 7.0, 7.0]), torch.tensor([[7, 7, 7]]), torch.tensor([7, 7])):
        with pytest.raises(ValueError):
            ops.agent_counts(bad, 3, 7, dev)
    with pytest.raises(ValueError, match="GPU"):                             # a padded batch has no CPU path either
        ops.agent_counts([7, 3, 7], 3, 7, dev)
    held = ops.AgentCounts((7, 3, 7), 7, "cuda:0")                           # (validated; uploaded by the first launch)
    assert held._dev is None
    assert ops.agent_counts(held, 3, 7, dev) is held
    with pytest.raises(ValueError):
        ops.agent_counts(held, 3, 8, dev)
    with pytest.raises(ValueError):
        ops.agent_counts(held, 4, 7, dev)


def test_forwards_take_the_counts_last():
    import inspect
    import groupnet_amd as G
    from groupnet_amd import MS_HGNN_batch as M, ops
    from groupnet_amd.multiscale import MultiScaleHGNN
    for fn in (G.MS_HGNN_oridinary.forward, G.MS_HGNN_hyper.forward, MultiScaleHGNN.forward, M.run_message_passing,
               ops.topk_incidence, ops.node2edge_grouped, ops.node2edge, ops.agg_scatter_grouped, ops.agg_scatter,
               ops.affinity_topk, ops.AffinityTail.__init__):
        ps = list(inspect.signature(fn).parameters.values())
        assert ps[-1].name == "n_agents" and ps[-1].default is None, fn


# ---------------------------------------------------------------------------------------------------------------------
# the suite's own oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_case_table():
    assert [(c["N"], c["counts"], c["scales"], c["seed"]) for c in C.CASES] == [
        (7, [1, 2, 3, 5, 6, 7], [2, 5, 7], 0), (17, [17, 3, 16, 9, 1], [2, 5, 17], 3),
        (50, [50, 23, 5], [2, 4, 8, 16], 5), (113, [113, 40], [2, 8, 113], 5)]
    for c in C.CASES:
        assert all(1 <= n <= c["N"] for n in c["counts"]) and max(c["counts"]) == c["N"] and min(c["counts"]) < c["N"]


@pytest.mark.parametrize("case", C.CASES, ids=[c["id"] for c in C.CASES])
def test_cases_keep_their_selections_apart(case):
    """The condition on the inputs: no valid row of any top-k scale has its k-th and (k+1)-th affinity closer than
    MIN_GAP = 2e-5, for the fp32 inputs and for their bf16 roundings (a change of generator shows up here)."""
    for bf16 in (False, True):
        h, _ = C.inputs(case, bf16=bf16)
        gap = C.min_gap(case, h)
        print(f"{case['id']} {'bf16' if bf16 else 'fp32'}: smallest gap {gap:.2e}")
        assert gap >= C.MIN_GAP, (case["id"], bf16, gap)


def test_padded_incidence_follows_the_contract():
    case = C.BY_ID["n7"]
    h, _ = C.inputs(case)
    for s in case["scales"]:
        H = C.padded_incidence(case, h, s)
        for b, n in enumerate(case["counts"]):
            assert not H[b, :, n:].any() and (s == 7 or not H[b, n:].any())
            if s == 7:
                assert H.shape[1] == 1 and bool((H[b, 0, :n] == 1).all())
            else:
                assert bool((H[b, :n].sum(-1) == min(s, n)).all())
                if n > s:                                            # the reference's own graph of that scene
                    assert torch.equal(H[b, :n, :n], O.topk_incidence(C.scene_corr(h, b, n), s)[0])


@pytest.mark.parametrize("nmp", [1, 2])
def test_per_scene_oracle_is_the_batch_oracle_when_nothing_is_padded(nmp):
    """The oracle's plumbing (noise gathered at padded indices, incidences, module order): with every count equal to N
    it is `ms_hgnn_multiscale_forward` on the whole batch, to float64 rounding."""
    from launch_forms import state64
    case = dict(C.BY_ID["n7"], counts=[7] * 6)
    _, sp, shs = C.cpu_block(case, nmp)
    h, U = C.inputs(case, nmp)
    with torch.no_grad():
        ref, Href, _ = O.ms_hgnn_multiscale_forward(state64(sp), [state64(s) for s in shs], case["scales"], h.double(),
                                                    [u.double() for u in U[0]], [[u.double() for u in us] for us in U[1:]],
                                                    decomposed=True, nmp_layers=nmp)
    for b in range(case["B"]):
        feats, facs, Hs = C.scene_oracle(sp, shs, case, h, U, b, nmp)
        got = torch.cat(feats, dim=-1)
        assert float((got - ref[b, :, 64:]).abs().max()) <= 1e-12
        assert torch.equal(torch.cat([H[0] for H in Hs]).double(), Href[b])
        assert all(bool(torch.isfinite(f).all()) for f in facs)


def test_per_scene_oracle_is_finite_at_every_count():
    case = C.BY_ID["n7"]
    h, U, sp, shs, per_scene = C.block_oracle("n7")
    for b, (feats, facs, Hs) in enumerate(per_scene):
        n = case["counts"][b]
        assert all(f.shape == (n, 64) and bool(torch.isfinite(f).all()) for f in feats)
        assert facs[0].shape == (n * n, C.K_PAIR) and all(bool(torch.isfinite(f).all()) for f in facs)
