"""The deterministic training mode without a GPU: the plan query of the ordered split-K GEMM (pure host arithmetic), the
switch and the route keyword, the refusals of the two new entry points before any launch, and — with a recording stub in
place of the library — which entry points a whole `backward.round_backward` issues with the mode on and off."""
import contextlib
import ctypes
import types

import pytest
import torch

import backward_kernel_refs as R
import deterministic_cases as D


def _lib():
    from groupnet_amd import _lib as L
    return L, L.load()


def _descs(cases, keep):
    """The descriptors `backward.GemmBatch.add` builds for the cases on CPU tensors (the plan query reads addresses and
    shapes only).  keep: holds the tensors."""
    from groupnet_amd.backward import GemmBatch
    gb = GemmBatch()
    for c in cases:
        o = D.operands(c)
        keep.append(o)
        D.add(gb, c, o)
    return gb.descs


def _plan(descs):
    L, lib = _lib()
    arr = (L.GemmDesc * len(descs))(*descs)
    plan = L.GemmDetPlan()
    return lib.gn_gemm_grouped_det_plan(arr, len(descs), plan), plan


def _regions(cases, plan):
    """(offset, bytes) of every workspace region of the plan."""
    out = []
    for i, c in enumerate(cases):
        if not c.accum:
            assert plan.offset[i] == plan.cs_offset[i] == -1 and plan.chain[i] == plan.cs_chain[i] == -1
            continue
        out.append((plan.offset[i], 4 * plan.splits[i] * c.M * c.N))
        assert (plan.cs_offset[i] >= 0) == c.colsum and (plan.cs_chain[i] >= 0) == c.colsum
        if c.colsum:
            out.append((plan.cs_offset[i], 4 * plan.splits[i] * c.M))
    return out


def test_gates_are_the_owners():
    import ragged_backward_cases as RB
    import test_backward_gpu as TB
    from groupnet_amd import route
    assert (D.TOL_CLEAN, D.TOL_ANY) == (TB.TOL_CLEAN, TB.TOL_ANY)
    assert D.N2E_MAX_N == route.N2E_BWD_SCENE_MAX_N == RB.LDS_LIMIT_N


def test_plan_states_the_split_rule_and_disjoint_regions():
    L, _ = _lib()
    mixed = [c for pair in zip(R.GEMM_BATCH, R.GEMM_ACCUM + D.ORDER_CASES) for c in pair] + R.GEMM_BATCH[11:]
    for cases in (R.GEMM_ACCUM, D.ORDER_CASES, mixed):
        keep = []
        rc, plan = _plan(_descs(cases, keep))
        assert rc == L.GN_OK and plan.n == len(cases)
        for i, c in enumerate(cases):
            assert (plan.splits[i], plan.kchunk[i]) == D.split_rule(c.M, c.N, c.K, c.accum), c.name
            assert plan.splits[i] == R.gemm_splits(c.M, c.N, c.K, c.accum), c.name      # the atomic form's rule
            assert plan.kernel[i] == (L.GEMM_KERNEL_VECTOR if R.gemm_vec(c) else L.GEMM_KERNEL_SCALAR), c.name
            assert plan.chain[i] == (i if c.accum else -1), c.name                       # every destination its own
        regions = sorted(_regions(cases, plan))
        assert len(regions) == sum(c.accum + (c.accum and c.colsum) for c in cases)
        for (o0, n0), (o1, _) in zip(regions, regions[1:]):
            assert o0 % 16 == 0 and o0 + n0 <= o1
        assert regions[-1][0] + regions[-1][1] <= plan.workspace_bytes
        assert plan.n_chains == sum(c.accum for c in cases)
    assert [D.split_rule(c.M, c.N, c.K, True) for c in D.ORDER_CASES] == [(33, 256), (3, 256), (9, 256)]


def test_a_plan_entry_is_the_same_alone_and_at_any_position():
    keep = []
    others = _descs(R.GEMM_ACCUM + R.GEMM_BATCH[:12], keep)
    for c in D.ORDER_CASES + R.GEMM_ACCUM[:3]:
        mine = _descs([c], keep)
        rc, alone = _plan(mine)
        assert rc == 0
        for pos in (0, 3, len(others)):
            rc, plan = _plan(others[:pos] + mine + others[pos:])
            assert rc == 0
            assert (plan.splits[pos], plan.kchunk[pos], plan.kernel[pos]) == (alone.splits[0], alone.kchunk[0], alone.kernel[0])
            assert plan.chain[pos] == pos and (plan.cs_chain[pos] == pos) == c.colsum


def test_slices_of_the_order_cases_run_as_one_split_on_the_same_kernel():
    """What the GPU order check rests on (deterministic_cases' docstring), asserted through the plan query."""
    from groupnet_amd.backward import GemmBatch
    for c in D.ORDER_CASES + [D.CHAIN_SECOND]:
        o = D.operands(c)
        rc, whole = _plan(_descs([c], [o]))
        assert rc == 0 and whole.kernel[0] == 1 and whole.splits[0] > 1
        slices = D.k_slices(c, o)
        assert len(slices) == whole.splits[0] and sum(s["K"] for s in slices) == c.K
        gb = GemmBatch()
        for s in slices:
            assert s["K"] % 32 == 0 and s["K"] <= whole.kchunk[0]
            if c.tC:        # the ordered entry itself on the slice, onto a zeroed destination
                gb.add(s["A"], s["B"], torch.zeros(c.N, c.M), tA=c.tA, tB=c.tB, rs=s["rs"], accum=True, tC=True)
            else:           # a plain problem
                gb.add(s["A"], s["B"], torch.zeros(c.M, c.N), tA=c.tA, tB=c.tB, rs=s["rs"],
                       colsum=torch.zeros(c.M) if c.colsum else None)
        rc, plan = _plan(gb.descs)
        assert rc == 0
        assert all(plan.splits[i] == 1 and plan.kernel[i] == whole.kernel[0] for i in range(len(slices))), c.name


def test_identical_destinations_chain_and_partial_overlaps_are_refused():
    from groupnet_amd.backward import GemmBatch
    L, _ = _lib()
    g = torch.Generator().manual_seed(1)
    Rn = lambda *s: torch.randn(*s, generator=g)
    dY, X, dY2, X2 = Rn(512, 96), Rn(512, 64), Rn(288, 96), Rn(288, 64)
    W, b, other = torch.zeros(96, 136), torch.zeros(96), torch.zeros(96, 64)

    def batch(*dst):
        gb = GemmBatch()
        for (A, Bm), (C, cs) in zip(((dY, X), (dY2, X2), (dY, X2[:, :64].repeat(2, 1)[:512])), dst):
            gb.add(A, Bm, C, tA=True, accum=True, colsum=cs)
        return _plan(gb.descs)

    # the same C and the same colsum twice, a third problem elsewhere sharing only the colsum
    rc, plan = batch((W[:, :64], b), (W[:, :64], b), (other, b))
    assert rc == 0 and list(plan.chain[:3]) == [0, 0, 2] and list(plan.cs_chain[:3]) == [0, 0, 0] and plan.n_chains == 2
    # column slices of one matrix interleave without sharing an element
    rc, plan = batch((W[:, :64], b), (W[:, 64:128], None), (other, None))
    assert rc == 0 and list(plan.chain[:3]) == [0, 1, 2]
    # shifted by 8 columns, by one row, a colsum shifted by one, a colsum inside a C: refused
    assert batch((W[:, :64], None), (W[:, 8:72], None), (other, None))[0] == L.GN_ERR_SHAPE
    big = torch.zeros(97, 64)
    assert batch((big[:96], None), (big[1:], None), (other, None))[0] == L.GN_ERR_SHAPE
    bb = torch.zeros(97)
    assert batch((W[:, :64], bb[:96]), (other, bb[1:]), (big[:96], None))[0] == L.GN_ERR_SHAPE
    assert batch((other, other.view(-1)[:96]), (W[:, :64], None), (big[:96], None))[0] == L.GN_ERR_SHAPE
    # the same address with another shape is not the same destination
    gb = GemmBatch()
    gb.add(dY, X, other, tA=True, accum=True)
    gb.add(dY[:, :64], X, other[:64], tA=True, accum=True)
    assert _plan(gb.descs)[0] == L.GN_ERR_SHAPE


def test_entry_points_refuse_before_any_launch():
    """Validation is host code: the error codes without a GPU (a GN_OK here would have launched)."""
    L, lib = _lib()
    P = ctypes.c_void_p
    keep = []
    descs = _descs(R.GEMM_ACCUM[:2], keep)
    arr = (L.GemmDesc * 2)(*descs)
    rc, plan = _plan(descs)
    need = plan.workspace_bytes
    assert rc == 0 and need > 0
    assert lib.gn_gemm_grouped_det_f32(arr, 2, None, need, P(0)) == L.GN_ERR_NULL
    assert lib.gn_gemm_grouped_det_f32(arr, 2, P(4096 + 4), need, P(0)) == L.GN_ERR_ALIGN
    assert lib.gn_gemm_grouped_det_f32(arr, 2, P(4096), need - 4, P(0)) == L.GN_ERR_SHAPE
    assert lib.gn_gemm_grouped_det_f32(None, 2, P(4096), need, P(0)) == L.GN_ERR_NULL
    assert lib.gn_gemm_grouped_det_f32(arr, 0, P(4096), need, P(0)) == L.GN_ERR_SHAPE
    assert lib.gn_gemm_grouped_det_f32(arr, L.GEMM_DET_MAX + 1, P(4096), need, P(0)) == L.GN_ERR_SHAPE
    assert lib.gn_gemm_grouped_det_plan(arr, 2, None) == L.GN_ERR_NULL
    bad = (L.GemmDesc * 1)(L.GemmDesc(A=16, B=16, C=16, M=4, N=4, K=4, lda=4, ldb=4, ldc=3, alpha=1.0))
    assert lib.gn_gemm_grouped_det_plan(bad, 1, plan) == L.GN_ERR_SHAPE      # as gn_gemm_grouped_f32: ldc < N
    assert lib.gn_gemm_grouped_det_f32(bad, 1, P(4096), 1 << 20, P(0)) == L.GN_ERR_SHAPE
    grp = lambda **kw: (L.N2EBwdGroup * 1)(L.N2EBwdGroup(**{**dict(xp=16, pq=16, H=16, w2=16, b2=16, dedges=16, dxp=16,
                                                                  dpq=16, dw2=16, db2=16, E=3, sym=0), **kw}))
    n2e = lambda g, B, N, nv, part: lib.gn_node2edge_bwd_det_grouped_f32(g, 1, B, N, nv, part, P(0))
    assert n2e(grp(), 2, D.N2E_MAX_N + 1, None, P(64)) == L.GN_ERR_LDS
    assert n2e(grp(), 2, D.N2E_MAX_N + 1, P(64), P(64)) == L.GN_ERR_LDS
    assert n2e(grp(), 2, 11, None, None) == L.GN_ERR_NULL
    assert n2e(grp(), 2, 11, None, P(66)) == L.GN_ERR_ALIGN
    assert n2e(grp(), 2, 11, P(66), P(64)) == L.GN_ERR_ALIGN                # the counts
    assert n2e(grp(dw2=0), 2, 11, None, P(64)) == L.GN_ERR_NULL
    assert n2e(grp(H=0, E=120), 2, 11, None, P(64)) == L.GN_ERR_SHAPE         # pairwise: E == N*N
    assert n2e(grp(), 0, 11, None, P(64)) == L.GN_ERR_SHAPE
    assert lib.gn_node2edge_bwd_det_grouped_f32(None, 1, 2, 11, None, P(64), P(0)) == L.GN_ERR_NULL


def test_switch_setter_environment_and_none(monkeypatch):
    import groupnet_amd as G
    from groupnet_amd import MS_HGNN_batch as M
    monkeypatch.delenv("GN_DETERMINISTIC", raising=False)
    monkeypatch.setattr(M, "_DETERMINISTIC", None)
    assert G.deterministic() is False                       # default off
    monkeypatch.setenv("GN_DETERMINISTIC", "1")             # read per call
    assert G.deterministic() is True
    G.set_deterministic(False)                              # the setter wins
    assert G.deterministic() is False
    monkeypatch.setenv("GN_DETERMINISTIC", "0")
    G.set_deterministic(True)
    assert G.deterministic() is True
    G.set_deterministic(None)                               # back to the environment
    assert G.deterministic() is False
    monkeypatch.setenv("GN_DETERMINISTIC", "1")
    assert G.deterministic() is True
    # torch's own flag is not read
    monkeypatch.delenv("GN_DETERMINISTIC")
    monkeypatch.setattr(torch, "are_deterministic_algorithms_enabled", lambda: True)
    assert G.deterministic() is False


def test_route_keyword():
    from groupnet_amd import route as RT
    for pairwise in ((True,), (False,), (True, False)):
        for ragged in (False, True):
            with pytest.raises(NotImplementedError, match="140"):
                RT.backward_round_route(141, pairwise, ragged, deterministic=True)
            for N in (1, 11, 140):
                assert RT.backward_round_route(N, pairwise, ragged, deterministic=True) == \
                    RT.backward_round_route(N, pairwise, ragged) == RT.BackwardRound(True, True, True)
    # without the keyword: today's value
    assert RT.backward_round_route(141, (True, False)) == RT.BackwardRound(False, False, False)
    assert RT.backward_round_route(141, (False,)) == RT.BackwardRound(False, True, False)
    assert RT.backward_round_route(141, (True,), False, deterministic=False) == RT.backward_round_route(141, (True,))


# ---- a whole round with a recording stub in place of the library ---------------------------------------------------
class _Stub:
    """Every entry point returns GN_OK and is recorded: (name, groups) — of the node->edge entries also (E, sym) per group."""

    def __init__(self, calls):
        self.calls = calls

    def __getattr__(self, name):
        def call(*a):
            if name.startswith("gn_gemm_grouped"):
                self.calls.append((name, a[1]))
            elif name.startswith("gn_node2edge_bwd"):
                self.calls.append((name, a[1], tuple((a[0][i].E, bool(a[0][i].sym)) for i in range(a[1]))))
            return 0
        return call


def _round_on_the_stub(monkeypatch, counts, det):
    """`backward.modules_backward` for a pairwise + a hyper module (nmp_layers = 2: two rounds) on CPU tensors of the right
    shapes, every launch going to the stub.  -> (recorded calls, N, kinds, edge types)."""
    import test_backward_gpu as TB
    from groupnet_amd import MS_HGNN_batch as M, backward as BW, ops
    from groupnet_amd.weights import _HID, _LGF_LD
    B, N, nmp, Dm = 3, 5, 2, 64
    monkeypatch.delenv("GN_DETERMINISTIC", raising=False)
    monkeypatch.setattr(M, "_DETERMINISTIC", det)
    calls = []
    monkeypatch.setattr(BW, "load", lambda: _Stub(calls))
    monkeypatch.setattr(BW, "stream_handle", lambda: None)
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    z = torch.zeros

    def gather(items):
        calls.append(("agg_gather_grouped", len(items)))
        return [z(B, (N * (N + 1) // 2) if sym else H.shape[1], Dm) for _, H, sym, _ in items]

    def scatter(items, divisor=None, **kw):
        calls.append(("agg_scatter_grouped", len(items)))
        return [z(B, N, 2 * Dm) for _ in items]
    monkeypatch.setattr(ops, "agg_gather_grouped", gather)
    monkeypatch.setattr(ops, "agg_scatter_grouped", scatter)
    monkeypatch.setattr(ops, "zero_padding", lambda items, counts: None)
    monkeypatch.setattr(BW, "_bwd_weights", lambda mod, j: dict(
        Wpq=z(Dm, Dm), bpq=z(Dm), Wd0=z(256, Dm), bd0=z(256), Wd1=z(_LGF_LD, 256), bd1=z(_LGF_LD),
        W1cat=z(mod.edge_types * _HID, Dm), b1cat=z(mod.edge_types * _HID), W2cat=z(Dm, mod.edge_types * _HID),
        b2mat=z((mod.edge_types + 3) // 4 * 4, Dm)))
    pair, hyper = TB._modules(1, nmp)
    traces = []
    for mod, H in ((pair, None), (hyper, z(B, N, N))):
        t = BW.ModuleTrace(mod, z(B, N, Dm), H)
        E, K = (N * (N + 1) // 2 if H is None else N), mod.edge_types
        t.xs = [z(B, N, Dm)] * nmp
        t.dists = [z(B, N * N if H is None else N, K)] * nmp
        t.tails = [dict(x=z(B * N, 2 * Dm), hid=z(B * N, 128))] * nmp
        t.n2e = [dict(x1=z(B * N, 256), xp=z(B, N, Dm), pq=z(B, N, Dm), edges=z(B, E, Dm))] * nmp
        t.estage = [dict(z1=z(B * E, 128), z=z(B * E, Dm), dh1=z(B * E, 256), lgf=z(B * E, _LGF_LD))] * nmp
        if counts is not None:
            t.counts = types.SimpleNamespace(dev=torch.tensor(counts, dtype=torch.int32))
        traces.append(t)
    BW.modules_backward(traces, [z(B, N, Dm)] * 2, [z(B, N * N, pair.edge_types), z(B, N, hyper.edge_types)])
    return calls, N, ["pair", "hyper"], [pair.edge_types, hyper.edge_types]


@pytest.mark.parametrize("counts", [None, (5, 2, 1)], ids=["full", "ragged"])
def test_a_round_issues_only_the_ordered_entries_with_the_mode_on_and_todays_with_it_off(counts, monkeypatch):
    import test_backward_route_gpu as TR
    from groupnet_amd import route as RT
    off, N, kinds, types_ = _round_on_the_stub(monkeypatch, counts, False)
    on, _, _, _ = _round_on_the_stub(monkeypatch, counts, True)
    rt = RT.backward_round_route(N, (True, False), counts is not None)
    today = TR.stated(rt, N, kinds, types_, [[True, True]] * 2)        # the sequence tests/test_backward_route_gpu.py pins
    n2e_today = "gn_node2edge_bwd_grouped_f32" if counts is None else "gn_node2edge_bwd_ragged_grouped_f32"
    today = [(n2e_today, *c[1:]) if c[0] == "gn_node2edge_bwd_grouped_f32" else c for c in today]
    assert off == today
    ordered = {"gn_gemm_grouped_f32": "gn_gemm_grouped_det_f32", n2e_today: "gn_node2edge_bwd_det_grouped_f32"}
    plans = [c for c in on if c[0] == "gn_gemm_grouped_det_plan"]
    launches = [c for c in on if c[0] != "gn_gemm_grouped_det_plan"]
    assert launches == [(ordered.get(c[0], c[0]), *c[1:]) for c in today]
    names = {c[0] for c in on}
    assert not names & {"gn_gemm_grouped_f32", "gn_node2edge_bwd_grouped_f32", "gn_node2edge_bwd_ragged_grouped_f32",
                        "gn_node2edge_bwd_f32"}
    # the plan is asked where a batch holds accumulate problems: deo and the two weight-gradient launches of each round
    assert len(plans) == 3 * 2 and all(n in (2, 8 + sum(types_), 16) for _, n in plans)
