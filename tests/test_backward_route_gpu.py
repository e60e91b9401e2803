"""`backward.round_backward` follows `route.backward_round_route`: the grouped launches the backward is made of —
`ops.node2edge_grouped`, `ops.agg_gather_grouped`, `ops.agg_scatter_grouped` and the library's `gn_gemm_grouped_f32`,
`gn_node2edge_bwd_grouped_f32`, `gn_node2edge_bwd_f32` — are wrapped with recording pass-throughs (names and group counts;
of the node->edge entries also each group's rows and `sym`), one forward and one backward run per case, and the recorded
backward is the sequence the route states.  Every case also names, as literals, the fields of the route its behaviour
rests on, and its gradients are held against the oracle's autograd (same weights, inputs and noise) under
tests/test_backward_gpu.py's `TOL_ANY`.  The cases are the smallest on each boundary of the round's route."""
import functools

import pytest
import torch

import test_backward_gpu as TB
from oracle import ms_hgnn_oracle as O

pytestmark = pytest.mark.gpu

SCALE = 3                   # of the hyper module (`test_backward_gpu._modules`): E = N hyperedges
BOTH, FACTORS = (True, True), (False, True)          # which of (node_feat, factors) the loss reads

# case -> (B, N, nmp_layers, modules as (kind, outputs the loss reads)), what its route must say
CASES = {
    "pair+hyper": ((2, 5, 1, (("pair", BOTH), ("hyper", BOTH))), dict(pair_rows=True, kept=True, n2e_grouped=True)),
    "pair+hyper-nmp2": ((2, 5, 2, (("pair", BOTH), ("hyper", BOTH))), dict(pair_rows=True, kept=True, n2e_grouped=True)),
    # the edge2node block of the last round runs for the modules whose node_feat is read
    "live-subset": ((2, 5, 1, (("pair", FACTORS), ("hyper", BOTH))), dict(pair_rows=True, kept=True, n2e_grouped=True)),
    "pair-largest-scene": ((1, 140, 1, (("pair", BOTH),)), dict(pair_rows=True, kept=True, n2e_grouped=True)),
    "pair-first-beyond": ((1, 141, 1, (("pair", BOTH),)), dict(pair_rows=False, kept=False, n2e_grouped=False)),
    "hyper-beyond": ((1, 141, 1, (("hyper", BOTH),)), dict(kept=True, n2e_grouped=False)),
    "pair+hyper-beyond": ((1, 141, 1, (("pair", BOTH), ("hyper", BOTH))), dict(pair_rows=False, kept=False, n2e_grouped=False)),
}


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def reference(kind, B, N, nmp, outputs):
    """The oracle's autograd for one module of a case, computed once per (module, shape, loss) and left unchanged:
    h and the module's weights depend on (N, nmp) alone, so the modules of a case — and the cases of one shape — share them."""
    pair, hyper = TB._modules(500 + N, nmp)
    mod = pair if kind == "pair" else hyper
    state = {k: v.detach().clone().requires_grad_(True) for k, v in mod.state_dict().items()}
    h = torch.randn(B, N, 64, generator=torch.Generator().manual_seed(N + nmp))
    g = torch.Generator().manual_seed(N + nmp + (1000 if kind == "pair" else 2000))
    U = [torch.rand(s, generator=g) for s in O.noise_shapes(B, N, None if kind == "pair" else SCALE, nmp)]
    hh = h.clone().requires_grad_(True)
    if kind == "pair":
        (nf, fac), H = O.ms_hgnn_pairwise_forward(state, hh, U, nmp_layers=nmp, decomposed=True), None
    else:
        nf, fac, H = O.ms_hgnn_hyper_forward(state, hh, O.affinity(h), SCALE, U, nmp_layers=nmp, decomposed=True)
    R = [torch.randn(t.shape, generator=g) for t in (nf, fac)]
    sum((t * r).sum() for t, r, used in zip((nf, fac), R, outputs) if used).backward()
    return dict(h=h, U=U, H=H, R=R, nf=nf.detach(), g_h=hh.grad, grads={k: v.grad for k, v in state.items()})


def record(monkeypatch):
    from groupnet_amd import _lib, ops
    calls = []

    def wrap(owner, name, what):
        real = getattr(owner, name)

        def through(*args, **kwargs):
            calls.append((name, *what(*args, **kwargs)))
            return real(*args, **kwargs)
        monkeypatch.setattr(owner, name, through)
    wrap(ops, "node2edge_grouped", lambda items, **kw: (len(items), tuple(len(it) > 5 and bool(it[5]) for it in items)))
    wrap(ops, "agg_gather_grouped", lambda items: (len(items),))
    wrap(ops, "agg_scatter_grouped", lambda items, divisor=None, **kw: (len(items),))
    lib = _lib.load()
    wrap(lib, "gn_gemm_grouped_f32", lambda descs, n, stream: (n,))
    wrap(lib, "gn_node2edge_bwd_grouped_f32",
         lambda arr, n, B, N, stream: (n, tuple((arr[i].E, bool(arr[i].sym)) for i in range(n))))
    wrap(lib, "gn_node2edge_bwd_f32", lambda *a: (1, ((a[12], bool(a[13])),)))
    return calls


def stated(rt, N, kinds, types, live_rounds):
    """The recorded calls of a backward that follows the route `rt`: kinds / types = per module "pair" | "hyper" and its K
    edge types; live_rounds = per round, last round first, which modules' round output carries a gradient."""
    n, gemm = len(kinds), lambda k: ("gn_gemm_grouped_f32", k)
    pair_rows = [kind == "pair" and rt.pair_rows for kind in kinds]
    rows = tuple(((N * (N + 1) // 2 if sym else N * N) if kind == "pair" else N, sym) for kind, sym in zip(kinds, pair_rows))
    ev = []
    for live in live_rounds:
        nl = sum(live)
        if not rt.kept:         # node MLP (2 layers), attention layer 0, the pooling, edge MLP (2), distribution | factor (2)
            ev += [gemm(n)] * 3 + [("node2edge_grouped", n, tuple(pair_rows))] + [gemm(n)] * 4
        if nl:                  # eo, Hc, dy1, (da, dx), dfeat, T, deo, d ori; then e1, e0, W1cat, b2 and K x W2 per module
            ev += [("agg_gather_grouped", nl), gemm(nl), gemm(nl), gemm(2 * nl), ("agg_gather_grouped", nl), gemm(nl),
                   gemm(nl), ("agg_scatter_grouped", nl), gemm(sum(4 + K for K, on in zip(types, live) if on))]
        ev += [gemm(n)] * 4     # dd1, dz, dz1, dedges
        if rt.n2e_grouped:
            ev.append(("gn_node2edge_bwd_grouped_f32", n, rows))
        else:
            ev += [("gn_node2edge_bwd_f32", 1, (r,)) for r in rows]
        ev += [gemm(n)] * 3 + [gemm(8 * n)]     # dxp += dpq Wpq, dx1, dx; then 8 weight-gradient problems per module
    return ev


@pytest.mark.parametrize("name", list(CASES))
def test_backward_follows_the_round_route(name, monkeypatch):
    """Forward and backward as `MSHGNNFunction` runs them, the backward entered at `modules_backward` with the loss's
    gradients — None for an output the loss does not read, which is how a module falls out of the edge2node block
    (autograd itself hands a custom function zeros there)."""
    from groupnet_amd import MS_HGNN_batch as M, route as R
    from groupnet_amd.backward import ModuleTrace, modules_backward
    (B, N, nmp, modules), expect = CASES[name]
    kinds, n = [kind for kind, _ in modules], len(modules)
    rt = R.backward_round_route(N, tuple(kind == "pair" for kind in kinds))
    assert {k: getattr(rt, k) for k in expect} == expect, (rt, expect)
    refs = [reference(kind, B, N, nmp, outputs) for kind, outputs in modules]
    pair, hyper = TB._modules(500 + N, nmp)
    mods = [(pair if kind == "pair" else hyper).to(dev()).train() for kind in kinds]
    x = refs[0]["h"].to(dev())
    Hs = [None if r["H"] is None else r["H"].to(dev()) for r in refs]
    calls = record(monkeypatch)
    traces = [ModuleTrace(m, x, H) for m, H in zip(mods, Hs)]
    with torch.no_grad(), M.training_call():
        res = M.run_message_passing(mods, [x] * n, Hs, [[u.to(dev()) for u in r["U"]] for r in refs], [None] * n,
                                    traces=traces)
    for (nf, _), r in zip(res, refs):
        assert float((nf.cpu() - r["nf"]).abs().max()) <= 1e-5
    g_out = [[w.to(dev()) if used else None for w, used in zip(r["R"], outputs)] for r, (_, outputs) in zip(refs, modules)]
    calls.clear()
    dxs, grads = modules_backward(traces, [g[0] for g in g_out], [g[1] for g in g_out])
    torch.cuda.synchronize()

    # the last round's edge2node block runs where node_feat is read; every earlier round feeds the next one
    live_rounds = [[outputs[0] for _, outputs in modules]] + [[True] * n] * (nmp - 1)
    want = stated(rt, N, kinds, [m.edge_types for m in mods], live_rounds)
    assert calls == want, (calls, want)
    names, counts = [c[0] for c in calls], [c[1] for c in calls]
    if rt.kept:
        assert "node2edge_grouped" not in names                    # nothing is re-computed
    if name == "pair+hyper-nmp2":
        assert names.count("gn_node2edge_bwd_grouped_f32") == 2     # one per round
    if name == "live-subset":       # the block and its weight gradients with one group, everything after with two
        assert counts == [1, 1, 1, 2, 1, 1, 1, 1, 4 + mods[1].edge_types] + [2] * 8 + [16]
        assert names[0] == names[4] == "agg_gather_grouped" and names[7] == "agg_scatter_grouped"
    if name == "pair-largest-scene":
        assert calls[-5] == ("gn_node2edge_bwd_grouped_f32", 1, ((9870, True),))
    if name == "pair-first-beyond":
        assert calls[3] == ("node2edge_grouped", 1, (False,))
        assert calls[-5] == ("gn_node2edge_bwd_f32", 1, ((141 * 141, False),))
    if name == "pair+hyper-beyond":
        assert names.count("gn_node2edge_bwd_f32") == 2 and names.count("node2edge_grouped") == 1

    g_h = sum(r["g_h"] for r in refs)
    eh = float((sum(dxs).cpu() - g_h).abs().max()) / float(g_h.abs().max())
    assert eh <= TB.TOL_ANY, (name, "dL/dh", eh)
    for m, r, kind in zip(mods, refs, kinds):
        used = [k for k, v in r["grads"].items() if v is not None and float(v.abs().max()) > 0]
        assert len(used) >= 15
        ew, where = TB._check({k: grads.get(p) for k, p in m.named_parameters()}, r["grads"], used, TB.TOL_ANY)
        print(f"\n{name}/{kind}: dL/dh {eh:.1e}, worst parameter {ew:.1e} ({where}), {len(used)} used parameters")
