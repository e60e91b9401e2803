"""The launchers' plans (gn_*_plan_*, decided on the host: no GPU) against tests/launch_forms.py `expected_forms`, the
tests' own statement of the launch rules: every case of the GPU launch-form tests, the switch points, a sweep over the
sizes at which a rule changes form, the environment switches, and the launchers' error codes."""
import ctypes
import itertools

import pytest

from launch_forms import (BACKWARD_CASES, FORWARD_CASES, PLACEHOLDER, SCATTER_GPU_CASES, assert_plans_match,
                          assert_scatter_plan, case_forms, expected_forms, launch_descriptors, pair_count, scatter_case_groups,
                          scatter_forms)

SWEEP_B = (1, 5, 64, 369, 370, 512, 2231, 2232, 4064, 4065, 4096, 24544, 24545)
SWEEP_N = (3, 11, 16, 17, 50, 64, 65)
MODES = (("f16x3", "fp32"), ("bf16x6", "fp32"), ("fp32", "fp32"), ("f16x3", "bf16"))
SWITCH_POINTS = [dict(B=B, N=11, scales=[2, 5, 11]) for B in (369, 370, 512, 2231, 2232, 4064, 4065, 24544, 24545)] + [
    dict(B=512, N=11, scales=[2, 5, 11], precision="fp32"), dict(B=512, N=17, scales=[2, 5, 17])]


def _lib():
    from groupnet_amd import _lib as L
    return L, L.load()


def _ask(stem, twin, arr, *args):
    """(return code, plan) of gn_<stem>_plan_{f32,bf16} for a descriptor array and the launcher's scalar arguments."""
    L, lib = _lib()
    plan = L.LaunchPlan()
    rc = getattr(lib, f"gn_{stem}_plan_{'bf16' if twin else 'f32'}")(arr, len(arr) if arr is not None else 0, *args,
                                                                      ctypes.byref(plan))
    return rc, plan


def _name(plan):
    return _lib()[1].gn_kernel_name(plan.kernel).decode()


def check_plans(forms, d, block, where):
    """The plans of the descriptors `d` (launch_descriptors) agree with `forms` (expected_forms of the same arguments)."""
    twin, groups = d["twin"], forms["groups"]
    B, N = groups[0]["rows"] // groups[0]["E"], d["mlp2"][6]
    # the aggregation with the closing stage: accepted exactly when the rules say the closing is fused (the block asks only
    # in its latency form; a module on its own never does)
    rc_c, plan_c = _ask("agg_mlp", twin, d["agg_closing"])
    if block:
        assert (rc_c == 0 and plan_c.closing == 1) == forms["fused_closing"], (where, rc_c)
    plans = [(rc_c, plan_c) if forms["fused_closing"] else _ask("agg_mlp", twin, d["agg"]),
             None if forms["fused_closing"] else _ask("mlp2", twin, *d["mlp2"]),
             # (training and the fp32 cores also pool the pairwise group in that launch: its form is the hyper groups')
             _ask("node2edge", twin, d["n2e"], B, N) if d["n2e"] is not None and any(x.H for x in d["n2e"]) else None,
             _ask("agg_gather", twin, d["gather"], B, N) if d["gather"] is not None else None]
    scatter = _ask("agg_scatter", twin, d["scatter"], B, N, ctypes.c_float(N)) if d["scatter"] is not None else None
    assert all(p is None or p[0] == 0 for p in plans + [scatter]), (where, [p and p[0] for p in plans + [scatter]])
    assert_plans_match(forms, *[p and p[1] for p in plans], where, scatter=scatter and scatter[1])


def _kw(case):
    return dict(B=case["B"], N=case["N"], scales=case["scales"], precision=case["precision"], dtype=case["dtype"],
                training=case["kind"] == "train", block=case["kind"] != "hyper", with_pair=case["kind"] != "hyper")


@pytest.mark.parametrize("case", FORWARD_CASES + BACKWARD_CASES, ids=[c["id"] for c in FORWARD_CASES + BACKWARD_CASES])
def test_plans_of_the_gpu_cases(case):
    check_plans(case_forms(case), launch_descriptors(**_kw(case)), case["kind"] == "block", case["id"])


def test_plans_at_the_switch_points():
    for kw in SWITCH_POINTS:
        check_plans(expected_forms(**kw), launch_descriptors(**kw), True, kw)


@pytest.mark.parametrize("precision,dtype", MODES, ids=[p if d == "fp32" else d for p, d in MODES])
def test_plans_over_the_size_sweep(precision, dtype):
    n = 0
    for B, N in itertools.product(SWEEP_B, SWEEP_N):
        for s in (2, min(5, N), N):
            kw = dict(B=B, N=N, scales=[s], precision=precision, dtype=dtype)
            check_plans(expected_forms(**kw), launch_descriptors(**kw), True, kw)
            n += 1
        kw = dict(B=B, N=N, scales=[2, min(5, N), N], precision=precision, dtype=dtype)
        check_plans(expected_forms(**kw), launch_descriptors(**kw), True, kw)
    assert n == 3 * len(SWEEP_B) * len(SWEEP_N)


def test_switches_move_the_plan(monkeypatch):
    """Every switch is read per call: set and unset between two queries of one process, it moves the plan as its comment
    in the launchers says."""
    for v in ("GN_AGG_RB2", "GN_EDGE_RB2", "GN_RB2_MIN_PAIRS", "GN_MLP2_XS", "GN_N2E_ROWS", "GN_AGG_LINES", "GN_AGG_HSTAGE",
              "GN_XCD", "GN_POOL_STAGE", "GN_SCATTER_PAIRS"):
        monkeypatch.delenv(v, raising=False)

    def name(stem, twin, *a):
        rc, plan = _ask(stem, twin, *a)
        assert rc == 0, (stem, rc)
        return _name(plan)
    # bf16 storage, B = 64, N = 11: far below 2048 row-block pairs
    d = launch_descriptors(64, 11, [2, 5, 11], dtype="bf16")
    tau = (ctypes.c_float(0.5), 0, None, ctypes.c_longlong(0))
    assert (name("agg_mlp", True, d["agg"]), name("edge_mlp_gumbel", True, d["edge"], *tau)) == ("agg_x_kernel", "edge_x_kernel")
    monkeypatch.setenv("GN_AGG_RB2", "1")
    monkeypatch.setenv("GN_EDGE_RB2", "1")
    assert (name("agg_mlp", True, d["agg"]), name("edge_mlp_gumbel", True, d["edge"], *tau)) == ("agg_rb2_kernel", "edge_rb2_kernel")
    monkeypatch.delenv("GN_AGG_RB2")
    monkeypatch.delenv("GN_EDGE_RB2")
    monkeypatch.setenv("GN_RB2_MIN_PAIRS", "8")
    assert (name("agg_mlp", True, d["agg"]), name("edge_mlp_gumbel", True, d["edge"], *tau)) == ("agg_rb2_kernel", "edge_rb2_kernel")
    monkeypatch.setenv("GN_AGG_RB2", "0")
    monkeypatch.setenv("GN_EDGE_RB2", "0")
    assert (name("agg_mlp", True, d["agg"]), name("edge_mlp_gumbel", True, d["edge"], *tau)) == ("agg_x_kernel", "edge_x_kernel")
    for v in ("GN_AGG_RB2", "GN_EDGE_RB2", "GN_RB2_MIN_PAIRS"):
        monkeypatch.delenv(v)
    assert name("agg_mlp", True, d["agg"]) == "agg_x_kernel"
    # closing MLP: xs below 1536 row blocks (B = 2232 unfused: 768 x 4 above it)
    small, large = launch_descriptors(64, 17, [2, 5, 17]), launch_descriptors(2232, 11, [2, 5, 11])
    assert (name("mlp2", False, *small["mlp2"]), name("mlp2", False, *large["mlp2"])) == ("mlp2_xs_kernel", "mlp2_x_kernel")
    monkeypatch.setenv("GN_MLP2_XS", "0")
    assert name("mlp2", False, *small["mlp2"]) == "mlp2_x_kernel"
    monkeypatch.setenv("GN_MLP2_XS", "1")
    assert name("mlp2", False, *large["mlp2"]) == "mlp2_xs_kernel"
    monkeypatch.delenv("GN_MLP2_XS")
    assert name("mlp2", False, *small["mlp2"]) == "mlp2_xs_kernel"
    # node -> edge: banded at B = 512, N = 17 by launch size
    n2e = launch_descriptors(512, 17, [2, 5, 17])["n2e"]
    variant = lambda: _ask("node2edge", False, n2e, 512, 17)[1].variant
    assert variant() == 0
    monkeypatch.setenv("GN_N2E_ROWS", "1")
    assert variant() == 1
    monkeypatch.setenv("GN_N2E_ROWS", "0")
    assert variant() == 0
    monkeypatch.delenv("GN_N2E_ROWS")
    rows = launch_descriptors(2736, 17, [2, 5, 17])["n2e"]
    assert _ask("node2edge", False, rows, 2736, 17)[1].variant == 1
    monkeypatch.setenv("GN_N2E_ROWS", "0")
    assert _ask("node2edge", False, rows, 2736, 17)[1].variant == 0
    monkeypatch.delenv("GN_N2E_ROWS")
    # the closing stage needs the staged ori rows of the line-layout gather
    d = launch_descriptors(512, 11, [2, 5, 11])
    closing = lambda: _ask("agg_mlp", False, d["agg_closing"])
    assert closing()[0] == 0 and list(closing()[1].lines)[:4] == [0, 2, 2, 2]
    for v in ("GN_AGG_LINES", "GN_AGG_HSTAGE"):
        monkeypatch.setenv(v, "0")
        assert closing()[0] == -2, v
        rc, plan = _ask("agg_mlp", False, d["agg"])
        assert rc == 0 and list(plan.lines)[:4] == [0] + [0 if v == "GN_AGG_LINES" else 1] * 3
        monkeypatch.delenv(v)
    assert closing()[0] == 0
    # XCD order: 8 x the largest per-XCD share, or the plain sum
    rc, plan = closing()
    wgs = sum(plan.wgs[i] for i in range(4))
    assert plan.xcd == 1 and plan.grid[0] == case_forms(dict(B=512, N=11, scales=[2, 5, 11], precision="f16x3", dtype="fp32",
                                                             kind="block"))["agg_grid"] >= wgs
    monkeypatch.setenv("GN_XCD", "0")
    rc, plan = closing()
    assert plan.xcd == 0 and plan.grid[0] == wgs
    monkeypatch.delenv("GN_XCD")
    assert closing()[1].xcd == 1


def _scatter_groups(N, spec):
    """spec: a string of group kinds — s: the unordered pairs, o: the ordered pairs, h: a hyper group (E = N) with a dense
    H, m: ... in mask form, 1: the one-hyperedge group (E = 1, dense), w: ... in mask form."""
    kinds = dict(s=dict(E=pair_count(N), sym=True), o=dict(E=N * N), h=dict(E=N, H=True), m=dict(E=N, colmask=True),
                 w=dict(E=1, colmask=True))
    kinds["1"] = dict(E=1, H=True)
    return [kinds[c] for c in spec]


def _scatter_plan(B, N, groups, twin):
    L, _ = _lib()
    P = PLACEHOLDER
    arr = (L.ScatterGroup * len(groups))(*[L.ScatterGroup(feat=P, ori=P, out=P, E=g["E"], sym=int(bool(g.get("sym"))),
                                                         H=P if g.get("H") else 0, colmask=P if g.get("colmask") else 0)
                                           for g in groups])
    return _ask("agg_scatter", twin, arr, B, N, ctypes.c_float(N))


# (B, N, groups): both sides of every rule of scatter_plan
SCATTER_SWITCH_POINTS = (
    # the pairs kernel: B >= 256 and 16 N <= 1024, beside a hyper group and alone; the ordered pairs never take it
    [(B, N, spec) for B in (255, 256) for N in (64, 65) for spec in ("s", "sh", "o")]
    # a hyper group is staged while E (64 + N) floats fit 64 KiB: N = E = 99 | 100
    + [(2, N, spec) for N in (99, 100) for spec in ("h", "hs")]
    # scenes per workgroup: 1 | 2 at 2048 workgroups of one and of two groups, 8 | 16 with ten groups; a tile beyond
    # 12 KiB (N = E = 64) is never doubled
    + [(B, 3, spec) for B in (4094, 4095) for spec in ("h", "m")] + [(B, 3, spec) for B in (2046, 2047) for spec in ("hh", "mm")]
    + [(B, 3, spec) for B in (3264, 3265) for spec in ("h" * 10, "m" * 10, "mmmmwmmmmw")]
    + [(4095, 64, "h"), (4095, 64, "m"), (4095, 64, "mw"), (70000, 17, "h1s"), (70000, 17, "mws")])


@pytest.mark.parametrize("twin", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("pairs_env", [None, "0", "1"], ids=["unset", "pairs0", "pairs1"])
def test_scatter_plans_at_the_switch_points(twin, pairs_env, monkeypatch):
    """gn_agg_scatter_plan_* against `scatter_forms` on both sides of every rule, GN_SCATTER_PAIRS unset, 0 and 1 (read
    per call), both storage types; and the case table reaches every form and every G."""
    if pairs_env is None:
        monkeypatch.delenv("GN_SCATTER_PAIRS", raising=False)
    else:
        monkeypatch.setenv("GN_SCATTER_PAIRS", pairs_env)
    seen = set()
    for B, N, spec in SCATTER_SWITCH_POINTS:
        groups = _scatter_groups(N, spec)
        sf = scatter_forms(B, N, groups, pairs_switch=pairs_env != "0")
        rc, plan = _scatter_plan(B, N, groups, twin)
        assert rc == 0 and plan.precision == int(twin), (B, N, spec, rc)
        assert_scatter_plan(sf, plan, (B, N, spec))
        seen |= {(N, B, spec[i], k) for i, (k, _) in sf["own"].items()} | {(sf["kernel"], len(spec), B, sf["G"])}
    pairs = pairs_env != "0"
    for B, N in ((255, 64), (256, 64), (255, 65), (256, 65)):
        assert (N, B, "s", "agg_scatter_pairs_kernel" if pairs and (B, N) == (256, 64) else "agg_scatter_direct_kernel") in seen
        assert (N, B, "o", "agg_scatter_direct_kernel") in seen
    assert (99, 2, "h", "agg_scatter_direct_kernel") not in seen and (100, 2, "h", "agg_scatter_direct_kernel") in seen
    for kern in ("agg_scatter_kernel", "agg_scatter_mask_kernel"):
        assert {(kern, 1, 4094, 1), (kern, 1, 4095, 2), (kern, 2, 2046, 1), (kern, 2, 2047, 2), (kern, 10, 3264, 8),
                (kern, 10, 3265, 16)} <= seen
    assert ("agg_scatter_kernel", 1, 4095, 1) in seen and ("agg_scatter_mask_kernel", 1, 4095, 1) in seen      # N = E = 64
    # dense and mask hyper groups in one call: refused by both, nothing launched
    for spec in ("hm", "mh", "sm1"):
        groups = _scatter_groups(17, spec)
        assert scatter_forms(5, 17, groups) is None and _scatter_plan(5, 17, groups, twin)[0] == -2, spec


def test_scatter_gpu_cases_reach_the_forms_they_name(monkeypatch):
    """Every case of the GPU test of the scatter's forms: the rules and the library's plan give the form the case names,
    and the packed cases leave one scene to the last workgroup."""
    monkeypatch.delenv("GN_SCATTER_PAIRS", raising=False)
    for B, N, spec, dtypes, (kernel, G) in SCATTER_GPU_CASES:
        groups = scatter_case_groups(N, spec)
        sf = scatter_forms(B, N, groups)
        if G:
            assert (sf["kernel"], sf["G"], sf["own"]) == (kernel, G, {}) and (G == 1 or B % G == 1), (B, N, spec)
        else:
            assert sf["kernel"] is None and [k for k, _ in sf["own"].values()] == [kernel], (B, N, spec)
        for dt in dtypes:
            rc, plan = _scatter_plan(B, N, groups, dt == "bf16")
            assert rc == 0
            assert_scatter_plan(sf, plan, (B, N, spec, dt))
    reached = {c[4] for c in SCATTER_GPU_CASES}
    assert {k for k, _ in reached} == {"agg_scatter_pairs_kernel", "agg_scatter_direct_kernel", "agg_scatter_kernel",
                                       "agg_scatter_mask_kernel"}


def test_edge_plan_sizes_the_stage_from_the_static_lds(monkeypatch):
    """The edge launch's dynamic LDS is the weight ring and the pool stage in one region.  The kernel's static LDS, which
    bounds the stage, is known to the runtime only: here it is an argument (tests/test_edge_lds_layout_gpu.py checks the
    real values through launch_info).  GN_POOL_STAGE = 0: the ring alone, every hyper group unstaged."""
    monkeypatch.delenv("GN_POOL_STAGE", raising=False)
    monkeypatch.delenv("GN_EDGE_RB2", raising=False)
    d = launch_descriptors(512, 16, [2, 5, 16])      # (N = 16: the hyper stage, 144 node rows, is larger than the ring)
    ask = lambda static: _ask("edge_mlp_gumbel", False, d["edge"], ctypes.c_float(0.5), 0, None, ctypes.c_longlong(static))
    rc, free = ask(0)                       # no static LDS: the largest stage fits
    assert rc == 0 and _name(free) == "edge_x_kernel" and free.precision == 2
    # (the scale = N group, one hyperedge per scene, would stage the nodes of 129 scenes: never staged)
    assert free.stage_bytes == free.dyn_lds and list(free.unstaged)[:4] == [0, 0, 0, 1]
    rc, full = ask(160 * 1024)              # static LDS takes the whole share: nothing beyond the ring
    assert rc == 0 and full.stage_bytes == full.dyn_lds < free.dyn_lds
    assert list(full.unstaged)[:4] == [0, 1, 1, 1]      # the E = 16 groups pool from global memory, a workgroup per row block
    assert sum(full.wgs[i] for i in range(4)) > sum(free.wgs[i] for i in range(4))
    monkeypatch.setenv("GN_POOL_STAGE", "0")
    rc, off = ask(0)
    assert rc == 0 and off.stage_bytes == -1 and off.dyn_lds == full.dyn_lds      # the ring alone
    assert list(off.unstaged)[:4] == [0, 0, 0, 0]                                  # (per-member reference form, no sparse grid)
    monkeypatch.delenv("GN_POOL_STAGE")
    assert ask(0)[1].dyn_lds == free.dyn_lds


def test_queries_return_the_launchers_error_codes():
    """Every invalid descriptor of tests/test_capi_cpu.py::test_null_and_shape_errors_do_not_launch: the plan query
    returns what the launcher returns."""
    L, lib = _lib()
    P = ctypes.c_void_p
    plan = ctypes.byref(L.LaunchPlan())

    def both(stem, arr, *args, tail=()):
        a = getattr(lib, f"gn_{stem}_f32")(arr, *args, P(0))
        b = getattr(lib, f"gn_{stem}_plan_f32")(arr, *args, *tail, plan)
        assert a == b, (stem, a, b)
        return a
    g = (L.Mlp2Group * 1)(L.Mlp2Group(x=16, W=16, bias=16, y=16))
    assert both("mlp2", g, 1, 5, 96, 128, 64, 64, 0, 1.0) == -2
    assert both("mlp2", g, 0, 5, 128, 128, 64, 64, 0, 1.0) == -2
    assert both("mlp2", g, 11, 5, 128, 128, 64, 64, 0, 1.0) == -2
    assert both("mlp2", None, 1, 5, 128, 128, 64, 64, 0, 1.0) == -1
    g[0].x = 0
    assert both("mlp2", g, 1, 22, 64, 128, 64, 64, 11, 11.0) == -2
    assert both("mlp2", g, 1, 22, 128, 128, 64, 64, 11, 0.0) == -2
    a = (L.AggGroup * 1)(L.AggGroup(eo=16, edge_feat=16, W=16, b1=16, b2=16, feat=16, rows=5, K=17))
    assert both("agg_mlp", a, 1) == -2
    a[0].K, a[0].W = 6, 8
    assert both("agg_mlp", a, 1) == -4
    n = (L.N2EGroup * 1)(L.N2EGroup(xp=16, pq=16, w2=16, edges=16, b2=16, E=8))
    assert both("node2edge", n, 1, 2, 3) == -2
    n[0].b2 = 0
    assert both("node2edge", n, 1, 2, 3) == -1
    e = (L.EdgeGroup * 1)(L.EdgeGroup(edges=16, W=16, bias=16, edge_feat=16, dist=16, rows=10, K=16))
    assert both("edge_mlp_gumbel", e, 1, 0.5, 0, P(0), tail=(0,)) == -2
    e[0].K = 10
    assert both("edge_mlp_gumbel", e, 1, 0.0, 0, P(0), tail=(0,)) == -2
    assert lib.gn_agg_mlp_plan_f32(a, 1, None) == -1 and lib.gn_kernel_name(99) is None
