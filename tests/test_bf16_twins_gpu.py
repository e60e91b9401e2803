"""The bf16 twins (`gn_*_bf16`) element by element (tests/bf16_twin_cases.py; the conditions on the references:
tests/test_bf16_twins_cpu.py).

Every stage alone through `groupnet_amd.ops` on bf16 tensors, the plan of each launch held against the rules where a
helper states them (a case must not silently run another kernel than the one named):

A. random data against the float64 emulation: EVERY element of every output is the rounding of some value within the
   slack, [bf16(pre - s), bf16(pre + s)] — no whole-tensor norm, no excluded rows.  pq of the node stage is held on the x'
   the twin stored, and against the wider a-priori reference as well.  Every test prints, per output, the share of elements not bit-identical to the emulation and the worst
   |twin - pre| / (s + ulp) (records).
B. the exact-arithmetic probes: the twin, and fp32 storage on all three matrix paths, equal the float64 reference bit
   for bit.
"""
import pytest
import torch

import bf16_twin_cases as T
from bottleneck_cases import closing_case, closing_launch_form
from device_noise_cases import KERNELS, select_kernel
from edge_type_cases import agg_launch_forms
from test_bottleneck_gpu import _launch, holder  # noqa: F401  (holder: a fixture)
from test_device_noise_gpu import _assert_kernel, _spy_edge_plans
from test_edge_types_gpu import _agg_source, _name, _set_precision
from test_launch_forms_gpu import _spy_plans

pytestmark = pytest.mark.gpu

TWIN_EDGE_KERNELS = [k for k in KERNELS if k.dtype == "bfloat16"]      # one and two row blocks per wave (GN_EDGE_RB2)


def dev():
    return torch.device("cuda:0")


def _hold(case, what: str, got: torch.Tensor, o: T.Out, lines) -> None:
    """THE RULE on every element of one output."""
    assert got.numel() == o.pre.numel(), (T.case_id(case), what, tuple(got.shape), tuple(o.pre.shape))
    r = T.rule_report(got, o)
    lines.append(f"{what}: {r['differ']:.2%} of {r['n']} not bit-identical, worst |twin - pre| / (s + ulp) {r['worst']:.2f}")
    assert r["fail"] == 0, (T.case_id(case), what, f"{r['fail']} of {r['n']} elements outside [round(pre - s), round(pre + s)]", lines[-1])


@pytest.mark.parametrize("case", T.NODE_CASES, ids=[T.case_id(c) for c in T.NODE_CASES])
def test_node_stage_rule(case):
    from groupnet_amd import ops
    c = T.case_inputs(case)
    pk = c["mod"].to(dev())._packed_n2e(0)
    xp, pq = ops.node_mlp(c["x"].to(dev()).bfloat16(), pk)
    assert xp.dtype == pq.dtype == torch.bfloat16
    ref = T.reference(case)
    lines = []
    _hold(case, "xp", xp, ref["xp"], lines)
    # pq from the x' the twin stored: one layer behind a determined value; condition (b) again on that very input
    with torch.no_grad():
        on_stored = T.node_emul(c["state"], c["x"], T.Arith(), xp_stored=xp.float())["pq"]
    assert float(T.allowance_share(on_stored, T.ref64(case)["pq"]).max()) <= 1.0
    _hold(case, "pq", pq, on_stored, lines)
    # ... and against the a-priori reference, which takes nothing from the kernel (x's flippable elements propagated: wider)
    _hold(case, "pq (a-priori reference)", pq, T.case_inputs(case)["ref"]["pq_apriori"], lines)
    print(f"\n{T.case_id(case)}: " + "; ".join(lines), end="")


@pytest.mark.parametrize("kernel", TWIN_EDGE_KERNELS, ids=[k.id for k in TWIN_EDGE_KERNELS])
@pytest.mark.parametrize("case", T.EDGE_CASES, ids=[T.case_id(c) for c in T.EDGE_CASES])
def test_edge_head_rule(case, kernel, monkeypatch):
    from groupnet_amd import ops
    dtype = select_kernel(kernel, monkeypatch)
    plans = []
    _spy_edge_plans(monkeypatch, plans)
    c = T.case_inputs(case)
    K, sym_N = c["K"], c["sym_N"]
    pk = c["mod"].to(dev())._packed()
    (fd, dist), = ops.edge_mlp_gumbel_grouped([(c["edges"].to(dev()).to(dtype), c["U"].to(dev()), pk, K, sym_N, True)])
    assert fd.dtype == torch.float32 and dist.dtype == torch.bfloat16
    _assert_kernel(plans, kernel, 1)
    ref = T.reference(case)
    lines = []
    _hold(case, "fac * dist", fd, ref["fd"], lines)
    _hold(case, "dist", dist, ref["dist"], lines)
    print(f"\n{T.case_id(case)} {kernel.id}: " + "; ".join(lines), end="")


@pytest.mark.parametrize("case", T.AGG_CASES, ids=[T.case_id(c) for c in T.AGG_CASES])
def test_typed_aggregation_rule(case, monkeypatch):
    from groupnet_amd import ops
    _, K, rb2, form, B, N, x = case
    _set_precision("f16x3", monkeypatch)
    plans = []
    _spy_plans(monkeypatch, plans)
    c = T.case_inputs(case)
    pk = c["mod"].to(dev())._packed()
    ref = T.reference(case)["feat"]
    lines = []
    # (the scene form has a kernel of its own: it runs, and is held, under both settings)
    for flag in (("0", "1") if form == "scene" else ("1" if rb2 else "0",)):
        monkeypatch.setenv("GN_AGG_RB2", flag)
        n0 = len(plans)
        (got,) = ops.agg_mlp_grouped([(_agg_source(case[3:], c["inp"], K, pk, torch.bfloat16), c["inp"]["ef"].to(dev()), pk, K)])
        assert got.dtype == torch.bfloat16
        (stem, rc, plan), = plans[n0:]
        want = agg_launch_forms(case[3:], K, "f16x3", "bf16", flag)
        assert rc == 0 and plan.n_groups == 1 and (plan.wpr[0], bool(plan.node_form[0])) == (want["wpr"], want["node_form"])
        if want["scene_grid"] is not None:
            assert (_name(plan.pre_kernel[0]), plan.pre_grid[0]) == ("agg_scene_kernel", want["scene_grid"])
        else:
            assert _name(plan.kernel) == want["kernel"] and plan.pre_grid[0] == 0, _name(plan.kernel)
        _hold(case, f"feat (GN_AGG_RB2={flag})", got, ref, lines)
    print(f"\n{T.case_id(case)}: " + "; ".join(lines), end="")


@pytest.mark.parametrize("case", T.CLOSING_CASES, ids=[T.case_id(c) for c in T.CLOSING_CASES])
def test_closing_mlp_rule(case, holder, monkeypatch):  # noqa: F811
    _, d, form = case
    plans, lines = [], []
    _spy_plans(monkeypatch, plans)
    ref = T.reference(case)["y"]
    c = closing_case((form,), d, True)
    for xs in ("0", "1"):                       # both bf16-core kernels (GN_MLP2_XS); _launch holds the plan
        (y,) = _launch(holder, c, (form,), d, ("f16x3", "bf16"), xs, monkeypatch, plans)
        _hold(case, f"y ({closing_launch_form((form,), d, 'f16x3', 'bf16', xs)[0]})", y, ref, lines)
    print(f"\n{T.case_id(case)}: " + "; ".join(lines), end="")


# ---- B. exact-arithmetic probes: bit for bit, on bf16 storage and on the three matrix paths of fp32 storage -------------------
PATHS = ("f16x3", "bf16x6", "fp32")
STORAGE = [("bf16", "f16x3")] + [("fp32", p) for p in PATHS]
STORAGE_IDS = ["bf16"] + list(PATHS)


def _same(case, what, got, want):
    g = got.detach().double().cpu().reshape(want.shape)
    bad = int((g != want).sum())
    assert bad == 0, (T.probe_id(case), what, f"{bad} of {want.numel()} elements differ from the exact result",
                      float((g - want).abs().max()))


@pytest.mark.parametrize("storage,path", STORAGE, ids=STORAGE_IDS)
@pytest.mark.parametrize("case", T.PROBE_NODE, ids=[T.probe_id(c) for c in T.PROBE_NODE])
def test_node_stage_probe(case, storage, path, monkeypatch):
    from groupnet_amd import ops
    _set_precision(path, monkeypatch)
    c, ref = T.probe_inputs(case), T.probe_reference(case)
    tdt = torch.bfloat16 if storage == "bf16" else torch.float32
    xp, pq = ops.node_mlp(c["x"].to(dev()).to(tdt), c["mod"].to(dev())._packed_n2e(0))
    assert xp.dtype == tdt
    _same(case, "xp", xp, ref["xp"])
    _same(case, "pq", pq, ref["pq"])


@pytest.mark.parametrize("kernel", KERNELS, ids=[k.id for k in KERNELS])
@pytest.mark.parametrize("case", T.PROBE_EDGE, ids=[T.probe_id(c) for c in T.PROBE_EDGE])
def test_edge_head_probe(case, kernel, monkeypatch):
    from groupnet_amd import ops
    dtype = select_kernel(kernel, monkeypatch)
    plans = []
    _spy_edge_plans(monkeypatch, plans)
    c, ref = T.probe_inputs(case), T.probe_reference(case)
    (fd, dist), = ops.edge_mlp_gumbel_grouped([(c["edges"].to(dev()).to(dtype), c["U"].to(dev()), c["mod"].to(dev())._packed(),
                                                c["K"], c["sym_N"], True)])
    _assert_kernel(plans, kernel, 1)
    _same(case, "dist", dist, ref["dist"])
    _same(case, "fac * dist", fd, ref["fd"])


# every form a storage type has (the fp32 cores have no node form)
AGG_PROBE_RUNS = [(c, st, p) for c in T.PROBE_AGG for st, p in STORAGE
                  if c[2] in (T.TWIN_FORMS if st == "bf16" else T.FP32_FORMS) and not (p == "fp32" and c[2] == "pair-node")]


@pytest.mark.parametrize("case,storage,path", AGG_PROBE_RUNS,
                         ids=[f"{T.probe_id(c)}-{'bf16' if st == 'bf16' else p}" for c, st, p in AGG_PROBE_RUNS])
def test_typed_aggregation_probe(case, storage, path, monkeypatch):
    from groupnet_amd import ops
    _, K, form, B, N, x = case
    twin = storage == "bf16"
    _set_precision(path, monkeypatch)
    plans = []
    _spy_plans(monkeypatch, plans)
    c, ref = T.probe_inputs(case), T.probe_reference(case)["feat"]
    pk = c["mod"].to(dev())._packed()
    tdt = torch.bfloat16 if twin else torch.float32
    for flag in (("0", "1") if twin else (None,)):
        if flag is None:
            monkeypatch.delenv("GN_AGG_RB2", raising=False)
        else:
            monkeypatch.setenv("GN_AGG_RB2", flag)
        n0 = len(plans)
        (got,) = ops.agg_mlp_grouped([(_agg_source(case[2:], c["inp"], K, pk, tdt), c["inp"]["ef"].to(dev()), pk, K)])
        (stem, rc, plan), = plans[n0:]
        want = agg_launch_forms(case[2:], K, path, storage, flag)
        assert rc == 0 and (plan.wpr[0], bool(plan.node_form[0])) == (want["wpr"], want["node_form"])
        if want["scene_grid"] is not None:
            assert (_name(plan.pre_kernel[0]), plan.pre_grid[0]) == ("agg_scene_kernel", want["scene_grid"])
        else:
            assert _name(plan.kernel) == want["kernel"] and plan.pre_grid[0] == 0, _name(plan.kernel)
        _same(case, f"feat (GN_AGG_RB2={flag})", got, ref)


@pytest.mark.parametrize("storage,path", STORAGE, ids=STORAGE_IDS)
@pytest.mark.parametrize("case", T.PROBE_CLOSING, ids=[T.probe_id(c) for c in T.PROBE_CLOSING])
def test_closing_mlp_probe(case, storage, path, holder, monkeypatch):  # noqa: F811
    from test_bottleneck_gpu import _xs_settings
    _, d, form = case
    plans = []
    _spy_plans(monkeypatch, plans)
    c, ref = T.probe_inputs(case), T.probe_reference(case)["y"]
    mode = (path, storage)
    for xs in _xs_settings(mode, d):
        (y,) = _launch(holder, dict(srcs=[c["src"]], mlps=[c["mod"]]), (form,), d, mode, xs, monkeypatch, plans)
        _same(case, f"y (GN_MLP2_XS={xs})", y, ref)
