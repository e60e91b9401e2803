"""The closing MLP and whole modules at every bottleneck width, against float64.

The suite compared results with a reference at the widths 64, 96 and 1024 only, while the launchers branch on the output
width dout of the closing MLP (tests/bottleneck_cases.py lists where).  Four parts, every reference plain torch in float64
on inputs drawn on the CPU (tests/test_bottleneck_cpu.py holds the conditions on those inputs):

  1. `ops.mlp2_grouped` alone: (a) ROWS = 69 plain rows at every width 1..64 and beyond, both bf16-core kernels
     (GN_MLP2_XS = 0 | 1) and the three matrix paths, the plan of that very launch held against the rule (kernel,
     tiles[2]); (b) the output written as a column block of a wider, sentinel-filled tensor with guard rows, at a row
     stride that is a multiple of 4 and at one that is not; (c) the fused-scatter input forms, two groups in one launch,
     and the kept activations of training; (d) the other exported (din, dh); (e) all of it on bf16 storage;
  2. `run_message_passing(fuse_closing=True)` on [pairwise, hyper 3, hyper N] on both sides of the widths at which the
     aggregation launch takes the closing stage (33..64), the outputs being column blocks of one wide tensor;
  3. `MS_HGNN_oridinary` / `MS_HGNN_hyper` through their own forward at D_EDGES, N = 5, 11 and 20, one and two rounds, fp32
     and bf16 storage, and the refusal of bf16 storage beyond 64 before anything is launched;
  4. training: dL/dh and every parameter gradient against float64 autograd of the oracle.

Gates (none measured on the code under test).  fp32 storage: max|hip - ref64| <= TOL_FEAT (2e-6) of max|ref64|, factors
TOL_FAC (5e-6) absolute; the fp32 CPU reference stays within a third of that on every case's inputs.  bf16 storage:
max|hip - ref64| <= 4 e_emu, e_emu the distance from ref64 of a CPU restatement with operands, hidden activations and
results rounded to bf16, and 4 e_emu <= 1.5e-2 of max|ref64|.  Gradients: TOL_CLEAN / TOL_ANY of tests/test_backward_gpu.py.
Every test prints `measured / reference's own error / gate`; the module prints the worst per part, path and width class
when it ends.
"""
import contextlib

import pytest
import torch

from bottleneck_cases import (BACKWARD_D, BACKWARD_KINDS, BACKWARD_SIZE, D_ALL, D_EDGES, D_IMAGE, D_WIDE, FUSED_CASES, INPUT_FORMS,
                              MODULE_KINDS, MODULE_N, OTHER_D, OTHER_WIDTHS, PLACEMENT_D, ROWS, TOL_FEAT, TWO_GROUPS, X_FORM,
                              backward_case, closing_case, closing_launch_form, form_edges, form_id, module_case, module_case_id,
                              module_cases, module_forms, width_class)
from edge_type_cases import abs_err, backward_reference, rel_err
from relu_probe import WINDOW
from test_backward_gpu import TOL_ANY, TOL_CLEAN, _check
from test_launch_forms_gpu import _spy_plans
from test_parity_gpu import _with_precision
from test_route_gpu import record

pytestmark = pytest.mark.gpu

MODES = (("f16x3", "fp32"), ("bf16x6", "fp32"), ("fp32", "fp32"), ("f16x3", "bf16"))      # (matrix path, storage)
MODE_IDS = [p if d == "fp32" else d for p, d in MODES]
SENTINEL = -24576.0      # (bf16-representable)
WORST = {}               # (part, path, width class) -> (measured, reference's own error, gate), shares of max|ref64|


def dev():
    return torch.device("cuda:0")


def _name(kernel):
    from groupnet_amd import _lib
    return (_lib.load().gn_kernel_name(kernel) or b"").decode()


def _note(part, mode, d, measured, own, gate):
    key = (part, mode, width_class(d))
    if key not in WORST or measured / gate > WORST[key][0] / WORST[key][2]:
        WORST[key] = (measured, own, gate)


@pytest.fixture(scope="module", autouse=True)
def _summary():
    yield
    lines = [f"  {part:<10} {mode:<7} {cls:<7} measured {m:.2e}  reference {o:.2e}  gate {g:.2e}"
             for (part, mode, cls), (m, o, g) in sorted(WORST.items())]
    print("\nbottleneck width, worst per part / path / width class (shares of max|ref64|):\n" + "\n".join(lines))


@pytest.fixture(scope="module")
def holder():
    """A module whose `_packed_mlp2` packs any two-layer MLP (as tests/test_weights_gpu.py)."""
    from bottleneck_cases import pair_module
    return pair_module(64, 1)


@contextlib.contextmanager
def nan_allocations(monkeypatch):
    """torch.empty hands out NaN-filled floating-point tensors: an element a kernel leaves unwritten shows."""
    real = torch.empty

    def empty(*args, **kwargs):
        t = real(*args, **kwargs)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    monkeypatch.setattr(torch, "empty", empty)
    try:
        yield
    finally:
        monkeypatch.setattr(torch, "empty", real)


def _spec(form, src, tdt):
    from groupnet_amd import ops
    kind = form[0]
    t = lambda x: x.to(dev()).to(tdt)
    if kind == "x":
        return t(src["x"])
    if kind == "nodeagg":
        return ops.NodeAggSpec(t(src["agg"]), t(src["ori"]))
    return ops.ScatterSpec(t(src["feat"]), None if kind == "sym" else src["H"].to(dev()), t(src["ori"]), kind == "sym")


def _launch(holder, c, forms, d, mode, xs, monkeypatch, plans, outs=None, keep=None, dh=128):
    """One ops.mlp2_grouped launch of the case's groups on the matrix path / storage `mode` with GN_MLP2_XS = xs; the plan
    of that launch is held against `closing_launch_form`.  -> the outputs."""
    from groupnet_amd import ops
    precision, dtype = mode
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    if xs is None:
        monkeypatch.delenv("GN_MLP2_XS", raising=False)
    else:
        monkeypatch.setenv("GN_MLP2_XS", xs)
    items = [(_spec(f, s, tdt), holder._packed_mlp2(m.to(dev())), None if outs is None else outs[i])
             for i, (f, s, m) in enumerate(zip(forms, c["srcs"], c["mlps"]))]
    n0 = len(plans)
    ys = _with_precision(precision, lambda: ops.mlp2_grouped(items, keep))
    torch.cuda.synchronize()
    (stem, rc, plan), = plans[n0:]
    want = closing_launch_form(forms, d, precision, dtype, xs, keep is not None, dh)
    assert stem == "gn_mlp2" and rc == 0 and (_name(plan.kernel), plan.tiles[2]) == want, (forms, d, mode, xs, _name(plan.kernel))
    assert all(y.dtype == tdt for y in ys)
    return ys


def _gate_y(part, c, ys, d, mode, what):
    """Every group's output against float64 at the case's gate -> 'measured / own / gate' of the worst group."""
    worst = None
    for y, ref, gate, own in zip(ys, c["y64"], c["gate"], c["err_ref"]):
        top = float(ref.abs().max())
        err = abs_err(y.reshape(ref.shape), ref)
        own_share = own / top if mode[1] == "bf16" else own
        _note(part, MODE_IDS[MODES.index(mode)], d, err / top, own_share, gate / top)
        if worst is None or err / gate > worst[0] / worst[2]:
            worst = (err / top, own_share, gate / top)
        assert bool(torch.isfinite(y).all()) and err <= gate, (what, d, mode, err / top, gate / top)
    return f"{d}: {worst[0]:.1e}/{worst[1]:.1e}/{worst[2]:.1e}"


def _xs_settings(mode, d):
    """Both bf16-core kernels where they run; the fp32-core kernels do not read the switch."""
    return ("0", "1") if (mode[1] == "bf16" or mode[0] != "fp32") and d <= 64 else (None,)


# ---- 1a. plain rows at every width -------------------------------------------------------------------------------------
A_CHUNKS = [D_ALL[0:16], D_ALL[16:32], D_ALL[32:48], D_ALL[48:64], D_WIDE]


@pytest.mark.parametrize("widths", A_CHUNKS, ids=[f"d{w[0]}-{w[-1]}" for w in A_CHUNKS])
@pytest.mark.parametrize("mode", MODES[:3], ids=MODE_IDS[:3])
def test_plain_rows_at_every_width(mode, widths, holder, monkeypatch):
    """69 rows (two full 32-row blocks and a ragged one), 128 -> 128 -> dout, both kernels, against float64."""
    plans, lines = [], []
    _spy_plans(monkeypatch, plans)
    for d in widths:
        c = closing_case((X_FORM,), d)
        for xs in _xs_settings(mode, d):
            ys = _launch(holder, c, (X_FORM,), d, mode, xs, monkeypatch, plans)
            assert ys[0].shape == (ROWS, d)
            lines.append(("" if xs is None else f"xs{xs} ") + _gate_y("1a rows", c, ys, d, mode, "plain rows"))
    print(f"\nplain rows {mode[0]} (measured / fp32 reference / gate, of max|ref64|): " + "; ".join(lines), end="")


def test_plain_rows_on_bf16_storage(holder, monkeypatch):
    plans, lines = [], []
    _spy_plans(monkeypatch, plans)
    mode = MODES[3]
    for d in D_IMAGE:
        c = closing_case((X_FORM,), d, True)
        for xs in ("0", "1"):
            ys = _launch(holder, c, (X_FORM,), d, mode, xs, monkeypatch, plans)
            lines.append(f"xs{xs} " + _gate_y("1a rows", c, ys, d, mode, "plain rows"))
    print(f"\nplain rows bf16 storage (measured / e_emu / gate = 4 e_emu, of max|ref64|): " + "; ".join(lines), end="")


# ---- 1b. output placement ---------------------------------------------------------------------------------------------
def _strides(d):
    """(row stride, first column) of the two placements: a stride that is a multiple of 4 (the block starts at column 4,
    16-byte aligned on fp32 storage), and one that is not (at d = 36: 38, the element branch through ldy alone)."""
    odd = d + 2 if (d + 2) % 4 else d + 3
    return ((d + 8 + 3) // 4 * 4, 4), (odd, 1)


@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_output_placement(mode, holder, monkeypatch):
    """The output as a column block of a wider tensor prefilled with a sentinel, five guard rows behind the 69: everything
    outside the block comes back bit-identical, the block equals the stand-alone result bit for bit."""
    plans, lines = [], []
    _spy_plans(monkeypatch, plans)
    tdt = torch.bfloat16 if mode[1] == "bf16" else torch.float32
    for d in PLACEMENT_D:
        c = closing_case((X_FORM,), d, mode[1] == "bf16")
        for xs in _xs_settings(mode, d):
            (alone,) = _launch(holder, c, (X_FORM,), d, mode, xs, monkeypatch, plans)
            assert alone.stride() == (d, 1)
            lines.append(_gate_y("1b placed", c, [alone], d, mode, "placement"))
            for ldy, c0 in _strides(d):
                buf = torch.full((ROWS + 5, ldy), SENTINEL, dtype=tdt, device=dev())
                before = buf.clone()
                out = buf[:ROWS, c0:c0 + d]
                (y,) = _launch(holder, c, (X_FORM,), d, mode, xs, monkeypatch, plans, outs=[out])
                assert y.data_ptr() == out.data_ptr() and out.stride(0) == ldy
                assert torch.equal(out, alone), (d, ldy, xs, "the block in place differs from the stand-alone result")
                buf[:ROWS, c0:c0 + d] = SENTINEL
                assert torch.equal(buf, before), (d, ldy, xs, "a store left its column block or its rows")
    print(f"\nplacement {MODE_IDS[MODES.index(mode)]}: strides {[_strides(d) for d in PLACEMENT_D]}; " + "; ".join(lines), end="")


# ---- 1c. input forms ----------------------------------------------------------------------------------------------------
C_FORMS = [(f,) for f in INPUT_FORMS] + [TWO_GROUPS]


@pytest.mark.parametrize("forms", C_FORMS, ids=["+".join(form_id(f) for f in fs) for fs in C_FORMS])
@pytest.mark.parametrize("mode", MODES, ids=MODE_IDS)
def test_input_forms(mode, forms, holder, monkeypatch):
    """x = cat(H^T feat, ori) / N formed inside the kernel: the unordered pairs of the pairwise graph, a top-k H with E = N
    and E = 1, E = 20 (beyond the xs kernel's 16 hyperedges: mlp2_x_kernel whatever the switch says — asserted from the
    plan), H^T feat per node, two groups in one launch."""
    plans, lines = [], []
    _spy_plans(monkeypatch, plans)
    twin = mode[1] == "bf16"
    for d in (D_EDGES if mode == MODES[2] else D_IMAGE):
        c = closing_case(forms, d, twin)
        for xs in _xs_settings(mode, d):
            ys = _launch(holder, c, forms, d, mode, xs, monkeypatch, plans)
            if mode != MODES[2] and any(form_edges(f) > 16 and f[0] == "hyper" for f in forms):
                assert _name(plans[-1][2].kernel) == "mlp2_x_kernel"
            lines.append(("" if xs is None else f"xs{xs} ") + _gate_y("1c forms", c, ys, d, mode, forms))
    print(f"\ninput forms {MODE_IDS[MODES.index(mode)]} {[form_id(f) for f in forms]}: " + "; ".join(lines), end="")


@pytest.mark.parametrize("forms", [(X_FORM,)] + C_FORMS, ids=["+".join(form_id(f) for f in fs) for fs in [(X_FORM,)] + C_FORMS])
@pytest.mark.parametrize("mode", MODES[:3], ids=MODE_IDS[:3])
def test_kept_activations(mode, forms, holder, monkeypatch):
    """keep= (training): in_out, the input rows as evaluated, and hid_out = relu(W0 x + b0), allocated from NaN, against the
    same float64 reference at the same gate; y as without them."""
    plans, lines = [], []
    _spy_plans(monkeypatch, plans)
    for d in D_EDGES:
        c = closing_case(forms, d)
        for xs in _xs_settings(mode, d):
            keep = []
            with nan_allocations(monkeypatch):
                ys = _launch(holder, c, forms, d, mode, xs, monkeypatch, plans, keep=keep)
            lines.append(_gate_y("1c keep", c, ys, d, mode, forms))
            for kd, x64, hid64 in zip(keep, c["x64"], c["hid64"]):
                ex, eh = rel_err(kd["x"], x64), rel_err(kd["hid"], hid64)
                assert bool(torch.isfinite(kd["x"]).all()) and bool(torch.isfinite(kd["hid"]).all())
                assert max(ex, eh) <= TOL_FEAT, (forms, d, mode, xs, ex, eh)
    print(f"\nkept activations {mode[0]} {[form_id(f) for f in forms]}: " + "; ".join(lines), end="")


# ---- 1d. the other exported widths -----------------------------------------------------------------------------------
@pytest.mark.parametrize("din,dh", OTHER_WIDTHS)
@pytest.mark.parametrize("mode", MODES[:3], ids=MODE_IDS[:3])
def test_other_layer_widths(mode, din, dh, holder, monkeypatch):
    """(din, dh) = (64, 128), (64, 256), (128, 256) with one and two output tiles: the instantiations of the C ABI that only
    ran on the plain kernel."""
    plans, lines = [], []
    _spy_plans(monkeypatch, plans)
    form = ("x", 0, din, 0)
    for d in OTHER_D:
        c = closing_case((form,), d, False, din, dh)
        for xs in _xs_settings(mode, d):
            ys = _launch(holder, c, (form,), d, mode, xs, monkeypatch, plans, dh=dh)
            assert list(plans[-1][2].tiles)[:2] == [din // 32, dh // 32]
            lines.append(("" if xs is None else f"xs{xs} ") + _gate_y("1d widths", c, ys, d, mode, (din, dh)))
    print(f"\n{din} -> {dh} -> dout {mode[0]}: " + "; ".join(lines), end="")


# ---- 2. the fused closing stage and its fallback ---------------------------------------------------------------------------
def _set_precision(mode, monkeypatch):
    from groupnet_amd import ops
    monkeypatch.setattr(ops, "BF16X6", ops.BF16X6)      # (restored after the test)
    monkeypatch.setattr(ops, "F16X3", ops.F16X3)
    ops.set_precision(mode)


def _gate_modules(part, case, c, res, what=""):
    """[(node_feat, factors)] of the compared scenes against the float64 oracle at the case's gates."""
    d, twin = case[1], case[6] == "bf16"
    sel = c["scenes"].to(dev())
    parts = []
    for (nf, fac), (f64, c64), (gf, gc), (of, oc) in zip(res, c["ref"], c["gate"], c["err_ref"]):
        top = float(f64.abs().max())
        ef, ec = abs_err(nf[sel], f64), abs_err(fac[sel], c64)
        own = of / top if twin else of
        _note(part, "bf16" if twin else "f16x3", d, ef / top, own, gf / top)
        parts.append(f"{ef / top:.1e}/{own:.1e}/{gf / top:.1e} fac {ec:.1e}/{oc:.1e}/{gc:.1e}")
        assert nf.shape[-1] == d and ef <= gf and ec <= gc, (module_case_id(case), what, ef / top, gf / top, ec, gc)
    return " | ".join(parts)


@pytest.mark.parametrize("case", FUSED_CASES, ids=[module_case_id(c) for c in FUSED_CASES])
def test_latency_form_takes_or_declines_the_closing_stage_by_width(case, monkeypatch):
    """fuse_closing=True on [pairwise, hyper 3, hyper N], the outputs column blocks of one (B, N, 3 d) tensor: at 33..64 the
    aggregation launch applies the closing MLP (plan.closing, no mlp2_grouped call), rows bit-identical to the forward
    with the separate launch; at 16, 32 and 96 the plan declines and the forward is the one that never asked."""
    from groupnet_amd.MS_HGNN_batch import run_message_passing
    tag, d, B, N, scales, nmp, dtype = case
    c, forms = module_case(case), module_forms(case)
    _set_precision("f16x3", monkeypatch)
    mods = [m.to(dev()).eval() for m in c["mods"]]
    hd = c["h"].to(dev())
    Hd = [None if H is None else H.to(dev()) for H in c["Hs"]]
    Ud = [[u.to(dev()) for u in per] for per in c["U"]]
    plans = []
    _spy_plans(monkeypatch, plans)
    calls = record(monkeypatch)

    def forward(fuse):
        wide = torch.full((B + 1, N, 3 * d), SENTINEL, device=dev())       # (one guard scene behind the batch)
        outs = [wide[:B, :, i * d:(i + 1) * d] for i in range(3)]
        n0, p0 = len(calls), len(plans)
        with torch.no_grad():
            res = run_message_passing(mods, [hd] * 3, Hd, Ud, outs, fuse_closing=fuse)
        torch.cuda.synchronize()
        assert all(r[0].data_ptr() == o.data_ptr() and o.stride(1) == 3 * d for r, o in zip(res, outs))
        assert bool((wide[B] == SENTINEL).all()) and bool(torch.isfinite(wide[:B]).all())
        return res, wide, calls[n0:], [p for s, rc, p in plans[p0:] if s == "gn_agg_mlp"]
    res, wide, asked, agg_plans = forward(True)
    taken = [cl[3] is not None for cl in asked if cl[0] == "agg_mlp_closing"]
    names = [cl[0] for cl in asked]
    want = 32 < d <= 64
    assert forms["fused_closing"] == want and taken == [want], (module_case_id(case), taken)
    assert ("mlp2_grouped" in names) == (not want) and [p.closing for p in agg_plans] == [int(want)]
    line = _gate_modules("2 latency", case, c, res, "asked")
    plain, wide0, never, _ = forward(False)
    assert "agg_mlp_closing" not in [cl[0] for cl in never] and "mlp2_grouped" in [cl[0] for cl in never]
    assert torch.equal(wide, wide0), "the rows of the fused closing stage (or of its fallback) differ from the separate launch's"
    assert all(torch.equal(a[1], b[1]) for a, b in zip(res, plain))
    print(f"\n{module_case_id(case)} closing {'fused' if want else 'declined'} (draw {c['draw']}; measured / fp32 oracle / gate): {line}", end="")


# ---- 3. whole modules ------------------------------------------------------------------------------------------------------
def _module_forward(case, c):
    from groupnet_amd import ops
    tag, d, B, N, scales, nmp, dtype = case
    twin = dtype == "bf16"
    mod = c["mods"][0].to(dev()).eval()
    h = c["h"].to(dev()).to(torch.bfloat16 if twin else torch.float32)
    U = [u.to(dev()) for u in c["U"][0]]
    with torch.no_grad():
        if scales[0] is None:
            nf, fac = mod(h, noise_u=U)
        elif twin:      # (the incidence is handed in: the bf16 affinity's near-ties are tests/test_bf16_gpu.py's subject)
            nf, fac, _ = mod(h, None, noise_u=U, H=c["Hs"][0].to(dev()))
        else:
            nf, fac, H = mod(h, ops.affinity(h), noise_u=U)
            assert torch.equal(H.cpu(), c["Hs"][0]), "top-k incidence differs from the oracle"
    torch.cuda.synchronize()
    assert nf.shape == (B, N, d) and nf.dtype == h.dtype
    return nf, fac


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("N", MODULE_N)
@pytest.mark.parametrize("kind", MODULE_KINDS)
def test_modules_at_every_edge_width(kind, N, dtype, monkeypatch):
    """One module through its own forward at D_EDGES (bf16 storage: up to 64), B = 3: N = 5 and 11 form the closing MLP's
    input inside its kernel, N = 20 takes the stand-alone scatter."""
    _set_precision("f16x3", monkeypatch)
    lines = []
    for case in module_cases(kind, N, dtype):
        c = module_case(case)
        forms = module_forms(case)      # (bf16 storage: the pairwise module's scene form needs no scatter)
        assert (forms["scatter"] is not None) == (N > 16 and not forms["groups"][0]["node_form"])
        lines.append(f"{case[1]}: " + _gate_modules("3 module", case, c, [_module_forward(case, c)]))
    print(f"\n{kind} N={N} {dtype} (features measured / reference's own / gate of max|ref64|, factors absolute): " + "; ".join(lines), end="")


@pytest.mark.parametrize("kind", MODULE_KINDS)
def test_two_rounds_at_other_widths(kind, monkeypatch):
    """nmp_layers = 2: only the last closing MLP has the bottleneck width (the first stays 128 -> 128 -> 64)."""
    _set_precision("f16x3", monkeypatch)
    lines = []
    for case in module_cases(kind, 11, nmp=2):
        c = module_case(case)
        assert c["mods"][0].nmp_mlps[0].layers[1].out_features == 64 and c["mods"][0].nmp_mlp_end.layers[1].out_features == case[1]
        lines.append(f"{case[1]}: " + _gate_modules("3 nmp2", case, c, [_module_forward(case, c)]))
    print(f"\n{kind} two rounds: " + "; ".join(lines), end="")


@pytest.mark.parametrize("kind", MODULE_KINDS)
def test_bf16_storage_beyond_64_is_refused_before_any_launch(kind, monkeypatch):
    """bf16 activations with bottleneck_dim > 64: ValueError naming the limit, no entry point reached (neither the
    incidence's nor the grouped launches'), a sentinel-filled `out` untouched."""
    from bottleneck_cases import hyper_module, pair_module
    from groupnet_amd import ops
    from groupnet_amd.MS_HGNN_batch import run_message_passing
    calls = record(monkeypatch)
    built = []
    real_topk = ops.topk_incidence
    monkeypatch.setattr(ops, "topk_incidence", lambda *a, **k: built.append(1) or real_topk(*a, **k))
    B, N = 3, 11
    h = torch.randn(B, N, 64, device=dev()).bfloat16()
    corr = ops.affinity(h.float())
    for d in D_WIDE:
        mod = (pair_module(d, 5) if kind == "pair" else hyper_module(d, 3, 5)).to(dev()).eval()
        out = torch.full((B, N, d), SENTINEL, dtype=torch.bfloat16, device=dev())
        with torch.no_grad(), pytest.raises(ValueError, match=r"bottleneck_dim <= 64 \(got %d\)" % d):
            mod(h, out=out) if kind == "pair" else mod(h, corr, out=out)
        with pytest.raises(ValueError, match="bottleneck_dim <= 64"):
            run_message_passing([mod], [h], [None if kind == "pair" else torch.zeros(B, N, N, device=dev())], [None], [out])
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and not calls and not built, (kind, d, [c[0] for c in calls])
    # the same module on fp32 tensors runs
    with torch.no_grad():
        nf = mod(h.float())[0] if kind == "pair" else mod(h.float(), corr)[0]
    assert nf.shape == (B, N, D_WIDE[-1]) and bool(torch.isfinite(nf).all()) and calls


# ---- 4. training ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", BACKWARD_D)
@pytest.mark.parametrize("kind", BACKWARD_KINDS)
def test_gradients_match_float64_autograd_by_width(kind, d):
    """L = <node_feat, R1> + <factors, R2> at bottleneck width d: dL/dh and every parameter gradient of the HIP training path
    against float64 autograd of the oracle — the whole batch within TOL_ANY, its clean scenes alone within TOL_CLEAN, as
    tests/test_edge_types_gpu.py (inputs: `backward_case`, chosen on the oracle alone).  The closing MLP's GEMMs take d as
    their K (dy1 = g_y W1: lda = 1 at d = 1) and as their M (dW1 = g_y^T y1)."""
    B, N = BACKWARD_SIZE
    c = backward_case(kind, d)
    mod, h, U, R1, R2, K = c["mod"], c["h"], c["U"], c["R1"], c["R2"], c["K"]
    mod.to(dev()).train()
    tag = f"{kind} d={d} B={B} N={N} (draw {c['shift']})"

    def both(rows, tol):
        r = backward_reference("pair" if kind == "pair" else "hyper", c, rows)
        for p in mod.parameters():
            p.grad = None
        x = h[rows].clone().to(dev()).requires_grad_(True)
        if kind == "pair":
            nf2, fac2 = mod(x, noise_u=[U[rows].to(dev())])
        else:
            nf2, fac2, _ = mod(x, None, noise_u=[U[rows].to(dev())], H=r["H"].to(dev()))
        assert nf2.shape == (len(rows), N, d)
        assert abs_err(nf2, r["nf"]) <= 1e-5 and abs_err(fac2, r["fac"]) <= 1e-5
        ((nf2 * R1[rows].to(dev())).sum() + (fac2 * R2[rows].to(dev())).sum()).backward()
        eh = rel_err(x.grad, r["dh"])
        assert eh <= tol, (tag, "dL/dh", eh, tol)
        hip = {k: p.grad for k, p in mod.named_parameters()}
        used = [k for k in r["grads"] if k not in r["dead"]]
        assert len(used) == 24 + 4 * K, (tag, len(used))
        ew, where = _check(hip, r["grads"], used, tol)
        for k in r["dead"]:
            assert hip[k] is None or not bool(hip[k].any()), (tag, k, "gradient of a parameter the loss does not depend on")
        assert hip["nmp_mlp_end.layers.1.weight"].shape == (d, 128) and hip["nmp_mlp_end.layers.1.bias"].shape == (d,)
        return r["probe"], eh, ew, where

    rows_all = torch.arange(B)
    probe, eh, ew, where = both(rows_all, TOL_ANY)
    clean = probe.clean()
    assert bool(clean.any()), tag
    msg = (f"\nbackward {tag}: whole batch dL/dh {eh:.1e}, worst parameter {ew:.1e} ({where}), gate {TOL_ANY:g}; "
           f"{int(clean.sum())}/{B} scenes clean (window {WINDOW:g})")
    WORST[("4 grads", kind, width_class(d))] = max(WORST.get(("4 grads", kind, width_class(d)), (0, 0, TOL_ANY)), (max(eh, ew), 0.0, TOL_ANY))
    if bool(clean.all()):
        print(msg + f"; all clean: gated at {TOL_CLEAN:g}", end="")
        assert eh <= TOL_CLEAN and ew <= TOL_CLEAN, (tag, eh, ew, where)
        return
    _, eh2, ew2, where2 = both(rows_all[clean], TOL_CLEAN)
    print(msg + f"; clean scenes alone dL/dh {eh2:.1e}, worst parameter {ew2:.1e} ({where2}), gate {TOL_CLEAN:g}", end="")
