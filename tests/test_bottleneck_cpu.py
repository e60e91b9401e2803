"""The bottleneck width on the host (no GPU): the launch rules of tests/launch_forms.py at every width, the library's
plans against them, the references of tests/test_bottleneck_gpu.py against torch.nn.functional.linear, the flaws those
references must expose, and the conditions on the inputs that the gates of the GPU tests rest on."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

from bottleneck_cases import (ALL_MODULE_CASES, BACKWARD_D, BACKWARD_KINDS, BF16_CAP, BF16_MARGIN, D_ALL, D_EDGES, D_IMAGE,
                              D_WIDE, FLAWS, FUSED_CASES, FUSED_D, INPUT_FORMS, OTHER_D, OTHER_WIDTHS, PLACEMENT_D, ROWS,
                              TOL_FAC, TOL_FEAT, TWO_GROUPS, X_FORM, backward_case, closing_case, closing_input,
                              closing_launch_form, closing_ref, form_edges, module_case, module_case_id,
                              module_forms, width_class)
from edge_type_cases import backward_reference, rel_err
from launch_forms import PLACEHOLDER, expected_forms, launch_descriptors, mlp2_form
from test_launch_plan_cpu import MODES, _ask, _name, check_plans

SIZES = ((7, 11), (400, 11), (512, 17))
GN_ERR_SHAPE = -2


# ---- the launch rules -----------------------------------------------------------------------------------------------
def test_rules_by_width():
    """The default is the width every earlier case ran (64); the fused closing stage exists for 32 < width <= 64 only; the
    closing launch runs the xs / x kernel by launch size up to 64 and mlp2_kernel beyond."""
    kw = dict(B=7, N=11, scales=[3, 11])
    assert expected_forms(**kw) == expected_forms(**kw, bottleneck=64)
    for d in set(D_EDGES) | set(FUSED_D) | {20}:
        f = expected_forms(**kw, bottleneck=d)
        assert f["fused_closing"] == (32 < d <= 64), d
        assert f["mlp2"] == (None if 32 < d <= 64 else ("mlp2_xs_kernel" if d <= 32 else "mlp2_kernel")), d
        big = expected_forms(2232, 11, [2, 5, 11], bottleneck=d)
        assert not big["fused_closing"] and big["mlp2"] == ("mlp2_x_kernel" if d <= 64 else "mlp2_kernel"), d
        assert big["mlp2_tiles"] == (0 if d > 64 else (1 if d <= 32 else 2))
        twin = expected_forms(**kw, dtype="bf16", bottleneck=d)
        assert twin["mlp2_refused"] == (d > 64) and (twin["mlp2"] is None) == (d > 64)
        # the fp32 cores: the split kernel on a small launch of plain rows (N > 16), never beyond 64
        f32 = expected_forms(64, 17, [17], "fp32", bottleneck=d)
        assert f32["mlp2"] == ("mlp2_split_kernel" if d <= 64 else "mlp2_kernel"), d
        assert expected_forms(7, 11, [3], "fp32", bottleneck=d)["mlp2"] == "mlp2_kernel"
    assert [width_class(d) for d in (1, 32, 33, 64, 65)] == ["<=32", "<=32", "33..64", "33..64", ">64"]


@pytest.mark.parametrize("precision,dtype", MODES, ids=[p if d == "fp32" else d for p, d in MODES])
def test_plans_at_every_edge_width(precision, dtype):
    """gn_agg_mlp_plan_* (with and without the closing stage) / gn_mlp2_plan_* / the graph launches of a forward whose
    closing MLP has width d against `expected_forms(..., bottleneck=d)`: D_EDGES (and 16, 20: declined closing stages)
    x three launch sizes.  bf16 storage beyond 64: gn_mlp2_plan_bf16 answers GN_ERR_SHAPE."""
    twin = dtype == "bf16"
    seen = set()
    for (B, N), d in itertools.product(SIZES, D_EDGES + (16, 20)):
        for scales in ([3, N], [N], [2, 5, N]):
            kw = dict(B=B, N=N, scales=scales, precision=precision, dtype=dtype, bottleneck=d)
            forms, desc = expected_forms(**kw), launch_descriptors(**kw)
            assert desc["mlp2"][4:6] == (d, d * (2 + len(scales))) and desc["agg_closing"][0].dout == d
            rc_c, plan_c = _ask("agg_mlp", twin, desc["agg_closing"])
            if forms["mlp2_refused"]:
                assert twin and d > 64 and _ask("mlp2", True, *desc["mlp2"])[0] == GN_ERR_SHAPE, kw
                assert rc_c != 0 and _ask("agg_mlp", True, desc["agg"])[0] == 0, kw
                seen.add("refused")
                continue
            check_plans(forms, desc, True, kw)
            # the closing stage is declined by an error code (GN_ERR_SHAPE on fp32 storage), not by a plan without it
            if forms["fused_closing"]:
                assert (rc_c, plan_c.closing) == (0, 1), (kw, rc_c)
            else:
                assert rc_c != 0 and (twin or rc_c == GN_ERR_SHAPE), (kw, rc_c)
            if not forms["fused_closing"]:
                rc, plan = _ask("mlp2", twin, *desc["mlp2"])
                assert rc == 0 and (_name(plan), plan.tiles[2]) == (forms["mlp2"], forms["mlp2_tiles"]), kw
                assert plan.precision == (0 if d > 64 or (precision == "fp32" and not twin) else (1 if twin else (2 if precision == "f16x3" else 3)))
            seen.add((forms["fused_closing"], forms["mlp2"], forms["mlp2_tiles"]))
    if twin:
        assert seen == {"refused", (False, "mlp2_xs_kernel", 1), (False, "mlp2_xs_kernel", 2)}      # (x: test_rules_by_width)
    elif precision == "fp32":
        assert {(False, "mlp2_kernel", 0), (False, "mlp2_split_kernel", 0)} <= seen and not any(s[0] for s in seen)
    else:
        assert {(True, None, None), (False, "mlp2_xs_kernel", 1), (False, "mlp2_xs_kernel", 2), (False, "mlp2_kernel", 0)} <= seen


def test_fused_closing_answers_of_the_issue():
    """[pairwise, hyper 3, hyper N] at B = 7, N = 11 on the f16x3 path: the aggregation plan takes the closing stage at
    33, 40, 63 and 64 and answers GN_ERR_SHAPE at 16, 20, 32, 65 and 96 — the widths of FUSED_CASES among them."""
    for d, want in ((16, -2), (20, -2), (32, -2), (33, 0), (40, 0), (63, 0), (64, 0), (65, -2), (96, -2)):
        for B in (7, 400):
            desc = launch_descriptors(B, 11, [3, 11], bottleneck=d)
            rc, plan = _ask("agg_mlp", False, desc["agg_closing"])
            assert rc == want and (rc != 0 or plan.closing == 1), (d, B, rc)
    for case in FUSED_CASES:
        assert module_forms(case)["fused_closing"] == (32 < case[1] <= 64), module_case_id(case)
        # B = 400: the scale-3 group has 138 row blocks (two waves per row block, scenes packed per workgroup)
        g = module_forms(case)["groups"]
        assert [x["wpr"] for x in g] == ([1, 4, 4] if case[2] == 7 else [1, 2, 4])


def _mlp2_groups(forms, keep=False, image=True, half=True):
    from groupnet_amd import _lib as L
    P = PLACEHOLDER
    gs = []
    for f in forms:
        kind, B, N, s = f
        src = dict(x=P) if kind == "x" else dict(feat=P, ori=P, E=form_edges(f), sym=int(kind == "sym"), H=P if kind == "hyper" else 0)
        gs.append(L.Mlp2Group(W=P, bias=P, y=P, Wx=P if image else 0, Wh=P if image and half else 0,
                              in_out=P if keep else 0, hid_out=P if keep else 0, **src))
    return (L.Mlp2Group * len(gs))(*gs)


def test_single_launch_plans_at_every_width(monkeypatch):
    """gn_mlp2_plan_* of one launch with the descriptors tests/test_bottleneck_gpu.py passes (`closing_launch_form`): the
    x-tensor form at every width 1..64 and beyond, every input form at D_EDGES, both settings of GN_MLP2_XS and unset,
    the four modes, with and without kept activations — the kernel, tiles[2], and the refusal of bf16 storage beyond 64."""
    n = 0
    for xs in (None, "0", "1"):
        if xs is None:
            monkeypatch.delenv("GN_MLP2_XS", raising=False)
        else:
            monkeypatch.setenv("GN_MLP2_XS", xs)
        for (precision, dtype), forms in itertools.product(MODES, [(X_FORM,)] + [(f,) for f in INPUT_FORMS] + [TWO_GROUPS]):
            twin = dtype == "bf16"
            kind, B, N, s = forms[0]
            rows = ROWS if kind == "x" else B * N
            for d, keep in itertools.product(D_ALL + D_WIDE if kind == "x" else D_EDGES, (False, True)):
                if keep and twin:
                    continue
                image = d <= 64 and (twin or precision != "fp32")       # ops.mlp2_grouped passes the images up to 64 only
                arr = _mlp2_groups(forms, keep, image, half=precision == "f16x3" and not twin)
                rc, plan = _ask("mlp2", twin, arr, rows, 128, 128, d, d, 0 if kind == "x" else N, ctypes.c_float(max(N, 1)))
                want = closing_launch_form(forms, d, precision, dtype, xs, keep)
                if want is None:
                    assert twin and d > 64 and rc in (GN_ERR_SHAPE, -1), (forms, d, rc)
                    continue
                assert rc == 0 and (_name(plan), plan.tiles[2]) == want, (forms, precision, dtype, xs, d, keep, _name(plan))
                n += 1
    assert n > 3000
    # the answers of the issue's table
    assert mlp2_form(20, ROWS, 1) == ("mlp2_xs_kernel", 1) and mlp2_form(33, ROWS, 1) == ("mlp2_xs_kernel", 2)
    assert mlp2_form(65, ROWS, 1) == ("mlp2_kernel", 0) and mlp2_form(65, ROWS, 1, dtype="bf16") is None
    assert closing_launch_form((("hyper", 3, 20, 5),), 40, "f16x3", xs="1") == ("mlp2_x_kernel", 2)      # E = 20 > 16


def test_other_widths_have_all_eight_instantiations():
    """(din, dh) of OTHER_WIDTHS x one and two output tiles: the plan names the instantiation's tiles."""
    for (din, dh), d in itertools.product(OTHER_WIDTHS + ((128, 128),), OTHER_D):
        arr = _mlp2_groups((X_FORM,))
        rc, plan = _ask("mlp2", False, arr, ROWS, din, dh, d, d, 0, ctypes.c_float(1))
        assert rc == 0 and list(plan.tiles) == [din // 32, dh // 32, 1 if d <= 32 else 2], (din, dh, d)
        assert closing_launch_form((X_FORM,), d, "f16x3", dh=dh) == (_name(plan), plan.tiles[2])


# ---- the references ---------------------------------------------------------------------------------------------------
def _closing_cases(bf16=False):
    """Every (forms, d, din, dh) the GPU file runs on this storage type."""
    widths = D_IMAGE if bf16 else D_ALL + D_WIDE
    out = [((X_FORM,), d, 128, 128) for d in (sorted(set(widths) | set(PLACEMENT_D)))]
    out += [((f,), d, 128, 128) for f in INPUT_FORMS for d in (D_IMAGE if bf16 else D_EDGES)]
    out += [(TWO_GROUPS, d, 128, 128) for d in (D_IMAGE if bf16 else D_EDGES)]
    if not bf16:
        out += [((("x", 0, din, 0),), d, din, dh) for din, dh in OTHER_WIDTHS for d in OTHER_D]
    return out


def test_references_equal_linear_layers_in_float64():
    """closing_input / closing_ref (written out as products and sums) against torch.nn.functional.linear composed in
    float64, on the chosen draw of a sample of the cases: within 1e-12."""
    worst = 0.0
    for forms, d, din, dh in _closing_cases()[::3]:
        c = closing_case(forms, d, False, din, dh)
        for f, st, src, x64, y64, hid64 in zip(forms, c["states"], c["srcs"], c["x64"], c["y64"], c["hid64"]):
            if f[0] == "x":
                x = src["x"].double()
            else:
                kind, B, N, _ = f
                ori = src["ori"].double()
                if kind == "nodeagg":
                    agg = src["agg"].double()
                elif kind == "hyper":
                    agg = torch.einsum("ben,bef->bnf", src["H"].double(), src["feat"].double())
                else:       # every ordered edge (i, j) of the pairwise graph carries half its pair row onto i and onto j
                    from edge_type_cases import pair_index
                    row = pair_index(N)[2]
                    Hord = torch.zeros(N * N, N, dtype=torch.float64)
                    e = torch.arange(N * N)
                    Hord[e, e % N] += 0.5
                    Hord[e, e // N] += 0.5
                    full = src["feat"].double()[:, row]
                    agg = torch.einsum("en,bef->bnf", Hord, full)      # (a self-loop's 0.5 + 0.5: its pair row counts once)
                x = (torch.cat((agg, ori), -1) / N).reshape(B * N, 128)
            assert rel_err(x64, x) <= 1e-12, (forms, d)
            hid = torch.relu(F.linear(x, st["layers.0.weight"].double(), st["layers.0.bias"].double()))
            y = F.linear(hid, st["layers.1.weight"].double(), st["layers.1.bias"].double())
            e = max(rel_err(hid64, hid), rel_err(y64, y))
            worst = max(worst, e)
            assert e <= 1e-12, (forms, d, e)
    print(f"\nreferences against F.linear in float64: worst {worst:.1e}")


def test_flaws_move_the_references_by_more_than_ten_gates():
    """Each flaw, put into the reference, moves some output of some case by more than 10 gates: the second output tile's
    bias dropped, the / N left out, ori and the aggregate swapped, H applied untransposed."""
    moved = {f: 0.0 for f in FLAWS}
    for forms, d, din, dh in _closing_cases():
        if din != 128 or len(forms) > 1 or d not in D_EDGES:
            continue
        c = closing_case(forms, d)
        f, st, src, y64, gate = forms[0], c["states"][0], c["srcs"][0], c["y64"][0], c["gate"][0]
        for flaw in FLAWS:
            y = closing_ref(st, closing_input(f, src, flaw=flaw), flaw=flaw)[0]
            moved[flaw] = max(moved[flaw], float((y - y64).abs().max()) / gate)
            if flaw == "bias2" and d <= 32:
                assert torch.equal(y, y64)          # (one output tile: nothing to drop)
    print("\nflaws, in gates: " + ", ".join(f"{k} {v:.1e}" for k, v in moved.items()))
    assert all(v > 10 for v in moved.values()), moved


# ---- the conditions on the inputs ------------------------------------------------------------------------------------
def test_fp32_reference_stays_within_a_third_of_the_gate():
    """Every closing-MLP case on fp32 storage finds, among its 16 seeded draws, inputs on which the fp32 CPU reference is
    within TOL_FEAT / 3 of max|ref64| (y, and the kept x and hid); decided here, without the code under test."""
    worst, by_class, draws = 0.0, {}, {}
    for forms, d, din, dh in _closing_cases():
        c = closing_case(forms, d, False, din, dh)
        e = max(c["err_ref"])
        assert e <= TOL_FEAT / 3, (forms, d, e)
        by_class[width_class(d)] = max(by_class.get(width_class(d), 0.0), e)
        draws[c["draw"]] = draws.get(c["draw"], 0) + 1
        worst = max(worst, e)
    print(f"\nfp32 reference against float64, of max|ref64| (gate / 3 = {TOL_FEAT / 3:.2e}): "
          + ", ".join(f"{k}: {v:.2e}" for k, v in sorted(by_class.items())) + f"; draws used {sorted(draws.items())}")


def test_bf16_restatement_stays_within_the_cap():
    """bf16 storage: 4 e_emu <= 1.5e-2 of max|ref64| on the chosen draw of every case, and e_emu is a real error (> 0)."""
    worst, draws = 0.0, {}
    for forms, d, din, dh in _closing_cases(bf16=True):
        c = closing_case(forms, d, True, din, dh)
        for e, gate, y in zip(c["err_ref"], c["gate"], c["y64"]):
            share = gate / float(y.abs().max())
            assert 0 < e and gate == BF16_MARGIN * e and share <= BF16_CAP, (forms, d, share)
            worst = max(worst, share)
        draws[c["draw"]] = draws.get(c["draw"], 0) + 1
    print(f"\nbf16 restatement: worst 4 e_emu = {worst:.2e} of max|ref64| (cap {BF16_CAP:g}); draws used {sorted(draws.items())}")


def test_module_cases_find_inputs_on_the_oracle_alone():
    """Whole modules (parts 2 and 3): the fp32 oracle within a third of TOL_FEAT / TOL_FAC of the float64 one — bf16
    storage: four times the bf16 restatement's error within the cap — on the chosen draw of every case."""
    worst = dict(fp32=(0.0, 0.0), bf16=(0.0, 0.0))
    draws = {}
    for case in ALL_MODULE_CASES:
        c = module_case(case)
        twin = case[6] == "bf16"
        for (ef, ec), (gf, gc), (f64, _) in zip(c["err_ref"], c["gate"], c["ref"]):
            if twin:
                ef, ec = BF16_MARGIN * ef / float(f64.abs().max()), BF16_MARGIN * ec
                assert ef <= BF16_CAP and ec <= BF16_CAP, (module_case_id(case), ef, ec)
            else:
                assert ef <= TOL_FEAT / 3 and ec <= TOL_FAC / 3, (module_case_id(case), ef, ec)
            w = worst[case[6]]
            worst[case[6]] = (max(w[0], ef), max(w[1], ec))
        draws[c["draw"]] = draws.get(c["draw"], 0) + 1
        # N = 20 takes the stand-alone scatter, but for the pairwise module's scene form on bf16 storage
        forms = module_forms(case)
        assert (forms["scatter"] is not None) == (case[3] > 16 and not (twin and case[0] == "pair")), module_case_id(case)
    print(f"\nmodules: fp32 oracle {worst['fp32'][0]:.2e} of max|ref64| / {worst['fp32'][1]:.2e} (factors); bf16 4 e_emu "
          f"{worst['bf16'][0]:.2e} / {worst['bf16'][1]:.2e}; draws used {sorted(draws.items())}")


def test_backward_cases_find_inputs_on_the_oracle_alone():
    """Every case of the GPU training test finds a draw on which the float64 oracle keeps every ReLU input beyond 1e-7 of
    zero and has a clean scene; every parameter is live (the reference's edge types) but those the forward never reaches."""
    shifts = {}
    for kind, d in itertools.product(BACKWARD_KINDS, BACKWARD_D):
        c = backward_case(kind, d)
        assert c["R1"].shape == (4, 7, d) and c["mod"].bottleneck_dim == d
        shifts[kind, d] = c["shift"]
        r = backward_reference(kind, c, torch.arange(4))
        assert bool(r["probe"].clean().any()) and r["nf"].shape == (4, 7, d)
        assert len(r["grads"]) - len(r["dead"]) == 24 + 4 * c["K"], (kind, d, r["dead"])
        assert not any("nmp_mlp_end" in k for k in r["dead"])
        assert r["grads"]["nmp_mlp_end.layers.1.weight"].shape == (d, 128)
    print(f"\nbackward cases: draws used {sorted(set(shifts.values()))}")


# ---- the storage limit ------------------------------------------------------------------------------------------------
def test_bf16_storage_beyond_64_is_refused_before_any_launch():
    """run_message_passing validates the width against the storage type before it touches a tensor: on CPU tensors (no
    launch is possible) the refusal is the width's, and it names the limit."""
    from bottleneck_cases import hyper_module, pair_module
    from groupnet_amd.MS_HGNN_batch import run_message_passing
    for d in (65, 96, 1024):
        mods = [pair_module(d, 1), hyper_module(d, 3, 2)]
        h = torch.zeros(2, 5, 64, dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="bottleneck_dim.*64"):
            run_message_passing(mods, [h, h], [None, torch.zeros(2, 5, 5)], [None, None], [None, None])
    from groupnet_amd import MS_HGNN_batch as M
    assert M.BF16_MAX_BOTTLENECK == 64
    M._check_storage_width(1024, torch.float32)
    M._check_storage_width(64, torch.bfloat16)
