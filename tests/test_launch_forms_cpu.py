"""CPU checks of tests/launch_forms.py: the sampled float64 oracle is the full-batch oracle's rows, it agrees with the
fp32 oracle, and the GPU file's case table reaches every kernel form `expected_forms` can return."""
import torch

from launch_forms import (BACKWARD_CASES, FORWARD_CASES, block64, case_forms, clean_scenes, expected_forms, hyper64,
                          hyper_incidence, pairwise64, sample_scenes, state64)
from relu_probe import relu_probe
from oracle import ms_hgnn_oracle as O


def _modules(scales, nmp, seed):
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(seed)
    blk = MultiScaleHGNN(scales, nmp_layers=nmp)
    sp = {k: v.detach().clone() for k, v in blk.interaction.state_dict().items()}
    shs = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in blk.interaction_hyper]
    return blk, sp, shs


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def test_sampled_float64_oracle_equals_the_full_batch_rows():
    """B = 37, N = 7, scales {2, 3, 7}, nmp 1 and 2: the sampled oracle (noise sliced to the sample) against the rows of
    the float64 oracle of the whole batch, and both within 1e-5 of the fp32 oracle."""
    B, N, scales = 37, 7, [2, 3, 7]
    for nmp in (1, 2):
        blk, sp, shs = _modules(scales, nmp, seed=40 + nmp)
        h = torch.randn(B, N, 64)
        Up = [torch.rand(B, N * N, 6) for _ in range(nmp)]
        Uh = [[torch.rand(*shp) for _ in range(nmp)] for shp in blk.noise_shapes(B, N)[1:]]
        scenes = sample_scenes(B, N, expected_forms(B, N, scales), n=12, seed=3)
        assert 0 in scenes.tolist() and B - 1 in scenes.tolist() and len(scenes) == 12
        # full-batch float64 oracle
        corr = O.affinity(h)
        full_p, full_pf = O.ms_hgnn_pairwise_forward(state64(sp), h.double(), [u.double() for u in Up], nmp,
                                                     decomposed=True)
        full_h = [O.ms_hgnn_hyper_forward(state64(st), h.double(), corr.double(), s, [u.double() for u in U], nmp,
                                          decomposed=True) for st, s, U in zip(shs, scales, Uh)]
        # sampled
        nf, fac = pairwise64(sp, h, Up, scenes, nmp, chunk=5)
        assert nf.dtype == torch.float64
        assert _rel(nf, full_p[scenes]) <= 1e-12 and _rel(fac, full_pf[scenes]) <= 1e-12
        for (fnf, ffac, fH), st, s, U in zip(full_h, shs, scales, Uh):
            H = hyper_incidence(h, scenes, s)
            assert torch.equal(H.double(), fH[scenes])
            nf, fac = hyper64(st, h, H, U, scenes, nmp, chunk=4)
            assert _rel(nf, fnf[scenes]) <= 1e-12 and _rel(fac, ffac[scenes]) <= 1e-12
        out, facs = block64(sp, shs, scales, h, None, Up, Uh, scenes, nmp)
        want = torch.cat([h.double(), full_p] + [x[0] for x in full_h], dim=-1)[scenes]
        assert _rel(out, want) <= 1e-12
        # float64 against the fp32 oracle (nmp = 1: the block entry point)
        if nmp == 1:
            ref32, H32, _ = O.ms_hgnn_multiscale_forward(sp, shs, scales, h, Up, Uh, decomposed=True)
            err = float((out - ref32[scenes].double()).abs().max())
            print(f"\nfloat64 sampled oracle vs fp32 oracle: {err:.1e}")
            assert err <= 1e-5
            assert len(facs) == 1 + len(scales) and all(f is not None for f in facs)


def test_expected_forms_switch_points():
    """The launch sizes at which the rules of the issue change form (N = 11, scales {2,5,11})."""
    wpr = lambda B, i: expected_forms(B, 11, [2, 5, 11])["groups"][i]["wpr"]
    assert (wpr(369, 1), wpr(370, 1), wpr(2231, 1), wpr(2232, 1)) == (4, 2, 2, 1)
    assert (wpr(4064, 3), wpr(4065, 3), wpr(24544, 3), wpr(24545, 3)) == (4, 2, 2, 1)
    f = expected_forms(512, 11, [2, 5, 11])
    assert f["fused_closing"] and [g["spw"] for g in f["groups"][1:]] == [5, 5, 14]
    assert expected_forms(2231, 11, [2, 5, 11])["fused_closing"]
    assert not expected_forms(2232, 11, [2, 5, 11])["fused_closing"]
    assert not expected_forms(512, 11, [2, 5, 11], precision="fp32")["fused_closing"]
    assert not expected_forms(512, 17, [2, 5, 17])["fused_closing"]


def test_case_table_reaches_every_form():
    seen = {k: set() for k in ("wpr_E11", "wpr_E1", "fused", "mlp2", "n2e", "twin_scene_form", "gather_spw", "agg")}
    for c in FORWARD_CASES + BACKWARD_CASES:
        f = case_forms(c)
        for g in f["groups"]:
            if g["name"] != "pair" and g["E"] == 11:
                seen["wpr_E11"].add(g["wpr"])
            if g["name"] != "pair" and g["E"] == 1:
                seen["wpr_E1"].add(g["wpr"])
            if g["name"] == "pair" and c["dtype"] == "bf16":
                seen["twin_scene_form"].add((c["N"] <= 64, g["node_form"]))
        seen["fused"].add(f["fused_closing"])
        seen["agg"].add(f["agg_kernel"])
        for k in ("mlp2", "n2e", "gather_spw"):
            if f[k] is not None:
                seen[k].add(f[k])
    print("\n", seen)
    assert seen["wpr_E11"] == {1, 2, 4} and seen["wpr_E1"] == {1, 2, 4}
    assert seen["fused"] == {True, False}
    assert {"mlp2_xs_kernel", "mlp2_x_kernel"} <= seen["mlp2"]
    assert seen["n2e"] == {"banded", "rows"}
    assert seen["twin_scene_form"] == {(True, True), (False, False)}
    assert {1, 4} <= seen["gather_spw"]
    assert {"agg_x_kernel", "agg_mlp_kernel", "agg_rb2_kernel"} <= seen["agg"]
    # the sampler keeps its size and the first / last scene at every forward size
    for c in FORWARD_CASES:
        s = sample_scenes(c["B"], c["N"], case_forms(c), n=48)
        assert len(s) == min(48, c["B"]) and int(s[0]) == 0 and int(s[-1]) == c["B"] - 1
        assert bool((s[1:] > s[:-1]).all())


def test_clean_scenes_does_not_depend_on_the_chunking():
    """The probe sees only ReLU inputs whose batch is its own: per-chunk probes must give the verdict of one probe over
    the whole sample (a probe over chunked oracle calls would see nothing and call every scene clean)."""
    B, N, scales = 37, 9, [2, 4, 9]
    blk, sp, shs = _modules(scales, 1, seed=77)
    h = torch.randn(B, N, 64)
    noise = [[torch.rand(shp)] for shp in blk.noise_shapes(B, N)]
    scenes = sample_scenes(B, N, expected_forms(B, N, scales), n=20, seed=1)
    Hs = [hyper_incidence(h, scenes, s) for s in scales]
    with torch.no_grad(), relu_probe(len(scenes)) as probe:
        block64(sp, shs, scales, h, Hs, noise[0], noise[1:], scenes)
    want = probe.clean()
    assert probe.units > 0 and 0 < int(want.sum()) < len(scenes)
    for chunk in (1, 3, 20):
        assert torch.equal(clean_scenes(sp, shs, scales, h, Hs, noise[0], noise[1:], scenes, chunk=chunk), want)
    hyper_only = clean_scenes(sp, shs, scales, h, Hs, noise[0], noise[1:], scenes, with_pair=False, chunk=7)
    assert bool((hyper_only | ~want).all())      # fewer ReLU units: every clean scene stays clean
