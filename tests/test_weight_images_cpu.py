"""The tables, references and input searches of tests/test_weight_images_gpu.py (the range flag of the fp16 weight
images), without a GPU: every `image_flag(` call site of the kernels and every image name of the packers has a site in
the table, the table's forms are forms the launchers have, its image sizes are the packers', every case's inputs are
found on the references alone, and the flag predicate is restated in numpy."""
import math
import os
import re

import numpy as np
import pytest
import torch

import bottleneck_cases as BC
import edge_type_cases as EC
import weight_image_cases as W
from launch_forms import expected_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_image_flag_call_site_has_a_site():
    """The call sites are counted in the source text: a new reader of a flag word cannot arrive untested."""
    src = open(os.path.join(ROOT, "groupnet_amd", "csrc", "gn_mlp_bf16.hpp")).read()
    calls = [m.group(1) for m in re.finditer(r"ovf\.wf \|= image_flag\((.*)\);", src)]
    assert len(calls) == src.count("image_flag(") - 1 == 7, calls      # (less the definition)
    assert sorted(calls) == sorted(W.CALL_SITES), calls
    covered = {s.call_site for s in W.SITES}
    assert covered == set(W.CALL_SITES.values()), set(W.CALL_SITES.values()) - covered


def _cpu_packers():
    from groupnet_amd import weights
    from groupnet_amd.MS_HGNN_batch import _two_layer
    m = EC.pair_module(4, 1)
    plan = lambda: weights.PackPlan(torch.device("cpu"))
    h, a = m.nmp_mlp_start, m.edge_aggregation_list[0]
    return 4, dict(
        node_chain=weights.node_chain(plan(), _two_layer(m.node2edge_start_mlp[0]), _two_layer(m.attention_mlp[0])),
        edge_mlp=weights.edge_mlp(plan(), _two_layer(h.init_MLP), _two_layer(h.MLP_distribution), _two_layer(h.MLP_factor)),
        typed_agg=weights.typed_agg(plan(), [x.layers[0] for x in a.agg_mlp], [x.layers[1] for x in a.agg_mlp]),
        closing_mlp=weights.closing_mlp(plan(), *_two_layer(m.nmp_mlp_end)))


def test_every_image_name_has_a_site_and_the_table_knows_its_size():
    """The packers on a CPU PackPlan (no launch): every name in their XImages.src is in the table, and where the table has
    the image at these widths its sub-step count — where the kernel looks for the flag word — is the packed size."""
    K, packers = _cpu_packers()
    listed = {(s.packer, s.image) for s in W.SITES}
    for packer, pk in packers.items():
        for name, src in pk["xi"].src.items():
            assert (packer, name) in listed, (packer, name)
            sub = src.numel() // 1024 * 2
            like = [s for s in W.SITES if (s.packer, s.image) == (packer, name)]
            sizes = {s._replace(p=tuple((k, (K if k == "K" else 64 if k == "dout" else v)) for k, v in s.p)).substeps() for s in like
                     if dict(s.p).get("din", 128) == 128 and dict(s.p).get("dh", 128) == 128}
            assert sizes == {sub}, (packer, name, sizes, sub)
    assert {s.packer for s in W.SITES} == set(packers)


def test_the_table_lists_forms_the_launchers_have():
    for s in W.SITES:
        if s.kind == "agg":
            want = EC.agg_launch_forms(W.AGG_FORMS[s["form"]], s["K"], "f16x3")
            assert want["kernel"] == "agg_x_kernel" and want["node_form"] == (s["form"] == "pair-node"), s.id
            assert s["form"] != "pair-node" or s["K"] <= EC.NODE_FORM_MAX_K, s.id
            assert (s.image == "W2t") == s["form"].startswith("pair") and s.substeps() == s["K"] * (16 if s.image == "W2t" else 32)
        elif s.kind == "w1cat":
            assert s["K"] <= EC.NODE_FORM_MAX_K and s.substeps() == 16 * s["K"], s.id
        elif s.kind == "fused":
            forms = expected_forms(W.B, s["N"], [3], "f16x3", types=(6, 10), bottleneck=s["dout"])
            assert forms["fused_closing"] and forms["groups"][0]["node_form"], s.id
        elif s.kind == "mlp2":
            for keep in (False, True):
                got = BC.closing_launch_form((s["form"],), s["dout"], "f16x3", "fp32", s["xs"], keep, s["dh"])
                assert got == (W.MLP2_KERNELS[s["xs"]], 1 if s["dout"] <= 32 else 2), (s.id, got)
            assert s["form"][0] == "x" or s["din"] == 128, s.id          # (the fused scatter feeds a 128-wide MLP)
            assert s.call_site + "_kernel" == W.MLP2_KERNELS[s["xs"]]
    assert {s["K"] for s in W.SITES if s.kind == "w1cat"} == set(W.W1CAT_K)
    for form in ("eo", "gather", "pair"):
        assert {s["K"] for s in W.SITES if s.kind == "agg" and s["form"] == form} == set(W.AGG_K)
    assert {s["K"] for s in W.SITES if s.kind == "agg" and s["form"] == "pair-node"} == {K for K in W.AGG_K if K <= 12}
    assert all(W.SITE[i].kind in ("node", "edge", "mlp2") for i in W.KEEP_SITES)


def test_sources_are_the_weights_the_table_names():
    """`Site.feeds` against the layers `sources` hands out (their shapes), and every position lies in one of them."""
    for s in W.SITES:
        mods, inp = W.modules(s), W.inputs(s, 0)
        src = W.sources(s, mods)
        per_type = s["K"] if s.packer == "typed_agg" and "K" in dict(s.p) else 1
        assert len(src) == len(s.feeds) * per_type, s.id
        for p in W.positions(s, mods, inp):
            assert any(p.lin is l for l in src) and 0 <= p.r < p.lin.out_features and 0 <= p.c < p.lin.in_features, (s.id, p.label)
            assert set(W.images_flagged(s, p)) >= {s.image}, (s.id, p.label)
        labels = [p.label for p in W.positions(s, mods, inp)]
        assert labels[0] in ("first", "last") and len(set(labels)) == len(labels)


@pytest.mark.parametrize("kind", sorted({s.kind for s in W.SITES}))
def test_inputs_are_found_on_the_references_alone(kind):
    """Every case of the GPU file: a draw exists on which the fp32 CPU reference is within a third of the gate."""
    worst = {}
    for s in (x for x in W.SITES if x.kind == kind):
        for pos, value, _ in [(None, None, False)] + W.cases_of(s):
            c = W.case(s, pos, value)
            assert c["draw"] < W.DRAWS
            for n, (own, third) in c["own"].items():
                assert own <= third, (s.id, pos, value, n, own)
                worst[n] = max(worst.get(n, 0.0), own / third)
            if value is not None and math.isfinite(value):
                assert float(c["pos"].lin.weight.detach()[c["pos"].r, c["pos"].c]) == value
                for n in W.gated(s):       # (the tamed product keeps the outputs ordinary)
                    assert float(c["ref64"][n].abs().max()) < 1e3, (s.id, pos, value, n)
    print(f"\n{kind}: worst fp32 reference error as a share of a third of its gate: " + ", ".join(f"{n} {v:.2f}" for n, v in worst.items()), end="")


def test_flag_predicate_restated():
    """`!(fabsf(x) <= 65000.f)` in numpy fp32 against the expected flag of every listed value; NaN flags."""
    for value, flags in W.WEIGHT_VALUES + W.LIFE_VALUES:
        x = np.float32(value)
        assert float(x) == value or math.isnan(value)          # (every listed value is an fp32 number)
        assert bool(~(np.abs(x) <= np.float32(W.FLAG_LIMIT))) == flags == W.flag_expected(value), value
    assert np.float32(65001.0) <= np.float32(65504.0)          # (fp16 holds it: the flag is stricter than the format)
