"""The packed weight images of `groupnet_amd.weights` on the GPU: the matrix-by-matrix reference streams driving a
kernel, the one-launch pack plans against them, the two-part fp16 split, and the per-step repack batch of a training
step.  Needs an MI355X: `pytest -m gpu`."""
import contextlib

import pytest
import torch

from test_parity_gpu import TOL, build_modules, dev, maxerr

pytestmark = pytest.mark.gpu


def test_mlp2_shapes_and_pack():
    from groupnet_amd import MLP, ops, weights
    torch.manual_seed(3)
    for din, dh, dout, rows in [(128, 128, 64, 300), (64, 256, 64, 33), (128, 128, 1024, 70), (64, 128, 10, 129),
                                (128, 256, 7, 1)]:
        m = MLP(din, dout, hidden_size=(dh,))
        x = torch.randn(rows, din)
        l0, l1 = m.layers
        with torch.no_grad():      # plain torch fp32 layer math on the CPU as the reference of this op
            y_ref = torch.nn.functional.linear(torch.relu(torch.nn.functional.linear(x, l0.weight, l0.bias)),
                                               l1.weight, l1.bias)
        pk = dict(W=weights.pack_stream([l0.weight.detach().to(dev()), l1.weight.detach().to(dev())]),
                  bias=weights.bias_stream([l0.bias.detach().to(dev()), l1.bias.detach().to(dev())]),
                  din=din, dh=dh, dout=dout)
        y = ops.mlp2(x.to(dev()), pk)
        assert maxerr(y, y_ref) <= TOL, (din, dh, dout, rows)


def test_pack_plan_equals_matrix_by_matrix_packing():
    """The one-launch refresh of a module's packed weights (`weights.PackPlan`, gn_pack_segments_f32) writes
    bit for bit what packing matrix by matrix (gn_pack_linear_f32 + concatenation) produces — for the node,
    edge, typed-aggregation and closing MLP streams and every source of their bf16-core images (the layers' packed
    tiles in `weights.pipeline_order`, a ragged closing MLP included) — and follows in-place parameter updates."""
    import groupnet_amd as G
    from groupnet_amd import weights
    torch.manual_seed(17)
    pair, hyper = build_modules(2)
    ragged = G.MLP(128, 40, hidden_size=(128,)).to(dev())

    def pipeline(first, second):
        """Both layers packed matrix by matrix, re-ordered into A_t (rows of hidden tile t) / B_t (its columns)."""
        HT = (first.shape[0] + 31) // 32
        a = weights.pack_linear(first.detach().contiguous()).view(HT, -1)
        b = weights.pack_linear(second.detach().contiguous()).view(-1, HT, 1024)
        return torch.cat([a[t] if kind == "A" else b[:, t].reshape(-1) for kind, t in weights.pipeline_order(HT)])

    for m in (pair.to(dev()), hyper.to(dev())):
        K = m.edge_types
        for rnd in range(2):
            s0, s1 = m.node2edge_start_mlp[1].layers
            a0, a1 = m.attention_mlp[1].layers
            pk = m._packed_n2e(1)
            Wpq = torch.cat((a0.weight[:, :64], a0.weight[:, 64:]), 0).detach().contiguous()
            bpq = torch.cat((a0.bias, torch.zeros_like(a0.bias)), 0).detach()
            assert torch.equal(pk["W"], weights.pack_stream([s0.weight, s1.weight, Wpq]))
            assert torch.equal(pk["bias"], weights.bias_stream([s0.bias, s1.bias, bpq]))
            assert set(pk["xi"].src) == {"chain"}
            assert torch.equal(pk["xi"].src["chain"], torch.cat((pipeline(s0.weight, s1.weight), weights.pack_linear(Wpq))))
            st = m.nmp_mlps[1]
            i0, i1 = st.init_MLP.layers
            d0, d1 = st.MLP_distribution.layers
            f0, f1 = st.MLP_factor.layers
            Wd1 = torch.zeros(32, 256, device=dev())
            Wd1[:K, :128] = d1.weight.detach()
            Wd1[K, 128:] = f1.weight.detach()[0]
            bd1 = torch.zeros(32, device=dev())
            bd1[:K] = d1.bias.detach()
            bd1[K] = f1.bias.detach()[0]
            pk = st._packed()
            assert torch.equal(pk["W"], weights.edge_stream(i0.weight, i1.weight, torch.cat((d0.weight, f0.weight), 0).detach(), Wd1))
            assert torch.equal(pk["bias"], weights.bias_stream([i0.bias, i1.bias, torch.cat((d0.bias, f0.bias), 0), bd1]))
            assert set(pk["xi"].src) == {"edge"}
            assert torch.equal(pk["xi"].src["edge"], torch.cat((pipeline(i0.weight, i1.weight),
                                                                pipeline(torch.cat((d0.weight, f0.weight), 0), Wd1))))
            agg = m.edge_aggregation_list[0]
            l0 = [x.layers[0] for x in agg.agg_mlp]
            l1 = [x.layers[1] for x in agg.agg_mlp]
            pk = agg._packed()
            assert torch.equal(pk["W"], weights.pack_stream([w for a, b in zip(l0, l1) for w in (a.weight, b.weight)]))
            assert torch.equal(pk["b1"], torch.stack([l.bias.detach() for l in l0]))
            assert torch.equal(pk["b2"], torch.stack([l.bias.detach() for l in l1]))
            assert torch.equal(pk["W1cat"], weights.pack_linear(torch.cat([l.weight.detach() for l in l0], 0).contiguous()))
            assert torch.equal(pk["b1half"], torch.cat([l.bias.detach() for l in l0]) * 0.5)
            w2t = [weights.pack_linear(l.weight.detach().contiguous()).view(2, 4, 4, 256).permute(1, 0, 2, 3).reshape(-1) for l in l1]
            assert torch.equal(pk["W2t"], torch.cat(w2t))
            assert set(pk["xi"].src) == {"W2t", "W12", "W1cat"}
            assert torch.equal(pk["xi"].src["W2t"], torch.cat(w2t))
            assert torch.equal(pk["xi"].src["W1cat"], pk["W1cat"])
            assert torch.equal(pk["xi"].src["W12"], torch.cat([pipeline(a.weight, b.weight) for a, b in zip(l0, l1)]))
            e0, e1 = m.nmp_mlp_end.layers
            pk = m._packed_mlp2(m.nmp_mlp_end)
            assert torch.equal(pk["W"], weights.pack_stream([e0.weight, e1.weight]))
            assert torch.equal(pk["bias"], weights.bias_stream([e0.bias, e1.bias]))
            assert set(pk["xi"].src) == {"mlp2"}
            assert torch.equal(pk["xi"].src["mlp2"], pipeline(e0.weight, e1.weight))
            r0, r1 = ragged.layers
            pk = m._packed_mlp2(ragged)
            assert torch.equal(pk["W"], weights.pack_stream([r0.weight, r1.weight]))
            assert torch.equal(pk["xi"].src["mlp2"], pipeline(r0.weight, r1.weight))
            with torch.no_grad():          # in-place update (an optimizer step): the next access re-packs
                for p in list(m.parameters()) + list(ragged.parameters()):
                    p.add_(torch.randn_like(p) * 0.1)


def test_split_fp16_image_layout_and_flag():
    """gn_split_bf16_f32 with parts = 2: hi + lo reproduces every weight to 2^-22 relative (2^-25 absolute below the
    fp16 normal range), pieces in the (sub-step, part, lane, j) order of the bf16 images, flag word zero unless a
    weight exceeds the fp16 range."""
    from groupnet_amd import weights
    torch.manual_seed(5)
    packed = (torch.randn(6 * 1024, device=dev()) * torch.logspace(-6, 2, 6 * 1024, device=dev())).contiguous()
    img = weights.split_bf16(packed, parts=2)
    n = 6 * 2 * 2 * 64 * 8
    assert img.numel() == n + 8 and int(img[n:].abs().sum()) == 0
    parts = img[:n].view(torch.float16).view(6, 2, 2, 64, 8).float()          # (tile, half, part, lane, j)
    ref = weights.split_bf16(packed, parts=3).view(torch.bfloat16).view(6, 2, 3, 64, 8).float().sum(2)   # same element order
    got = parts.sum(2)
    err = (got - ref).abs()
    assert float((err / ref.abs().clamp_min(2.0 ** -3)).max()) <= 2.0 ** -21
    bad = packed.clone()
    bad[100] = 7.0e4
    img2 = weights.split_bf16(bad, parts=2)
    assert int(img2[n:].view(torch.int32)[0]) != 0


def test_repack_scope_two_launches_equal_the_per_plan_refreshes():
    """weights.repack_scope (what GraphedTrainStep wraps every step in): the first step records the pack plans / bf16-core
    images a training step touches, later steps rebuild ALL of them with two launches up front and skip the recorded
    per-plan launches.  Two blocks with identical weights take the same three SGD steps (the second and third step see
    parameters rewritten through `.data`, the case the per-step refresh exists for) — one inside the scope, one without:
    identical losses and parameters, bit for bit, and the scoped block's later steps really were served by the batch."""
    import copy
    from groupnet_amd import weights
    from groupnet_amd.multiscale import MultiScaleHGNN
    import groupnet_amd as G
    dev = lambda: torch.device("cuda:0")
    torch.manual_seed(31)
    a = MultiScaleHGNN([2, 5]).to(dev()).train()
    b = copy.deepcopy(a)
    B, N = 6, 7
    f = torch.randn(B, N, 64, device=dev())
    tgt = torch.randn(B, N, a.out_features, device=dev())
    U = [[torch.rand(s, device=dev())] for s in a.noise_shapes(B, N)]
    holder = {}
    calls = {"pack": 0}
    orig = weights.PackPlan.refresh

    def counting(self):
        before = weights._REPACK["done_plans"]
        if not (before is not None and id(self) in before):
            calls["pack"] += 1
        return orig(self)

    losses = {"a": [], "b": []}
    weights.PackPlan.refresh = counting
    try:
        for step in range(3):
            for name, blk in (("a", a), ("b", b)):
                ctx = weights.repack_scope(holder) if name == "a" else contextlib.nullcontext()
                calls["pack"] = 0
                with ctx:
                    out, _ = blk(f, noise_u=U)
                    loss = ((out - tgt) ** 2).mean()
                    blk.zero_grad(set_to_none=True)
                    loss.backward()
                if name == "a" and step > 0:
                    assert calls["pack"] == 0, "a recorded plan took its own refresh launch"
                if name == "b":
                    assert calls["pack"] > 0
                with torch.no_grad():
                    for p in blk.parameters():
                        if p.grad is not None:
                            p.data.add_(p.grad, alpha=-0.05)       # behind autograd's back: no version bump
                losses[name].append(float(loss.detach()))
    finally:
        weights.PackPlan.refresh = orig
    assert holder.get("batch") is not None and len(holder["batch"].plans) > 4
    print(f"\nrepack_scope: {len(holder['batch'].plans)} plans / {len(holder['batch'].splits)} images per step in two launches; "
          f"losses {losses['a']}")
    assert losses["a"] == losses["b"]
    assert losses["a"][2] != losses["a"][0]
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)
