"""Ragged batches on the device ("Ragged batches"): every stage that reads the per-scene agent count,
and whole modules, against the per-scene oracle of tests/ragged_cases.py — the existing CPU oracle run on each scene at
its own size.  Padded input rows hold finite garbage (N(0,1) x 100 for features and affinities, arbitrary values in
[0, 1) for the noise), padded positions of every output must be exactly zero, and counts that all equal N must give the
bits of the call without counts.

Gates.  fp32 storage: 1e-5 absolute against the float64 oracle (the project's gate; default-init outputs are of order
0.2); affinities 2e-6 (tests/test_parity_gpu.py); incidences bit for bit (the cases keep every selection 2e-5 apart:
tests/test_ragged_cpu.py).  bf16 storage: the twins' gate of tests/test_bf16_gpu.py, TOL_ORACLE = 8e-3 of the module's
largest oracle feature, against the oracle fed the bf16-rounded features; factors TOL_ORACLE absolute.
"""
import contextlib

import pytest
import torch

import ragged_cases as C
from conftest import load_case, load_state
from oracle import ms_hgnn_oracle as O
from test_bf16_gpu import TOL_ORACLE

pytestmark = pytest.mark.gpu

FUSED = [c for c in C.CASES if c["N"] <= 112]          # the fused tile at D = 64
IDS = lambda cs: [c["id"] for c in cs]


def dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def precision(mode):
    from groupnet_amd import ops
    old = ops.precision()
    ops.set_precision(mode)
    try:
        yield
    finally:
        ops.set_precision(old)


def maxerr(a, ref):
    return float((a.detach().cpu().double() - ref.double()).abs().max()) if ref.numel() else 0.0


def pair_row(i, j, N):
    """Row of the unordered pair {i, j} in the symmetric form."""
    i, j = min(i, j), max(i, j)
    return i * N - i * (i - 1) // 2 + (j - i)


# ---------------------------------------------------------------------------------------------------------------------
# incidence
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", FUSED, ids=IDS(FUSED))
def test_fused_affinity_topk_of_a_ragged_batch(case, dtype):
    from groupnet_amd import ops
    bf16 = dtype == "bf16"
    B, N, scales, counts = case["B"], case["N"], case["scales"], case["counts"]
    h, _ = C.inputs(case, bf16=bf16)
    x = C.with_garbage(case, h).to(dev())
    x = x.bfloat16() if bf16 else x
    final = torch.zeros(B, N, 128, dtype=x.dtype, device=dev())
    with torch.no_grad():
        corr, Hs, H_cat = ops.affinity_topk(x, scales, want_corr=True, f_out=final[..., :64], want_H_cat=True,
                                            n_agents=torch.tensor(counts))
    want_H = [C.padded_incidence(case, h, s) for s in scales]
    for s, H, W in zip(scales, Hs, want_H):
        assert H.dtype == torch.float32 and torch.equal(H.cpu(), W), f"scale {s}"
    assert H_cat.dtype == x.dtype and torch.equal(H_cat.float().cpu(), torch.cat(want_H, dim=1))
    assert torch.equal(final[..., :64], x) and not final[..., 64:].any()
    want_c = C.padded_corr(case, h)
    got_c = corr.cpu()
    for b, n in enumerate(counts):
        assert not got_c[b, n:].any() and not got_c[b, :, n:].any()
    print(f"\n{case['id']} {dtype}: corr error {maxerr(got_c, want_c):.2e} (gate {C.TOL_CORR:g})")
    assert maxerr(got_c, want_c) <= C.TOL_CORR
    # no scene padded: the call without counts, bit for bit
    with torch.no_grad():
        a = ops.affinity_topk(x, scales, want_corr=True, want_H_cat=True, n_agents=[N] * B)
        b = ops.affinity_topk(x, scales, want_corr=True, want_H_cat=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(torch.equal(p, q) for p, q in zip(a[1], b[1]))


@pytest.mark.parametrize("case", C.CASES, ids=IDS(C.CASES))
def test_banded_topk_of_a_ragged_batch(case):
    """The stand-alone top-k on a caller's corr whose padded rows and columns hold garbage."""
    import groupnet_amd as G
    from groupnet_amd import ops
    B, N, scales, counts = case["B"], case["N"], case["scales"], case["counts"]
    h, _ = C.inputs(case)
    corr = C.garbage_corr(case, C.padded_corr(case, h)).to(dev())
    with torch.no_grad():
        Hs = ops.topk_incidence(corr, scales, n_agents=counts)
        for s, H in zip(scales, Hs):
            assert torch.equal(H.cpu(), C.padded_incidence(case, h, s)), f"scale {s}"
        hyper = G.MS_HGNN_hyper(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=1,
                                scale=scales[0])
        assert torch.equal(hyper.init_adj_attention(corr, corr, scales[0], n_agents=counts), Hs[0])
        full = ops.topk_incidence(corr, scales)
        assert all(torch.equal(p, q) for p, q in zip(ops.topk_incidence(corr, scales, n_agents=[N] * B), full))
        assert not all(torch.equal(p, q) for p, q in zip(Hs, full))


# ---------------------------------------------------------------------------------------------------------------------
# node -> edge
# ---------------------------------------------------------------------------------------------------------------------
def _node_rows(mod, x):
    from groupnet_amd import ops
    pk = mod._packed_n2e(0)
    xp, pq = ops.node_mlp(x, pk)
    return xp, pq, pk["w2"], pk["b2"]


N2E_FORMS = [(c, f) for c in C.CASES for f in ("banded", "rows", "pair", "pair-sym")
             if not (c["N"] > 64 and f == "rows")]              # the row form ends at N = 64


@pytest.mark.parametrize("case,form", N2E_FORMS, ids=[f"{c['id']}-{f}" for c, f in N2E_FORMS])
def test_node2edge_of_a_ragged_batch(case, form, monkeypatch):
    """Hyper groups (every scale in one launch) in the banded and the row form, the pairwise graph ordered and sym."""
    from groupnet_amd import ops
    B, N, scales, counts = case["B"], case["N"], case["scales"], case["counts"]
    blk, sp, shs = C.cpu_block(case)
    blk = blk.to(dev()).eval()
    h, _ = C.inputs(case)
    x = C.with_garbage(case, h).to(dev())
    bad = []
    with torch.no_grad():
        if form in ("banded", "rows"):
            monkeypatch.setenv("GN_N2E_ROWS", "1" if form == "rows" else "0")
            Hs = [C.padded_incidence(case, h, s) for s in scales]
            items = [_node_rows(m, x) for m in blk.interaction_hyper]
            items = [(xp, pq, H.to(dev()), w2, b2) for (xp, pq, w2, b2), H in zip(items, Hs)]
            got = ops.node2edge_grouped(items, n_agents=counts)
            for s, st, H, g in zip(scales, shs, Hs, got):
                g = g.cpu()
                for b, n in enumerate(counts):
                    Hb = C.scene_incidence(C.scene_corr(h, b, n), s, N)
                    ref = C.node2edge64(st, h[b:b + 1, :n], Hb)
                    err = maxerr(g[b, :ref.shape[0]], ref)
                    if err > C.TOL or g[b, ref.shape[0]:].any():
                        bad.append((s, b, n, err))
            same = ops.node2edge_grouped(items, n_agents=[N] * B)
            assert all(torch.equal(p, q) for p, q in zip(same, ops.node2edge_grouped(items)))
        else:
            sym = form == "pair-sym"
            xp, pq, w2, b2 = _node_rows(blk.interaction, x)
            g = ops.node2edge(xp, pq, None, w2, b2, sym=sym, n_agents=counts).cpu()
            for b, n in enumerate(counts):
                ref = C.node2edge64(sp, h[b:b + 1, :n], O.pairwise_incidence(n, 1))      # (n*n, 64), edge i*n + j
                if sym:
                    rows = torch.tensor([pair_row(i, j, N) for i in range(n) for j in range(i, n)])
                    ref = ref[torch.tensor([i * n + j for i in range(n) for j in range(i, n)])]
                else:
                    rows = C.pair_index(N, n)
                pad = torch.ones(g.shape[1], dtype=torch.bool)
                pad[rows] = False
                err = maxerr(g[b, rows], ref)
                if err > C.TOL or g[b, pad].any():
                    bad.append((b, n, err))
            assert torch.equal(ops.node2edge(xp, pq, None, w2, b2, sym=sym, n_agents=[N] * B),
                               ops.node2edge(xp, pq, None, w2, b2, sym=sym))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------
# scatter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("divisor", [None, 1.0], ids=["own-count", "one"])
@pytest.mark.parametrize("case", C.BLOCK_CASES, ids=IDS(C.BLOCK_CASES))
def test_scatter_of_a_ragged_batch(case, divisor):
    """One launch over the pairwise graph (sym and ordered) and every hyper scale, against the float64 definition
    cat(H^T feat, ori) / divisor of each scene alone."""
    from groupnet_amd import ops
    B, N, scales, counts = case["B"], case["N"], case["scales"], case["counts"]
    h, _ = C.inputs(case)
    ori = C.with_garbage(case, h)
    gen = torch.Generator().manual_seed(5 + case["seed"])
    Es = [N * (N + 1) // 2, N * N] + [C.n_edges(N, s) for s in scales]
    feats = []
    for i, E in enumerate(Es):              # N(0,1) where a scene reads, x 100 where it must not
        f = torch.randn(B, E, 64, generator=gen)
        for b, n in enumerate(counts):
            rows = (torch.tensor([pair_row(a, j, N) for a in range(n) for j in range(a, n)]) if i == 0 else
                    C.pair_index(N, n) if i == 1 else torch.arange(min(n, E)))
            pad = torch.ones(E, dtype=torch.bool)
            pad[rows] = False
            f[b, pad] *= 100.0
        feats.append(f)
    Hs = [None, None] + [C.padded_incidence(case, h, s) for s in scales]
    od = ori.to(dev())
    items = [(f.to(dev()), None if H is None else H.to(dev()), od, i == 0) for i, (f, H) in enumerate(zip(feats, Hs))]
    with torch.no_grad():
        outs = [o.cpu() for o in ops.agg_scatter_grouped(items, divisor, n_agents=counts)]
    bad = []
    for i, (f, H, out) in enumerate(zip(feats, Hs, outs)):
        for b, n in enumerate(counts):
            d = float(n) if divisor is None else divisor
            fd = f[b].double()
            if H is not None:
                agg = H[b, :, :n].double().t() @ fd
            elif i == 0:
                agg = torch.stack([sum(fd[pair_row(a, j, N)] for j in range(n)) for a in range(n)])
            else:
                agg = torch.stack([sum(fd[a * N + j] + fd[j * N + a] for j in range(n)) for a in range(n)])
            err = maxerr(out[b, :n, :64], agg / d)
            exact = torch.equal(out[b, :n, 64:], ori[b, :n] / d)            # true division
            if err > C.TOL or not exact or out[b, n:].any():
                bad.append((i, b, n, err, exact))
    assert not bad, bad
    if divisor is None:
        with torch.no_grad():
            assert all(torch.equal(p, q) for p, q in zip(ops.agg_scatter_grouped(items, n_agents=[N] * B),
                                                         ops.agg_scatter_grouped(items)))


def test_zero_padding_launch():
    """Node rows in a column block of a wider tensor, bf16 hyperedge rows, ordered pair rows and a matrix per scene:
    padded positions become zeros, everything else keeps its bits."""
    from groupnet_amd import ops
    case = C.BY_ID["n7"]
    B, N, counts = case["B"], case["N"], case["counts"]
    wide = torch.randn(B, N, 192, device=dev())
    col = wide[..., 64:128]
    fac = torch.rand(B, N, 9, device=dev()).bfloat16()            # 18-byte rows: 2-byte stores
    one = torch.rand(B, 1, 10, device=dev())
    pairs = torch.rand(B, N * N, 6, device=dev())
    mat = torch.randn(B, N, N, device=dev())
    mat16 = torch.randn(B, N, N, device=dev()).bfloat16()
    pairs16 = torch.rand(B, N * N, 5, device=dev()).bfloat16()
    before = [t.clone() for t in (wide, fac, one, pairs, mat, mat16, pairs16)]
    held = ops.agent_counts(counts, B, N, dev())
    ops.zero_padding([(col, ops.ZERO_NODE_ROWS), (fac, ops.ZERO_EDGE_ROWS), (one, ops.ZERO_EDGE_ROWS),
                      (pairs, ops.ZERO_PAIR_ROWS), (mat, ops.ZERO_PAIR_ROWS), (mat16, ops.ZERO_PAIR_ROWS),
                      (pairs16, ops.ZERO_PAIR_ROWS)], held)
    want = [t.clone() for t in before]
    for b, n in enumerate(counts):
        want[0][b, n:, 64:128] = 0
        want[1][b, n:] = 0
        keep = torch.zeros(N, N, dtype=torch.bool, device=dev())
        keep[:n, :n] = True
        want[3][b][~keep.reshape(-1)] = 0
        want[4][b][~keep] = 0
        want[5][b][~keep] = 0
        want[6][b][~keep.reshape(-1)] = 0
    for got, w in zip((wide, fac, one, pairs, mat, mat16, pairs16), want):
        assert torch.equal(got, w)
    with pytest.raises(ValueError):
        ops.zero_padding([(mat.half(), ops.ZERO_PAIR_ROWS)], held)
    with pytest.raises(ValueError):
        ops.zero_padding([(col, ops.ZERO_PAIR_ROWS)], held)
    with pytest.raises(ValueError):
        ops.zero_padding([(col, ops.ZERO_NODE_ROWS)], counts)


# ---------------------------------------------------------------------------------------------------------------------
# whole block
# ---------------------------------------------------------------------------------------------------------------------
# form: "grouped" — the block as it is built; "ungrouped" — one engine call (and one zeroing launch) per module;
# "banded" — the route of N beyond the fused tile (gn_affinity_f32 + the ragged banded top-k), taken at a small N by
# answering the block's question about the graph's form for it
BLOCKS = ([(c["id"], p, 1, "fp32", "grouped") for c in C.BLOCK_CASES for p in ("f16x3", "bf16x6", "fp32")]
          + [("n7", "f16x3", 2, "fp32", "grouped"), ("n50", "f16x3", 1, "bf16", "grouped"),
             ("n17", "f16x3", 1, "fp32", "ungrouped"), ("n17", "f16x3", 1, "fp32", "banded")])


@pytest.mark.parametrize("case_id,mode,nmp,dtype,form", BLOCKS,
                         ids=[f"{c}-{p}-nmp{n}-{d}-{f}" for c, p, n, d, f in BLOCKS])
def test_block_on_a_ragged_batch(case_id, mode, nmp, dtype, form, monkeypatch):
    from groupnet_amd import MS_HGNN_batch as M, multiscale, ops
    case, bf16 = C.BY_ID[case_id], dtype == "bf16"
    B, N, scales, counts = case["B"], case["N"], case["scales"], case["counts"]
    h, U, sp, shs, per_scene = C.block_oracle(case_id, nmp, bf16)
    blk = C.cpu_block(case, nmp)[0].to(dev()).eval()
    blk.grouped = form != "ungrouped"
    zeroings, real_zero = [], ops.zero_padding
    monkeypatch.setattr(ops, "zero_padding", lambda *a, **k: zeroings.append(1) or real_zero(*a, **k))
    if form == "banded":
        monkeypatch.setattr(ops, "graph_form", lambda *a, **k: "banded")
    x = C.with_garbage(case, h).to(dev())
    x = x.bfloat16() if bf16 else x
    nd = [[u.to(dev()) for u in us] for us in U]
    res, orig = {}, M.run_message_passing

    def spy(*a, **k):
        r = orig(*a, **k)
        res.setdefault("all", []).extend(r)
        return r
    monkeypatch.setattr(multiscale, "run_message_passing", spy)
    with precision(mode), torch.no_grad():
        out, new_H = blk(x, noise_u=nd, n_agents=counts)
        assert len(res["all"]) == 1 + len(scales)
        assert len(zeroings) == (1 if blk.grouped else 1 + len(scales))        # one launch per engine call
        facs = [r[1].float().cpu() for r in res["all"]]
        same = blk(x, noise_u=nd, n_agents=[N] * B)
        full = blk(x, noise_u=nd)
    assert torch.equal(same[0], full[0]) and torch.equal(same[1], full[1])
    assert out.dtype == x.dtype and torch.equal(out[..., :64], x)             # f copied through, padding included
    out, bad = out.float().cpu(), []
    assert bool(torch.isfinite(out).all())
    assert torch.equal(new_H.float().cpu(), torch.cat([C.padded_incidence(case, h, s) for s in scales], dim=1))
    n_mod = 1 + len(scales)
    feat_err, fac_err, scale = [0.0] * n_mod, [0.0] * n_mod, [0.0] * n_mod
    for b, n in enumerate(counts):
        feats, rfacs, _ = per_scene[b]
        if out[b, n:, 64:].any():
            bad.append(f"scene {b}: padded node rows are not zero")
        for i in range(n_mod):
            got = out[b, :n, 64 * (1 + i):64 * (2 + i)]
            feat_err[i] = max(feat_err[i], maxerr(got, feats[i]))
            scale[i] = max(scale[i], float(feats[i].abs().max()))
            f = facs[i][b]
            rows = C.pair_index(N, n) if i == 0 else torch.arange(rfacs[i].shape[0])
            pad = torch.ones(f.shape[0], dtype=torch.bool)
            pad[rows] = False
            fac_err[i] = max(fac_err[i], maxerr(f[rows], rfacs[i]))
            if f[pad].any():
                bad.append(f"scene {b} module {i}: padded factors are not zero")
    print(f"\n{case_id} {mode} nmp={nmp} {dtype} {form}: features {['%.1e' % e for e in feat_err]} of {['%.2f' % s for s in scale]}, "
          f"factors {['%.1e' % e for e in fac_err]}")
    for i in range(n_mod):
        tol_feat, tol_fac = (TOL_ORACLE * scale[i], TOL_ORACLE) if bf16 else (C.TOL, C.TOL)
        if feat_err[i] > tol_feat:
            bad.append(f"module {i}: features {feat_err[i]:.3e} > {tol_feat:.3e}")
        if fac_err[i] > tol_fac:
            bad.append(f"module {i}: factors {fac_err[i]:.3e} > {tol_fac:.3e}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("K", [1, 9, 15])
def test_modules_with_an_odd_number_of_edge_types_on_bf16_storage(K):
    """bf16 factor rows of an odd number of types are 2 K bytes, not a multiple of 4: the zeroing launch writes them as
    2-byte words.  The pairwise module, a top-k module and a scale-N module of K types on case n17, each against the
    per-scene oracle at the twins' gate."""
    from edge_type_cases import hyper_module, pair_module
    from launch_forms import state64
    case = C.BY_ID["n17"]
    B, N, counts = case["B"], case["N"], case["counts"]
    h, _ = C.inputs(case, bf16=True)
    x = C.with_garbage(case, h).to(dev()).bfloat16()
    corr = C.garbage_corr(case, C.padded_corr(case, h)).to(dev())
    gen = torch.Generator().manual_seed(K)
    bad = []
    for mod, s in ((pair_module(K, K), None), (hyper_module(K, 5, K + 1), 5), (hyper_module(K, N, K + 2), N)):
        st = state64({k: v.detach().clone() for k, v in mod.state_dict().items()})
        E = N * N if s is None else C.n_edges(N, s)
        U = torch.rand(B, E, K, generator=gen)
        mod = mod.to(dev()).eval()
        with torch.no_grad():
            if s is None:
                nf, fac = mod(x, noise_u=U.to(dev()), n_agents=counts)
            else:
                nf, fac, H = mod(x, corr, noise_u=U.to(dev()), n_agents=counts)
                assert H.dtype == torch.bfloat16 and torch.equal(H.float().cpu(), C.padded_incidence(case, h, s))
        assert fac.dtype == torch.bfloat16 and fac.shape == (B, E, K)
        nf, fac = nf.float().cpu(), fac.float().cpu()
        feat_err = fac_err = scale = 0.0
        for b, n in enumerate(counts):
            hb = h[b:b + 1, :n].double()
            u = [t.double() for t in C.scene_noise([U], b, N, n, s is None)]
            with torch.no_grad():
                if s is None:
                    rf, rfac = O.ms_hgnn_pairwise_forward(st, hb, u, 1, decomposed=True)
                    rows = C.pair_index(N, n)
                else:
                    Hb = C.scene_incidence(C.scene_corr(h, b, n), s, N)
                    rf, rfac = O._message_passing(st, hb, Hb.double(), u, 1, True, None)
                    rows = torch.arange(rfac.shape[1])
            pad = torch.ones(E, dtype=torch.bool)
            pad[rows] = False
            feat_err, scale = max(feat_err, maxerr(nf[b, :n], rf[0])), max(scale, float(rf.abs().max()))
            fac_err = max(fac_err, maxerr(fac[b, rows], rfac[0]))
            if nf[b, n:].any() or fac[b, pad].any():
                bad.append(f"scale {s} scene {b}: padded positions are not zero")
        print(f"\nK={K} scale {s}: features {feat_err:.1e} of {scale:.2f}, factors {fac_err:.1e}")
        if feat_err > TOL_ORACLE * scale or fac_err > TOL_ORACLE:
            bad.append(f"scale {s}: features {feat_err:.3e} (max|ref| {scale:.3e}), factors {fac_err:.3e}")
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------------------------
def test_golden_scenes_in_a_padding_reproduce_the_reference():
    """Five scenes of the reference's own N = 11 golden in an N = 13 padding, n_agents = 11: the modules reproduce the
    stored outputs on the valid block."""
    import groupnet_amd as G
    c = load_case("syn_n11_b37")
    B, n, N = 5, 11, 13
    gen = torch.Generator().manual_seed(13)
    h = torch.randn(B, N, 64, generator=gen) * 100.0
    h[:, :n] = torch.from_numpy(c["h"][:B])
    corr = torch.randn(B, N, N, generator=gen) * 100.0
    corr[:, :n, :n] = torch.from_numpy(c["corr"][:B])
    idx = C.pair_index(N, n)
    kw = dict(h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=1)
    pair = G.MS_HGNN_oridinary(embedding_dim=16, **kw)
    pair.load_state_dict(load_state("pairwise"), strict=True)
    pair = pair.to(dev()).eval()
    counts = [n] * B
    hd, cd = h.to(dev()), corr.to(dev())
    with torch.no_grad():
        U = torch.rand(B, N * N, 6, generator=gen)
        U[:, idx] = torch.from_numpy(c["pair_U0"][:B])
        nf, fac = pair(hd, noise_u=U.to(dev()), n_agents=counts)
        assert maxerr(nf[:, :n], torch.from_numpy(c["pair_node_feat"][:B])) <= C.TOL
        assert maxerr(fac[:, idx], torch.from_numpy(c["pair_factors"][:B])) <= C.TOL
        assert not nf[:, n:].any()
        pad = torch.ones(N * N, dtype=torch.bool)
        pad[idx] = False
        assert not fac[:, pad].any()
        for s in c["scales"].tolist():
            scale = N if s == n else s                  # the stored all-agents scale is the padded module's scale N
            hyper = G.MS_HGNN_hyper(embedding_dim=64, scale=scale, **kw)
            hyper.load_state_dict(load_state("hyper"), strict=True)
            hyper = hyper.to(dev()).eval()
            E = 1 if s == n else n
            U = torch.rand(B, 1 if s == n else N, 10, generator=gen)
            U[:, :E] = torch.from_numpy(c[f"hyper{s}_U0"][:B])
            nf, fac, H = hyper(hd, cd, noise_u=U.to(dev()), n_agents=counts)
            assert H.shape == (B, 1 if s == n else N, N)
            assert torch.equal(H[:, :E, :n].cpu(), torch.from_numpy(c[f"hyper{s}_H"][:B])), s
            assert not H[:, E:].any() and not H[:, :, n:].any()
            assert maxerr(nf[:, :n], torch.from_numpy(c[f"hyper{s}_node_feat"][:B])) <= C.TOL, s
            assert maxerr(fac[:, :E], torch.from_numpy(c[f"hyper{s}_factor"][:B])) <= C.TOL, s
            assert not nf[:, n:].any() and not fac[:, E:].any()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(monkeypatch):
    import groupnet_amd as G
    from groupnet_amd import ops
    case = C.BY_ID["n7"]
    B, N, counts = case["B"], case["N"], case["counts"]
    blk = C.cpu_block(case)[0].to(dev())
    h, U = C.inputs(case)
    x = h.to(dev())
    corr = torch.zeros(B, N, N, device=dev())
    pair, hyper = blk.interaction, blk.interaction_hyper[0]
    with torch.no_grad():                   # weight images are packed once, outside the count
        blk.eval()(x, n_agents=counts)
    torch.cuda.synchronize()
    launches = []
    real, upload = ops.stream_handle, ops.AgentCounts.dev
    monkeypatch.setattr(ops, "stream_handle", lambda: launches.append(1) or real())
    # ... and the counts go to the device with the first launch: a refused call has copied nothing either
    monkeypatch.setattr(ops.AgentCounts, "dev", property(lambda self: launches.append("upload") or upload.fget(self)))
    blk.train()
    for call in (lambda: blk(x, n_agents=counts), lambda: pair(x, n_agents=counts),
                 lambda: hyper(x, corr, n_agents=counts)):
        with pytest.raises(NotImplementedError):         # autograd is recording: training is not built
            call()
    blk.eval()
    with torch.no_grad():
        with pytest.raises(ValueError):
            hyper(x, corr, H=torch.zeros(B, N, N, device=dev()), n_agents=counts)
        with pytest.raises(ValueError):
            hyper(x, corr, masks=ops.IncidenceMasks(torch.zeros(B, N, dtype=torch.int64, device=dev()),
                                                    torch.zeros(B, N, dtype=torch.int64, device=dev())), n_agents=counts)
        with pytest.raises(ValueError):
            blk(x, n_agents=torch.tensor(counts, device=dev()))              # a device tensor would have to be read back
        for bad in ([0] + counts[1:], counts[:-1], [N + 1] + counts[1:]):
            with pytest.raises(ValueError):
                blk(x, n_agents=bad)
        hyper.listall = True
        try:
            with pytest.raises(NotImplementedError):
                hyper(x, corr, n_agents=counts)
            with pytest.raises(NotImplementedError):
                blk(x, n_agents=counts)
        finally:
            hyper.listall = False
        big = G.MS_HGNN_hyper(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=1,
                              scale=N + 1).to(dev()).eval()
        with pytest.raises(RuntimeError):
            big(x, corr, n_agents=counts)
        with pytest.raises(ValueError):
            ops.affinity_topk(x, [2], want_masks=True, n_agents=counts)
    assert not launches
