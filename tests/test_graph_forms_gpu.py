"""The stage that builds the graph — cosine affinity, then the top-k incidence — on the GPU at the edges of its three
forms (tail of the node stage | stand-alone fused launch | banded pair; tests/launch_forms.py `graph_forms`), on ragged
bands and in every regime of the stand-alone top-k launcher's band size.  tests/test_graph_forms_cpu.py states what each
case reaches.  Needs an MI355X: `pytest -m gpu`.

Where a test calls a C entry point directly, the outputs are pre-filled with NaN and allocated one scene longer than B:
an element the kernel did not write shows, and so does a write past the last scene (the guard scene must still be all
NaN afterwards)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from incidence_mask_cases import np_masks, random_incidence
from launch_forms import (AFFINITY_CASES, AFFINITY_D_CASES, FUSED_CASES, SCATTER_GPU_CASES, TOPK_CASES, _spread,
                          assert_scatter_plan, graph_forms, scatter_case_groups, scatter_forms, topk_bands)
from oracle import ms_hgnn_oracle as O
from oracle import past_encoder_oracle as PO
from test_parity_gpu import TOL, TOL_CORR, maxerr

pytestmark = pytest.mark.gpu

NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def corr64(f):
    """float64 normalize(f) @ normalize(f)^T of the (fp32 / bf16) features as stored."""
    q = F.normalize(f.detach().cpu().double(), p=2, dim=2)
    return q @ q.transpose(1, 2)


def dot_bound(D):
    """A-priori bound of a length-D fp32 dot product of two unit vectors against exact arithmetic: D products and D - 1
    sums, each rounded once, plus the roundings of a normalisation (square, sum, root, divide) — (D + 8) 2^-24 — twice,
    for the two normalised operands."""
    return 2 * (D + 8) * 2.0 ** -24


def features(B, N, D, seed):
    """Random features; scene 0 holds an all-zero row (3) and a duplicate of row 1 in the LAST row (the ragged band)."""
    g = torch.Generator().manual_seed(seed)
    f = torch.randn(B, N, D, generator=g)
    f[0, 3] = 0
    f[0, N - 1] = f[0, 1]
    return f


# ---- a / b: gn_affinity_f32 alone ------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D", AFFINITY_CASES + AFFINITY_D_CASES, ids=lambda v: str(v))
def test_affinity_entry_on_ragged_bands_and_form_edges(B, N, D):
    """gn_affinity_f32 against float64 at: banded shapes whose last band has 1 / 8 rows and whose last panel has 49 / 1 / 8
    columns, the exact N = 256, the largest fused tile (N = 112), N = 41; D = 4, 36, 128 at N = 11 and D = 128 on both
    sides of its switch (99 | 100).  Bar: TOL_CORR at D = 64, the a-priori `dot_bound(D)` elsewhere (measured on MI355X:
    D = 4 1.2e-7, D = 36 1.8e-7, D = 128 4.8e-7 fused and 5.4e-7 banded; D = 64 3.6e-7 .. 4.8e-7).  corr is bitwise symmetric in both
    forms; a zero feature row gives an exactly zero row and column; a duplicated feature row a bitwise equal row."""
    from groupnet_amd._lib import load, stream_handle
    form = graph_forms(B, N, D)
    f = features(B, N, D, 1000 * D + N).to(dev())
    corr = torch.full((B + 1, N, N), NAN, device=dev())
    with torch.cuda.device(dev()):
        rc = load().gn_affinity_f32(f.data_ptr(), corr.data_ptr(), B, N, D, stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    c = corr.cpu()
    assert bool(torch.isnan(c[B]).all()), "a write past the last scene"
    assert not bool(torch.isnan(c[:B]).any()), "an element of corr was not written"
    c = c[:B]
    err = float((c.double() - corr64(f)).abs().max())
    bar = TOL_CORR if D == 64 else dot_bound(D)
    print(f"\naffinity B={B} N={N} D={D}: form {'banded' if form['form'] == 'banded' else 'fused'}, grid {form['aff_grid']}, "
          f"last band/panel {form['aff_last']}, max |corr - float64| = {err:.2e} (bar {bar:.2e})")
    assert err <= bar
    assert torch.equal(c, c.transpose(1, 2).contiguous())
    assert bool((c[0, 3] == 0).all()) and bool((c[0, :, 3] == 0).all())
    assert torch.equal(c[0, N - 1], c[0, 1]) and torch.equal(c[0, :, N - 1], c[0, :, 1])


# ---- c: gn_topk_incidence_f32 alone ----------------------------------------------------------------------------------
def _planted(corr):
    """In the first and the last scene: row 0 holds -0.0 beside +0.0, a NaN, +inf and -inf; row 1 a second NaN."""
    for b in (0, corr.shape[0] - 1):
        corr[b, 0, :5] = torch.tensor([-0.0, 0.0, NAN, float("inf"), float("-inf")], device=corr.device)
        corr[b, 1, 1] = NAN
    return corr


@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("B,N", TOPK_CASES, ids=lambda v: str(v))
def test_topk_entry_in_every_band_regime(B, N, kind):
    """gn_topk_incidence_f32 with eight scales in one call at the (RB, remainder) regimes of its launcher — one band of
    all N rows, the LDS cap with a short last band, a halved band with a remainder, RB < 8, RB = 8 with a last band of one
    row — on random normal affinities and on small integers with heavy ties, a NaN, +-inf and -0.0 beside +0.0.  Exact
    against the plain-C arg-max oracle and against the ranked rule (B >= 300: on 16 scenes, first and last included; every
    scene: fully written, k members per row)."""
    from groupnet_amd._lib import load, stream_handle
    from test_oracle_golden import _c_oracle, _c_topk
    RB, bands, rem = topk_bands(B, N)
    scales = [0, 1, 2, 5, N // 2, N - 2, N - 1, N]
    g = torch.Generator(device=dev()).manual_seed(31 * N + B)
    if kind == "normal":
        corr = torch.randn(B, N, N, device=dev(), generator=g)
    else:
        corr = _planted(torch.randint(0, 3, (B, N, N), device=dev(), generator=g).float())
    Hs = [torch.full((B + 1, 1 if s == N else N, N), NAN, device=dev()) for s in scales]
    Hl = (ctypes.c_void_p * 8)(*[h.data_ptr() for h in Hs])
    kl = (ctypes.c_int * 8)(*scales)
    with torch.cuda.device(dev()):
        rc = load().gn_topk_incidence_f32(corr.data_ptr(), Hl, kl, 8, B, N, stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    print(f"\ntop-k B={B} N={N} ({kind}): RB {RB}, {bands} bands, remainder {rem}")
    for s, H in zip(scales, Hs):
        assert bool(torch.isnan(H[B]).all()), ("a write past the last scene", s)
        assert not bool(torch.isnan(H[:B]).any()), ("an element of H was not written", s)
        assert bool((H[:B].sum(-1) == (N if s == N else max(s, 1))).all()), s
    pick = torch.tensor(_spread(range(B), 16) if B >= 300 else list(range(B)))
    assert pick[0] == 0 and pick[-1] == B - 1
    sub = corr[pick.to(dev())].cpu()
    lib = _c_oracle()
    for s, H in zip(scales, Hs):
        got = H[pick.to(dev())].cpu()
        rc, want = _c_topk(lib, sub.numpy(), s)
        assert rc == 0 and np.array_equal(got.numpy(), want), (B, N, s)
        assert torch.equal(got, O.topk_incidence_ranked(sub, s)), (B, N, s)


# ---- d: the fused launch through ops.affinity_topk -------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("B,N", FUSED_CASES, ids=lambda v: str(v))
def test_fused_launch_at_its_edges(B, N, dtype):
    """ops.affinity_topk at N = 40 | 41 (the tail's limit) and at N = 112 (the largest tile the launch can get), fp32 and
    bf16 storage.  With corr: every H is the ranked rule applied to the corr the same launch wrote, corr meets TOL_CORR
    against float64.  Without (production): the same H bit for bit, f into a column slice of a wider tensor, cat(H_s).
    Scene 0 random, scene 1 with rows 5 and N - 1 duplicates of row 2 (the lower index wins the tie), scene 2 with a NaN row
    and an all-zero row."""
    from groupnet_amd import ops
    g = torch.Generator().manual_seed(7 * N)
    f = torch.randn(B, N, 64, generator=g)
    f[1, 5] = f[1, 2]
    f[1, N - 1] = f[1, 2]
    f[2, 4] = NAN
    f[2, 7] = 0
    f = f.to(dtype).to(dev())
    scales = [1, 2, 5, N - 1, N]
    corr, Hs, _ = ops.affinity_topk(f, scales)
    c = corr.cpu()
    for s, H in zip(scales, Hs):
        assert torch.equal(H.cpu(), O.topk_incidence_ranked(c, s)), (N, s)
    ref = corr64(f.float())
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(c), nan) and bool(nan[2, 4].all()) and int(nan.sum()) == 2 * N - 1
    err = float((c.double() - ref)[~nan].abs().max())
    print(f"\nfused N={N} {dtype}: tile {graph_forms(B, N)['tile']} B, max |corr - float64| = {err:.2e}")
    assert err <= TOL_CORR
    assert bool((c[2, 7][~nan[2, 7]] == 0).all())
    for r in (2, 5, N - 1):      # the three copies tie exactly in every row; the top-1 of a copy's own row is the first copy
        assert torch.equal(c[1, :, r], c[1, :, 2])
        assert Hs[0][1, r].nonzero().flatten().tolist() == [2]
    # production form
    wide = torch.full((B, N, 192), NAN, dtype=dtype, device=dev())
    corr2, Hs2, H_cat = ops.affinity_topk(f, scales, want_corr=False, f_out=wide[..., 64:128], want_H_cat=True)
    assert corr2 is None
    for a, b in zip(Hs, Hs2):
        assert torch.equal(a, b)
    assert H_cat.dtype == dtype and torch.equal(H_cat, torch.cat(Hs, dim=1).to(dtype))
    assert torch.equal(_bits(wide[..., 64:128]), _bits(f))
    assert bool(torch.isnan(wide[..., :64]).all()) and bool(torch.isnan(wide[..., 128:]).all())


def _embed_excess(f, x, M, c):
    """max |f - float64 (M x + c)| / ((x_dim + 1) 2^-24 S), S = |c| + |M| |x| element-wise: at most 1 for a chain of x_dim
    fused multiply-adds onto c (one rounding each, on partial sums bounded by S; the + 1 covers the second-order terms)."""
    x, M, c = x.cpu().double(), M.cpu().double(), c.cpu().double()
    want = x @ M.t() + c[None]
    S = x.abs() @ M.abs().t() + c.abs()[None]
    return float(((f.cpu().double() - want).abs() / ((x.shape[-1] + 1) * 2.0 ** -24 * S)).max())


def test_fused_launch_embedding_form_with_masks_at_an_odd_raw_width():
    """embed = (x_raw, M, c) with x_dim = 5 at N = 17 and masks: N x_dim = 85 raw floats sit in front of the mask words,
    the one layout in which the words need the `nx & 1` pad to stay 8-byte aligned.  f against float64 M x + c: the kernel
    adds x_dim fused multiply-adds to c, hence the element-wise bound of `_embed_excess`.  H is the ranked rule on the
    launch's own corr; the words are the bit-mask form of that H."""
    from groupnet_amd import ops
    B, N, xd = 3, 17, 5
    g = torch.Generator().manual_seed(17)
    x, M, c = torch.randn(B, N, xd, generator=g) * 3, torch.randn(64, xd, generator=g), torch.randn(N, 64, generator=g)
    scales = [1, 2, 5, N - 1, N]
    corr, Hs, H_cat, f, masks = ops.affinity_topk(None, scales, embed=(x.to(dev()), M.to(dev()), c.to(dev())),
                                                  want_masks=True)
    assert H_cat is None and len(masks) == len(scales)
    excess = _embed_excess(f, x, M, c)
    print(f"\nembedding form: max |f - float64| / bound = {excess:.2f}")
    assert excess <= 1.0
    assert maxerr(corr, corr64(f)) <= TOL_CORR
    for s, H, m in zip(scales, Hs, masks):
        assert torch.equal(H.cpu(), O.topk_incidence_ranked(corr.cpu(), s)), s
        row, col = np_masks(H.cpu().numpy())
        assert np.array_equal(m.row.cpu().numpy(), row) and np.array_equal(m.col.cpu().numpy(), col), s


# ---- e: the switch points through the engine -------------------------------------------------------------------------
def _gaps(corr, scales):
    """Smallest gap between the k-th and the (k+1)-th affinity of a row, over every row and every scale k < N."""
    N = corr.shape[-1]
    srt = torch.sort(corr, dim=-1, descending=True).values
    return min(float((srt[..., s - 1] - srt[..., s]).min()) for s in scales if s < N)


@pytest.mark.parametrize("N", [112, 113])
def test_multiscale_block_on_both_sides_of_the_banded_switch(N):
    """MultiScaleHGNN([2, 8, N]) at B = 1, N = 112 (the largest fused tile) and N = 113 (the banded pair: 8 affinity bands
    with a last band of one row, top-k RB = 8 with a last band of one row) against the oracle: the incidence equal on
    every row — the seed leaves more than 1e-6 between the k-th and (k+1)-th affinity of every row, asserted — and the
    features within TOL."""
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(8)
    scales = [2, 8, N]
    blk = MultiScaleHGNN(scales)
    sp = {k: v.detach().clone() for k, v in blk.interaction.state_dict().items()}
    shs = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in blk.interaction_hyper]
    blk.to(dev()).eval()
    B = 1
    assert graph_forms(B, N)["form"] == ("fused" if N == 112 else "banded")
    h = torch.randn(B, N, 64)
    corr = O.affinity(h)
    assert _gaps(corr, scales) > 1e-6
    noise = [[torch.rand(s)] for s in blk.noise_shapes(B, N)]
    with torch.no_grad():
        out, H = blk(h.to(dev()), noise_u=[[u.to(dev()) for u in n] for n in noise])
        ref_pair, _ = O.ms_hgnn_pairwise_forward_chunked(sp, h, noise[0], slab=4096)
        refs, Hr = [], []
        for st, s, U in zip(shs, scales, noise[1:]):
            nf, _, Hs = O.ms_hgnn_hyper_forward(st, h, corr, s, U, decomposed=True)
            refs.append(nf)
            Hr.append(Hs)
    assert out.shape == (B, N, 64 * 5) and torch.equal(out[..., :64].cpu(), h)
    assert torch.equal(H.cpu(), torch.cat(Hr, dim=1))
    errs = [maxerr(out[..., 64:128], ref_pair)] + [maxerr(out[..., 64 * (2 + i):64 * (3 + i)], r) for i, r in enumerate(refs)]
    print(f"\nblock N={N}: pairwise / hyper errors {['%.1e' % e for e in errs]}")
    assert max(errs) <= TOL


def test_multiscale_block_banded_route_in_bf16():
    """The block at N = 113 on bf16 storage (the banded pair runs on the up-cast features): new_H has the input's dtype
    and is the fp32 run's on f.float(); out[..., :64] is f."""
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(8)
    N, scales = 113, [2, 8, 113]
    blk = MultiScaleHGNN(scales).to(dev()).eval()
    f = torch.randn(2, N, 64, device=dev()).to(torch.bfloat16)
    noise = [[torch.rand(s, device=dev())] for s in blk.noise_shapes(2, N)]
    with torch.no_grad():
        out, H = blk(f, noise_u=noise)
        _, H32 = blk(f.float(), noise_u=noise)
    assert out.dtype == H.dtype == torch.bfloat16 and H32.dtype == torch.float32
    assert torch.equal(H.float(), H32) and torch.equal(out[..., :64], f)
    assert bool(torch.isfinite(out.float()).all())


def test_deferred_embedding_job_counts_its_raw_inputs():
    """AffinityTail(None, [2], embed=...) with 20 raw inputs per agent: the node stage takes it at N = 37 and not at N = 38
    (`fits_tail`), where `node_stage_grouped(..., affinity=job)` issues the stand-alone launch — and H is right either
    way."""
    import groupnet_amd as G
    from groupnet_amd import ops
    torch.manual_seed(3)
    hyper = G.MS_HGNN_hyper(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=1,
                            scale=2).to(dev()).eval()
    pk = hyper._packed_n2e(0)
    alone = []
    orig = ops.AffinityTail.launch

    def counting(self):
        alone.append(self.f.shape[1])
        return orig(self)
    ops.AffinityTail.launch = counting
    try:
        for N, rides in ((37, True), (38, False)):
            B, xd = 3, 20
            x, M, c = (torch.randn(B, N, xd, device=dev()), torch.randn(64, xd, device=dev()),
                       torch.randn(N, 64, device=dev()))
            job = ops.AffinityTail(None, [2], want_corr=True, embed=(x, M, c))
            assert job.fits_tail() is rides
            ops.node_stage_grouped([(torch.randn(B, N, 64, device=dev()), pk)], affinity=job)
            assert job.done and (N in alone) is (not rides)
            assert _embed_excess(job.f, x, M, c) <= 1.0
            assert maxerr(job.corr, corr64(job.f)) <= TOL_CORR
            assert torch.equal(job.Hs[0].cpu(), O.topk_incidence_ranked(job.corr.cpu(), 2))
    finally:
        ops.AffinityTail.launch = orig


@pytest.mark.parametrize("N,seed", [(107, 20), (108, 8)])
def test_past_encoder_eval_on_both_sides_of_the_fused_tile(N, seed):
    """PastEncoder (scales [5, 11], past_length 5: 20 raw inputs per agent) in eval mode at N = 107, the last scene tile
    the fused launch takes, and N = 108, which it serves from the HIP GEMM embedding and the banded pair, against the
    encoder oracle with the same seeded host noise: incidence equal on every row (gaps above 1e-6, asserted), features
    within the encoder tests' bar."""
    from test_past_encoder import _inputs, close_to, make
    scales = [5, 11]
    enc = make(scales, seed=seed)
    assert enc.fused_front_end_fits(N, 5) is (N == 107)
    sd = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    enc.to(dev())
    B = 1
    x = _inputs(B, N, 5, torch.Generator().manual_seed(seed))
    _, corr = PO.embed_and_affinity(sd, x, B, N)
    assert _gaps(corr, scales) > 1e-6
    torch.manual_seed(77)
    want, Hs = PO.encode(sd, x, B, N, scales)
    torch.manual_seed(77)
    with torch.no_grad():
        out, new_H = enc(x.to(dev()), B, N)
    assert out.shape == want.shape
    close_to(out, want, f"PastEncoder N={N} vs oracle")
    assert torch.equal(new_H.cpu(), torch.cat(Hs, dim=1))


# ---- the scatter, once per planned form -----------------------------------------------------------------------------
def scatter_case_inputs(B, N, spec, dtype, seed=0):
    """Per group of a SCATTER_GPU_CASES case, on the GPU: {"feat" (as the launch reads it, storage type `dtype`), "ori",
    "H" (dense (B,E,N) fp32 or None), "col" (column words or None), "E", "sym", and for the reference "Hd" (the dense
    incidence, (E,N) shared by all scenes for the pairwise graph) and "fd" (the features `Hd` multiplies)}.
    Pairwise groups: ordered features (B, N*N, 64) against the oracle's `pairwise_incidence`; the unordered-pair features
    are formed from them exactly as test_symmetric_pairwise_stages_equal_ordered_ones does — diagonal doubled,
    off-diagonal summed.  bf16 storage: the ordered features are multiples of 1/8 within +-4, so that sum is exact in bf16
    and the launch reads the very numbers the reference sums."""
    g = torch.Generator(device=dev()).manual_seed(1000 * N + B + seed)
    rnd = lambda *shape: torch.randn(*shape, generator=g, device=dev())
    store = lambda t: t.to(dtype).contiguous()
    out = []
    for i, c in enumerate(spec):
        ori = store(rnd(B, N, 64))
        if c in "so":
            fd = rnd(B, N * N, 64)
            if dtype == torch.bfloat16:
                fd = (fd * 8).round().clamp(-32, 32) / 8
            Hd = O.pairwise_incidence(N, 1, torch.float64)[0].to(dev())
            feat = fd
            if c == "s":
                pr = [(a, b) for a in range(N) for b in range(a, N)]
                ij = torch.tensor([a * N + b for a, b in pr], device=dev())
                ji = torch.tensor([b * N + a for a, b in pr], device=dev())
                diag = torch.tensor([a == b for a, b in pr], device=dev())
                feat = torch.where(diag[None, :, None], 2 * fd[:, ij], fd[:, ij] + fd[:, ji])
            feat = store(feat)
            out.append(dict(feat=feat, ori=ori, H=None, col=None, E=feat.shape[1], sym=c == "s", Hd=Hd, fd=store(fd)))
        else:
            H = random_incidence(B, N, N, seed=17 * i + N + B)
            col = torch.from_numpy(np_masks(H.numpy())[1]).to(dev()) if c == "m" else None
            feat = store(rnd(B, N, 64))
            H = H.to(dev())
            out.append(dict(feat=feat, ori=ori, H=None if c == "m" else H, col=col, E=N, sym=False, Hd=H.double(), fd=feat))
    return out


def scatter_reference(grp, N, dtype, chunk=32):
    """float64 cat(H^T feat, ori) / N of one group and the a-priori bar per element.  fp32: the kernel rounds once per
    term it adds into a node (E_n terms: the non-zero entries of the node's column of H) and once for the division, the
    pair features once more where they were summed from the ordered ones: (E_n + 4) 2^-24 sum|H feat| / N covers them (the
    ori half: one division, 4 2^-24 |ori| / N).  bf16 storage: fp32 accumulation of the stored values, then the output
    rounding, 2^-8 |ref|."""
    Hd, B = grp["Hd"], grp["ori"].shape[0]
    refs, bars = [], []
    for b0 in range(0, B, chunk):
        sl = slice(b0, min(B, b0 + chunk))
        Ht = (Hd if Hd.dim() == 2 else Hd[sl]).transpose(-1, -2)            # (N, E) or (b, N, E)
        f, o = grp["fd"][sl].double(), grp["ori"][sl].double()
        terms = (Ht != 0).sum(-1, keepdim=True).double()                     # E_n
        terms = terms.expand(f.shape[0], N, 1) if terms.dim() == 2 else terms
        refs.append(torch.cat([Ht @ f, o], dim=-1) / N)
        bars.append(torch.cat([(terms + 4) * (Ht.abs() @ f.abs()), 4 * o.abs()], dim=-1) / N * 2.0 ** -24)
    ref, bar = torch.cat(refs), torch.cat(bars)
    return ref, bar + (2.0 ** -8 * ref.abs() if dtype == torch.bfloat16 else 0)


def scatter_descriptors(grps, outs):
    from groupnet_amd import _lib as L
    return (L.ScatterGroup * len(grps))(*[
        L.ScatterGroup(feat=g["feat"].data_ptr(), H=L.addr(g["H"]), ori=g["ori"].data_ptr(), out=o.data_ptr(), E=g["E"],
                       sym=int(g["sym"]), colmask=L.addr(g["col"])) for g, o in zip(grps, outs)])


SCATTER_IDS = [f"B{B}-N{N}-{spec[0]}x{len(spec)}-{dt}" for B, N, spec, dts, _ in SCATTER_GPU_CASES for dt in dts]


@pytest.mark.parametrize("B,N,spec,dt,form", [(B, N, spec, dt, form) for B, N, spec, dts, form in SCATTER_GPU_CASES for dt in dts],
                         ids=SCATTER_IDS)
def test_scatter_entry_in_every_planned_form(B, N, spec, dt, form, monkeypatch):
    """gn_agg_scatter_* once per form its plan can take — the pairs kernel at both ends of its N range, the direct kernel in
    its three modes (unordered pairs below B = 256 and beyond N = 64, ordered pairs, a hyper group beyond the staged
    tile), the staged kernel with 1, 2 and 16 scenes per workgroup (the last workgroup holding ONE scene) and the mask
    kernel likewise — against float64 cat(H^T feat, ori) / N with the dense H, at the a-priori bar of `scatter_reference`.
    The plan's form is asserted first.  Outputs are pre-filled with NaN and one scene longer than B."""
    from groupnet_amd import _lib as L
    monkeypatch.delenv("GN_SCATTER_PAIRS", raising=False)
    lib = L.load()
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    sfx = "bf16" if dt == "bf16" else "f32"
    grps = scatter_case_inputs(B, N, spec, dtype)
    outs = [torch.full((B + 1, N, 128), NAN, dtype=dtype, device=dev()) for _ in grps]
    arr = scatter_descriptors(grps, outs)
    plan = L.LaunchPlan()
    assert getattr(lib, f"gn_agg_scatter_plan_{sfx}")(arr, len(grps), B, N, float(N), ctypes.byref(plan)) == 0
    sf = scatter_forms(B, N, scatter_case_groups(N, spec))
    assert_scatter_plan(sf, plan, (B, N, spec, dt))
    kernel, G = form
    if G:
        assert (lib.gn_kernel_name(plan.kernel).decode(), plan.G) == (kernel, G) and (G == 1 or B % G == 1)
    else:
        assert plan.kernel == 0 and lib.gn_kernel_name(plan.pre_kernel[0]).decode() == kernel
    with torch.cuda.device(dev()):
        rc = getattr(lib, f"gn_agg_scatter_{sfx}")(arr, len(grps), B, N, float(N), L.stream_handle())
    torch.cuda.synchronize()
    assert rc == 0
    worst = 0.0
    for i, (grp, out) in enumerate(zip(grps, outs)):
        assert bool(torch.isnan(out[B]).all()), f"group {i}: a write past the last scene"
        got = out[:B].double()
        assert not bool(torch.isnan(got).any()), f"group {i}: an element was not written"
        ref, bar = scatter_reference(grp, N, dtype)
        excess = ((got - ref).abs() - bar).max().item()
        worst = max(worst, ((got - ref).abs() / bar.clamp_min(1e-300)).max().item())
        assert excess <= 0, f"group {i}: |got - ref| exceeds the bar by {excess:.3e}"
    print(f"\nscatter B={B} N={N} {spec[0]}x{len(spec)} {dt}: {kernel} G={G}, worst |err| / bar = {worst:.3f}")

