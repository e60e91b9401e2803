"""The bit-mask form of a hyperedge incidence (ABI 37) on the GPU, four groups:

  * the builder (gn_incidence_masks_f32) against the numpy statement of the masks (tests/incidence_mask_cases.py);
  * the masks the fused affinity + top-k launch emits against the builder applied to the H of the same launch;
  * the mask form of the stand-alone gather and scatter against the dense form, `torch.equal`;
  * the engine with the switch on against the switch off: the block, a module alone, a graph replay, and which kernels ran.

N: 17 is the smallest N that reaches the stand-alone launches, 33 puts members above bit 31, 64 uses bit 63, 50 is
BASELINE config 4.  Everything here is exact (bit patterns, `torch.equal`): there is no tolerance to derive."""
import ctypes

import numpy as np
import pytest
import torch

from incidence_mask_cases import np_masks, random_incidence

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def form():
    """Set the incidence form inside a test; the environment decides again afterwards."""
    from groupnet_amd import ops
    yield ops.set_incidence_form
    ops.set_incidence_form(None)


def _assert_masks(m, H, where):
    row, col = np_masks(H.cpu().numpy())
    assert np.array_equal(m.row.cpu().numpy(), row), f"{where}: rowmask"
    assert np.array_equal(m.col.cpu().numpy(), col), f"{where}: colmask"


# ---- builder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,E,N", [(3, 1, 1), (5, 17, 17), (4, 33, 33), (2, 64, 64), (2, 1, 64), (7, 50, 50)])
def test_builder_matches_numpy(B, E, N):
    from groupnet_amd import _lib, ops
    H = random_incidence(B, E, N, seed=B * 100 + N).to(dev())
    m = ops.incidence_masks(H)                        # reads the flag back: H is binary, no error
    assert m.row.dtype == m.col.dtype == torch.int64 and m.row.shape == (B, E) and m.col.shape == (B, N)
    _assert_masks(m, H, f"({B},{E},{N})")
    _assert_masks(ops.incidence_masks(H, assume_binary=True), H, "assume_binary")
    # the flag: written 0 for a binary H (whatever it held), 1 once one entry is a weight 2 — whose bit is set all the same
    flag = torch.full((1,), 7, dtype=torch.int32, device=dev())
    row, col = torch.empty_like(m.row), torch.empty_like(m.col)
    call = lambda h: _lib.load().gn_incidence_masks_f32(h.data_ptr(), B, E, N, row.data_ptr(), col.data_ptr(),
                                                         flag.data_ptr(), _lib.stream_handle())
    assert call(H) == 0 and int(flag.item()) == 0
    H2 = H.clone()
    H2[B - 1, E - 1, N // 2] = 2.0
    assert call(H2) == 0 and int(flag.item()) == 1
    _assert_masks(ops.IncidenceMasks(row, col), H2, "weight-2 entry")
    with pytest.raises(ValueError, match="0 and 1"):
        ops.incidence_masks(H2)
    _assert_masks(ops.incidence_masks(H2, assume_binary=True), H2, "weight-2 entry, unchecked")


# ---- fused emission -----------------------------------------------------------------------------------------------------
def _features(B, N, dtype, kind, seed):
    torch.manual_seed(seed)
    f = torch.randn(B, N, 64)
    if kind == "ties" and N >= 3:
        f[:, 1] = f[:, 0]                 # equal affinities in every row: the lower index wins
        f[:, N - 1] = f[:, 0]
    if kind == "nan" and N >= 2:
        f[0, N // 2, 5] = float("nan")    # a NaN row and column of corr: NaN ranks first
    return f.to(dev()).to(dtype)


# ties and NaN rows: one size inside a word and the full word
EMISSION_CASES = [(N, "random") for N in (2, 11, 17, 33, 50, 64)] + [(17, "ties"), (64, "ties"), (17, "nan"), (64, "nan")]


@pytest.mark.parametrize("N,kind", EMISSION_CASES, ids=[f"N{N}-{k}" for N, k in EMISSION_CASES])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_fused_emission_equals_the_builder(dtype, N, kind):
    from groupnet_amd import ops
    B = 3
    scales = sorted({1, 2, min(5, N), N - 1, N})
    f = _features(B, N, dtype, kind, seed=N)
    _, Hs0, Hcat0 = ops.affinity_topk(f, scales, want_corr=False, want_H_cat=True)
    _, Hs, Hcat, masks = ops.affinity_topk(f, scales, want_corr=False, want_H_cat=True, want_masks=True)
    assert len(masks) == len(scales)
    for s, H0, H, m in zip(scales, Hs0, Hs, masks):
        assert torch.equal(H, H0), f"scale {s}: H changed by asking for masks"
        assert m.row.shape == (B, H.shape[1]) and m.col.shape == (B, N)
        b = ops.incidence_masks(H)
        assert torch.equal(m.row, b.row) and torch.equal(m.col, b.col), f"scale {s}"
        _assert_masks(m, H, f"scale {s}")
        if s < N:      # rows have exactly k members (NaN and tie rules included)
            assert bool((H.sum(-1) == max(s, 1)).all())
    assert torch.equal(Hcat, Hcat0)


def test_fused_emission_refuses_n65():
    """N = 65 has no mask form: the Python face refuses before the launch."""
    from groupnet_amd import ops
    f = torch.randn(2, 65, 64, device=dev())
    with pytest.raises(ValueError, match="64"):
        ops.affinity_topk(f, [2], want_corr=False, want_masks=True)


# ---- gather and scatter -------------------------------------------------------------------------------------------------
def _groups(B, N, kind, seed):
    """[(H (B,E,N), masks)] with E = N, N, 1: top-k incidences with their emitted masks, or random ones through the builder."""
    from groupnet_amd import ops
    if kind == "topk":
        scales = [min(2, N), min(5, N), N] if N > 1 else [1, 1, 1]
        torch.manual_seed(seed)
        f = torch.randn(B, N, 64, device=dev())
        _, Hs, _, masks = ops.affinity_topk(f, scales, want_corr=False, want_masks=True)
        return list(zip(Hs, masks))
    Hs = [random_incidence(B, E, N, seed + i).to(dev()) for i, E in enumerate((N, N, 1))]
    return [(H, ops.incidence_masks(H)) for H in Hs]


@pytest.mark.parametrize("kind", ["topk", "random"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [1, 17, 33, 50, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_gather_and_scatter_mask_form_equals_dense(dtype, N, B, kind):
    from groupnet_amd import ops
    groups = _groups(B, N, kind, seed=7 * N + B)
    torch.manual_seed(N + B)
    oris = [torch.randn(B, N, 64, device=dev()).to(dtype) for _ in range(4)]
    feats = [torch.randn(B, H.shape[1], 64, device=dev()).to(dtype) for H, _ in groups]
    pfeat = torch.randn(B, N * (N + 1) // 2, 64, device=dev()).to(dtype)
    dense = ops.agg_gather_grouped([(o, H) for o, (H, _) in zip(oris, groups)] + [(oris[3], None, True)])
    for with_H in (True, False):       # H is not read in the mask form: it may be left out
        got = ops.agg_gather_grouped([(o, H if with_H else None, False, m) for o, (H, m) in zip(oris, groups)]
                                     + [(oris[3], None, True)])
        for g, (a, b) in enumerate(zip(got, dense)):
            assert torch.equal(a, b), f"gather group {g} (with_H={with_H})"
    for divisor in (float(N), 1.0):
        dense = ops.agg_scatter_grouped([(ft, H, o) for ft, o, (H, _) in zip(feats, oris, groups)]
                                        + [(pfeat, None, oris[3], True)], divisor)
        got = ops.agg_scatter_grouped([(ft, None, o, False, m) for ft, o, (_, m) in zip(feats, oris, groups)]
                                      + [(pfeat, None, oris[3], True)], divisor)
        for g, (a, b) in enumerate(zip(got, dense)):
            assert torch.equal(a, b), f"scatter group {g}, divisor {divisor}"
    # single-group faces
    H, m = groups[0]
    assert torch.equal(ops.agg_gather(oris[0], None, masks=m), ops.agg_gather(oris[0], H))
    assert torch.equal(ops.agg_scatter(feats[0], None, oris[0], masks=m), ops.agg_scatter(feats[0], H, oris[0]))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_packed_scenes_with_a_remainder(dtype):
    """N = 17 at a batch sized FROM THE EXPORTED PLAN so that several scenes share a workgroup (G > 1) and the last workgroup
    is short (B % G != 0); the write-only outputs are pre-filled with NaN, so an unwritten or overrun row shows."""
    from groupnet_amd import _lib, ops
    L, lib = _lib, _lib.load()
    N, Es = 17, (17, 17, 1)
    twin = dtype == torch.bfloat16
    sfx = "_bf16" if twin else "_f32"
    B = G = None
    for cand in (683, 1367, 2731, 5461):
        arr = (L.GatherGroup * 3)(*[L.GatherGroup(ori=16, eo=16, E=E, rowmask=16) for E in Es])
        plan = L.LaunchPlan()
        assert getattr(lib, "gn_agg_gather_plan" + sfx)(arr, 3, cand, N, ctypes.byref(plan)) == 0
        if plan.G > 1 and cand % plan.G != 0:
            B, G = cand, plan.G
            break
    assert B is not None and G > 1 and B % G != 0 and plan.kernel == L.K_AGG_GATHER_MASK
    torch.manual_seed(B)
    f = torch.randn(B, N, 64, device=dev())
    _, Hs, _, masks = ops.affinity_topk(f, [2, 5, N], want_corr=False, want_masks=True)
    oris = [torch.randn(B, N, 64, device=dev()).to(dtype) for _ in Es]
    feats = [torch.randn(B, E, 64, device=dev()).to(dtype) for E in Es]
    eos = [torch.full((B, E, 64), float("nan"), dtype=dtype, device=dev()) for E in Es]
    outs = [torch.full((B, N, 128), float("nan"), dtype=dtype, device=dev()) for _ in Es]
    ga = (L.GatherGroup * 3)(*[L.GatherGroup(ori=o.data_ptr(), eo=e.data_ptr(), E=E, rowmask=m.row.data_ptr())
                               for o, e, E, m in zip(oris, eos, Es, masks)])
    sa = (L.ScatterGroup * 3)(*[L.ScatterGroup(feat=ft.data_ptr(), ori=o.data_ptr(), out=y.data_ptr(), E=E,
                                               colmask=m.col.data_ptr())
                                for ft, o, y, E, m in zip(feats, oris, outs, Es, masks)])
    with torch.cuda.device(dev()):
        assert getattr(lib, "gn_agg_gather" + sfx)(ga, 3, B, N, L.stream_handle()) == 0
        assert getattr(lib, "gn_agg_scatter" + sfx)(sa, 3, B, N, float(N), L.stream_handle()) == 0
    want_eo = ops.agg_gather_grouped([(o, H) for o, H in zip(oris, Hs)])
    want_out = ops.agg_scatter_grouped([(ft, H, o) for ft, H, o in zip(feats, Hs, oris)])
    for g in range(3):
        assert not bool(torch.isnan(eos[g]).any()) and not bool(torch.isnan(outs[g]).any()), f"group {g}: unwritten rows"
        assert torch.equal(eos[g], want_eo[g]) and torch.equal(outs[g], want_out[g]), f"group {g} (B={B}, G={G})"


# ---- block level --------------------------------------------------------------------------------------------------------
def _spy(monkeypatch, log):
    """Every launch that goes through ops._fn: log gets (stem, kernel id of the gather's plan or None, mask words passed to
    the gather / scatter descriptors).  (The idea of tests/test_launch_forms_gpu.py `_spy_plans`.)"""
    from groupnet_amd import _lib, ops
    real = ops._fn

    def fn(stem, dt):
        f = real(stem, dt)

        def call(*a):
            kernel, words = None, None
            if stem == "gn_agg_gather":
                plan = _lib.LaunchPlan()
                assert real(stem + "_plan", dt)(*a[:-1], ctypes.byref(plan)) == 0
                kernel = plan.kernel
                words = sum(bool(a[0][g].rowmask) for g in range(a[1]))
            elif stem == "gn_agg_scatter":
                words = sum(bool(a[0][g].colmask) for g in range(a[1]))
            log.append((stem, kernel, words))
            return f(*a)
        return call
    monkeypatch.setattr(ops, "_fn", fn)


def _block(scales, nmp, seed):
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(seed)
    return MultiScaleHGNN(scales, nmp_layers=nmp).to(dev()).eval()


def _run_block(blk, x, noise, monkeypatch):
    """-> (out, new_H, [factors per module], launch log) of one forward with the injected noise."""
    from groupnet_amd import multiscale
    got, log = {}, []
    orig = multiscale.run_message_passing

    def keep(*a, **k):
        got["res"] = orig(*a, **k)
        return got["res"]
    with monkeypatch.context() as mp:
        mp.setattr(multiscale, "run_message_passing", keep)
        _spy(mp, log)
        with torch.no_grad():
            out, H = blk(x, noise_u=noise)
    return out, H, [r[1] for r in got["res"]], log


@pytest.mark.parametrize("N,scales,nmp", [(17, [2, 5, 17], 2), (50, [2, 4, 8, 16], 1)])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_block_mask_form_equals_dense(dtype, N, scales, nmp, monkeypatch, form):
    from groupnet_amd import _lib
    B, S = 6, len(scales)
    blk = _block(scales, nmp, seed=N)
    torch.manual_seed(N + 1)
    x = torch.randn(B, N, 64, device=dev()).to(dtype)
    noise = [[torch.rand(shp, device=dev()) for _ in range(nmp)] for shp in blk.noise_shapes(B, N)]
    form("dense")
    out_d, H_d, fac_d, log_d = _run_block(blk, x, noise, monkeypatch)
    form("mask")
    out_m, H_m, fac_m, log_m = _run_block(blk, x, noise, monkeypatch)
    assert torch.equal(out_m, out_d) and torch.equal(H_m, H_d)
    assert len(fac_m) == len(fac_d) == 1 + S and all(torch.equal(a, b) for a, b in zip(fac_m, fac_d))
    # the mask kernels really ran, once per round, for every hyper group — and the dense forward ran none
    gm, gd = [e for e in log_m if e[0] == "gn_agg_gather"], [e for e in log_d if e[0] == "gn_agg_gather"]
    sm, sd = [e for e in log_m if e[0] == "gn_agg_scatter"], [e for e in log_d if e[0] == "gn_agg_scatter"]
    assert gm == [("gn_agg_gather", _lib.K_AGG_GATHER_MASK, S)] * nmp and gd == [("gn_agg_gather", _lib.K_AGG_GATHER, 0)] * nmp
    assert sm == [("gn_agg_scatter", None, S)] * nmp and sd == [("gn_agg_scatter", None, 0)] * nmp
    # the fused launch emitted the masks itself (no tail, no builder launch)
    assert [e[0] for e in log_m].count("gn_affinity_topk") == 1
    assert _lib.load().gn_kernel_name(_lib.K_AGG_GATHER_MASK) == b"agg_gather_mask_kernel"


def test_switch_changes_no_launch_at_n11(monkeypatch, form):
    B, N, scales = 6, 11, [2, 5, 11]
    blk = _block(scales, 1, seed=3)
    torch.manual_seed(4)
    x = torch.randn(B, N, 64, device=dev())
    noise = [[torch.rand(shp, device=dev())] for shp in blk.noise_shapes(B, N)]
    form("dense")
    out_d, H_d, fac_d, log_d = _run_block(blk, x, noise, monkeypatch)
    form("mask")
    out_m, H_m, fac_m, log_m = _run_block(blk, x, noise, monkeypatch)
    assert log_m == log_d and len(log_d) > 0 and all(not e[2] for e in log_m)
    assert torch.equal(out_m, out_d) and torch.equal(H_m, H_d) and all(torch.equal(a, b) for a, b in zip(fac_m, fac_d))


def test_n70_stays_dense_silently(monkeypatch, form):
    from groupnet_amd import _lib
    B, N, scales = 2, 70, [2, 5]
    blk = _block(scales, 1, seed=5)
    torch.manual_seed(6)
    x = torch.randn(B, N, 64, device=dev())
    noise = [[torch.rand(shp, device=dev())] for shp in blk.noise_shapes(B, N)]
    form("dense")
    out_d, H_d, fac_d, log_d = _run_block(blk, x, noise, monkeypatch)
    form("mask")
    out_m, H_m, fac_m, log_m = _run_block(blk, x, noise, monkeypatch)
    assert log_m == log_d and ("gn_agg_gather", _lib.K_AGG_GATHER, 0) in log_m
    assert torch.equal(out_m, out_d) and torch.equal(H_m, H_d) and all(torch.equal(a, b) for a, b in zip(fac_m, fac_d))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_hyper_module_alone(dtype, monkeypatch, form):
    """MS_HGNN_hyper builds the masks of the H it built itself; a caller's H= stays dense unless masks= come with it."""
    import groupnet_amd as G
    from groupnet_amd import _lib, ops
    B, N, s = 5, 33, 4
    torch.manual_seed(9)
    mod = G.MS_HGNN_hyper(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=2,
                          scale=s).to(dev()).eval()
    h = torch.randn(B, N, 64, device=dev()).to(dtype)
    corr = ops.affinity(h.float())
    U = [torch.rand(B, N, 10, device=dev()) for _ in range(2)]

    def run(**kw):
        log = []
        with monkeypatch.context() as mp:
            _spy(mp, log)
            with torch.no_grad():
                res = mod(h, corr, noise_u=U, **kw)
        return res, [e for e in log if e[0] in ("gn_agg_gather", "gn_agg_scatter")]
    form("dense")
    (nf_d, fac_d, H_d), log_d = run()
    form("mask")
    (nf_m, fac_m, H_m), log_m = run()
    assert torch.equal(nf_m, nf_d) and torch.equal(fac_m, fac_d) and torch.equal(H_m, H_d)
    assert log_d == [("gn_agg_gather", _lib.K_AGG_GATHER, 0), ("gn_agg_scatter", None, 0)] * 2
    assert log_m == [("gn_agg_gather", _lib.K_AGG_GATHER_MASK, 1), ("gn_agg_scatter", None, 1)] * 2
    Hf = H_d.float().contiguous()
    (nf_h, fac_h, _), log_h = run(H=Hf)                                        # caller's H: dense
    assert log_h == log_d and torch.equal(nf_h, nf_d) and torch.equal(fac_h, fac_d)
    (nf_k, fac_k, _), log_k = run(H=Hf, masks=ops.incidence_masks(Hf))         # caller's H with its masks
    assert log_k == log_m and torch.equal(nf_k, nf_d) and torch.equal(fac_k, fac_d)
    (nf_w, _, _), log_w = run(H=2.0 * Hf)                                      # weight-2 rows: dense, other numbers
    assert log_w == log_d and not torch.equal(nf_w, nf_d)


def test_graph_replay_in_mask_form_equals_eager(monkeypatch, form):
    import groupnet_amd as G
    from groupnet_amd import _lib
    from groupnet_amd.graphs import GraphedMultiScale
    B, N = 6, 17
    blk = _block([2, 5, 17], 1, seed=11)
    torch.manual_seed(12)
    f = torch.randn(B, N, 64, device=dev())
    form("mask")
    log = []
    with monkeypatch.context() as mp:
        _spy(mp, log)
        g = GraphedMultiScale(blk, B, N, seed=77, warmup=1)
    # the last forward of the constructor is the captured one: its gather and scatter are the mask kernels
    assert [e for e in log if e[0] == "gn_agg_gather"][-1] == ("gn_agg_gather", _lib.K_AGG_GATHER_MASK, 3)
    assert [e for e in log if e[0] == "gn_agg_scatter"][-1] == ("gn_agg_scatter", None, 3)
    form("dense")                         # the graph keeps the form it was captured with
    o1, H1 = [t.clone() for t in g(f)]
    try:
        with torch.no_grad():
            G.set_noise_mode("device", seed=77, offset=0)
            e_dense = blk(f)
            form("mask")
            G.set_noise_mode("device", seed=77, offset=0)
            e_mask = blk(f)
    finally:
        G.set_noise_mode("host")
    assert torch.equal(o1, e_mask[0]) and torch.equal(H1, e_mask[1])
    assert torch.equal(o1, e_dense[0]) and torch.equal(H1, e_dense[1])


def test_past_encoder_mask_form_equals_dense(monkeypatch, form):
    """`_TrajectoryEncoder._encode`: the fused launch computes the embedding front-end AND emits the masks (its raw inputs and
    the mask words share the scene's LDS tile)."""
    import types
    from groupnet_amd import _lib
    from groupnet_amd.past_encoder import PastEncoder
    B, N, T = 4, 17, 5
    torch.manual_seed(21)
    enc = PastEncoder(types.SimpleNamespace(hidden_dim=64, hyper_scales=[2, 5, 17], past_length=T)).eval().to(dev())
    x = (torch.randn(B * N, T, 4) * 5).to(dev())

    def run():
        log = []
        torch.manual_seed(22)             # the encoder draws its own (host) noise: the same stream for both forms
        with monkeypatch.context() as mp:
            _spy(mp, log)
            with torch.no_grad():
                out, new_H = enc(x, B, N)
        return out, new_H, log
    form("dense")
    out_d, H_d, log_d = run()
    form("mask")
    out_m, H_m, log_m = run()
    assert torch.equal(out_m, out_d) and torch.equal(H_m, H_d)
    assert ("gn_agg_gather", _lib.K_AGG_GATHER, 0) in log_d and ("gn_agg_scatter", None, 0) in log_d
    assert ("gn_agg_gather", _lib.K_AGG_GATHER_MASK, 3) in log_m and ("gn_agg_scatter", None, 3) in log_m
