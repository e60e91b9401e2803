"""The bit-mask form of the incidence in the node -> edge launch and in training (gn_node2edge_masks_*; ABI 37, additive):

  * the row form reading member words against the dense row form, `torch.equal`, through the C ABI — member counts on both
    sides of the 16-member register path, empty and full rows, several scenes per workgroup with a ragged last one, and
    the banded fallback that ignores the words;
  * the inference block: which node -> edge entry point ran per round, with how many words, in which variant;
  * the backward's use of the scatter (divisor 1.0) in mask form;
  * training in mask form: a hyper module's gradients against torch autograd on the CPU oracle under the gates of
    tests/test_backward_gpu.py, a block's SGD step against the same step in dense form, the trajectory encoder, and a
    captured training step.

Forward results are compared with `torch.equal` (the forms are bit-identical on a 0/1 H); the two tolerances used — the
gradient gates and the split-K bound on updated weights — are those of tests/test_backward_gpu.py, not new ones."""
import copy
import ctypes
import types

import pytest
import torch

from incidence_mask_cases import random_incidence

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
P = ctypes.c_void_p


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def form():
    """Set the incidence form inside a test; the environment decides again afterwards."""
    from groupnet_amd import ops
    yield ops.set_incidence_form
    ops.set_incidence_form(None)


def _hyper_groups(B, N, kind, seed):
    """[(H (B,E,N), masks)] with E = N, N, 1: top-k incidences (scales 2, 5 and N: the all-ones edge has N members) with the
    masks their launch emitted, or random ones (an empty row, a full row, counts on both sides of 16) through the builder."""
    from groupnet_amd import ops
    if kind == "topk":
        scales = [min(2, N), min(5, N), N] if N > 1 else [1, 1, 1]
        torch.manual_seed(seed)
        f = torch.randn(B, N, 64, device=dev())
        _, Hs, _, masks = ops.affinity_topk(f, scales, want_corr=False, want_masks=True)
        return list(zip(Hs, masks))
    Hs = [random_incidence(B, E, N, seed + i).to(dev()) for i, E in enumerate((N, N, 1))]
    return [(H, ops.incidence_masks(H)) for H in Hs]


def _n2e_inputs(B, N, n, dtype, seed):
    """xp, pq per group (storage type), and the attention row w2 / bias b2 (fp32), scaled so that the softmax is not flat."""
    torch.manual_seed(seed)
    xps = [torch.randn(B, N, 64, device=dev()).to(dtype) for _ in range(n)]
    pqs = [torch.randn(B, N, 64, device=dev()).to(dtype) for _ in range(n)]
    w2s = [torch.randn(32, device=dev()) for _ in range(n)]
    b2s = [torch.randn(1, device=dev()) for _ in range(n)]
    return xps, pqs, w2s, b2s


def _masks_call(groups, xps, pqs, w2s, b2s, B, N, dtype, with_pair):
    """gn_node2edge_masks_* through the C ABI on NaN-filled outputs -> ([edges per group], plan of the same arguments)."""
    from groupnet_amd import _lib as L
    lib = L.load()
    sfx = "_bf16" if dtype == torch.bfloat16 else "_f32"
    Es = [H.shape[1] for H, _ in groups] + ([N * (N + 1) // 2] if with_pair else [])
    outs = [torch.full((B, E, 64), float("nan"), dtype=dtype, device=dev()) for E in Es]
    descs = [L.N2EGroup(xp=xp.data_ptr(), pq=pq.data_ptr(), H=H.data_ptr(), w2=w2.data_ptr(), edges=o.data_ptr(),
                        b2=b2.data_ptr(), E=H.shape[1])
             for (H, _), xp, pq, w2, b2, o in zip(groups, xps, pqs, w2s, b2s, outs)]
    words = [m.row.data_ptr() for _, m in groups]
    if with_pair:
        descs.append(L.N2EGroup(xp=xps[-1].data_ptr(), pq=pqs[-1].data_ptr(), w2=w2s[-1].data_ptr(),
                                edges=outs[-1].data_ptr(), b2=b2s[-1].data_ptr(), E=Es[-1], sym=1))
        words.append(None)
    arr, rows = (L.N2EGroup * len(descs))(*descs), (P * len(descs))(*words)
    plan = L.LaunchPlan()
    assert getattr(lib, "gn_node2edge_masks_plan" + sfx)(arr, rows, len(descs), B, N, ctypes.byref(plan)) == 0
    with torch.cuda.device(dev()):
        assert getattr(lib, "gn_node2edge_masks" + sfx)(arr, rows, len(descs), B, N, L.stream_handle()) == 0
    torch.cuda.synchronize()
    return outs, plan


def _dense_call(groups, xps, pqs, w2s, b2s, with_pair):
    from groupnet_amd import ops
    items = [(xp, pq, H, w2, b2) for (H, _), xp, pq, w2, b2 in zip(groups, xps, pqs, w2s, b2s)]
    if with_pair:
        items.append((xps[-1], pqs[-1], None, w2s[-1], b2s[-1], True))
    return ops.node2edge_grouped(items)


# ---- kernel against kernel ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ["1", "0"], ids=["rows", "banded"])
@pytest.mark.parametrize("kind", ["topk", "random"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("N", [1, 17, 33, 50, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_words_equal_dense(dtype, N, B, kind, rows, monkeypatch):
    """Three hyper groups with words and the pairwise group in one launch.  GN_N2E_ROWS=1 (read per call) makes both calls
    take the row form at these small shapes: variant 2 against variant 1.  GN_N2E_ROWS=0: the banded form, which ignores
    the words (variant 0)."""
    monkeypatch.setenv("GN_N2E_ROWS", rows)
    groups = _hyper_groups(B, N, kind, seed=11 * N + B)
    xps, pqs, w2s, b2s = _n2e_inputs(B, N, 4, dtype, seed=N + B)
    got, plan = _masks_call(groups, xps, pqs, w2s, b2s, B, N, dtype, with_pair=True)
    assert plan.variant == (2 if rows == "1" else 0) and plan.kernel == 14
    want = _dense_call(groups, xps, pqs, w2s, b2s, with_pair=True)
    for g, (a, b) in enumerate(zip(got, want)):
        assert not bool(torch.isnan(a).any()), f"group {g}: unwritten rows"
        assert torch.equal(a, b), f"group {g}"
    if N >= 17 and (kind == "topk" or B > 1):      # the cases hold what they are for: rows on both sides of the register path
        counts = torch.cat([H.sum(-1).flatten() for H, _ in groups])
        assert bool((counts > 16).any()) and bool((counts <= 16).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_several_scenes_per_workgroup_with_a_ragged_last_one(dtype, monkeypatch):
    """N = 17 in the row form at a batch sized FROM THE EXPORTED PLAN so that a workgroup holds several scenes (SGh > 1) and
    the last one is short (B % SGh != 0); NaN-filled outputs show an unwritten or overrun row."""
    from groupnet_amd import _lib as L
    from groupnet_amd import ops
    monkeypatch.setenv("GN_N2E_ROWS", "1")
    lib = L.load()
    N, Es = 17, (17, 17, 1)
    sfx = "_bf16" if dtype == torch.bfloat16 else "_f32"
    B = SG = None
    for cand in (683, 1367, 2731, 5461):
        arr = (L.N2EGroup * 3)(*[L.N2EGroup(xp=16, pq=16, H=16, w2=16, edges=16, b2=16, E=E) for E in Es])
        plan = L.LaunchPlan()
        assert getattr(lib, "gn_node2edge_masks_plan" + sfx)(arr, (P * 3)(32, 32, 32), 3, cand, N, ctypes.byref(plan)) == 0
        if plan.SGh > 1 and cand % plan.SGh != 0:
            B, SG = cand, plan.SGh
            break
    assert B is not None and SG > 1 and B % SG != 0 and plan.variant == 2
    torch.manual_seed(B)
    f = torch.randn(B, N, 64, device=dev())
    _, Hs, _, masks = ops.affinity_topk(f, [2, 5, N], want_corr=False, want_masks=True)
    groups = list(zip(Hs, masks))
    xps, pqs, w2s, b2s = _n2e_inputs(B, N, 3, dtype, seed=B + 1)
    got, plan = _masks_call(groups, xps, pqs, w2s, b2s, B, N, dtype, with_pair=False)
    assert plan.variant == 2 and plan.SGh == SG
    want = _dense_call(groups, xps, pqs, w2s, b2s, with_pair=False)
    for g, (a, b) in enumerate(zip(got, want)):
        assert not bool(torch.isnan(a).any()), f"group {g}: unwritten rows"
        assert torch.equal(a, b), f"group {g} (B={B}, SGh={SG})"


# ---- who launched what --------------------------------------------------------------------------------------------------
def _spy(mp, log):
    """Every launch that goes through ops._fn, and every call of the masks builder: log gets (stem, detail, words) with
    detail = the plan's kernel id for the gather, the plan's variant for the node -> edge launches; words = the number of
    groups that carry a member word."""
    from groupnet_amd import _lib, ops
    real, real_builder = ops._fn, ops.incidence_masks

    def fn(stem, dt):
        f = real(stem, dt)

        def call(*a):
            detail, words = None, None
            plan = _lib.LaunchPlan()
            if stem == "gn_agg_gather":
                assert real(stem + "_plan", dt)(*a[:-1], ctypes.byref(plan)) == 0
                detail, words = plan.kernel, sum(bool(a[0][g].rowmask) for g in range(a[1]))
            elif stem == "gn_agg_scatter":
                words = sum(bool(a[0][g].colmask) for g in range(a[1]))
            elif stem == "gn_node2edge_masks":
                assert real(stem + "_plan", dt)(*a[:-1], ctypes.byref(plan)) == 0
                detail, words = plan.variant, sum(bool(a[1][g]) for g in range(a[2]))
            elif stem == "gn_node2edge":
                assert real(stem + "_plan", dt)(*a[:-1], ctypes.byref(plan)) == 0
                detail, words = plan.variant, 0
            log.append((stem, detail, words))
            return f(*a)
        return call

    def builder(*a, **k):
        log.append(("gn_incidence_masks", None, None))
        return real_builder(*a, **k)
    mp.setattr(ops, "_fn", fn)
    mp.setattr(ops, "incidence_masks", builder)


def _of(log, stem):
    return [e for e in log if e[0] == stem]


def _block(scales, nmp, seed):
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(seed)
    return MultiScaleHGNN(scales, nmp_layers=nmp).to(dev()).eval()


def _run_block(blk, x, noise, monkeypatch):
    """-> (out, new_H, [factors per module], launch log) of one inference forward with the injected noise."""
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


BLOCK_CASES = [(17, [2, 5, 17], 2, None), (17, [2, 5, 17], 2, "1"), (50, [2, 4, 8, 16], 1, None)]


@pytest.mark.parametrize("N,scales,nmp,rows", BLOCK_CASES, ids=["N17", "N17-rows", "N50"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_inference_block_reads_the_words(dtype, N, scales, nmp, rows, monkeypatch, form):
    """One gn_node2edge_masks launch per round with a word for each hyper group; N = 17, B = 6 stays banded by the launch
    size (the words are then ignored) unless GN_N2E_ROWS=1 forces the row form, N = 50 takes it by the rule (E >= 24)."""
    if rows is None:
        monkeypatch.delenv("GN_N2E_ROWS", raising=False)
    else:
        monkeypatch.setenv("GN_N2E_ROWS", rows)
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
    row_form = rows == "1" or N == 50
    assert _of(log_m, "gn_node2edge_masks") == [("gn_node2edge_masks", 2 if row_form else 0, S)] * nmp
    assert _of(log_m, "gn_node2edge") == []
    assert _of(log_d, "gn_node2edge_masks") == []
    assert _of(log_d, "gn_node2edge") == [("gn_node2edge", 1 if row_form else 0, 0)] * nmp


# ---- the backward's scatter ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [17, 50])
def test_scatter_with_divisor_one(N):
    """d ori += H^T d eo: the scatter with divisor 1.0 and the pairwise group beside, as `round_backward` calls it."""
    from groupnet_amd import ops
    B = 3
    groups = _hyper_groups(B, N, "topk", seed=N)
    torch.manual_seed(N)
    oris = [torch.randn(B, N, 64, device=dev()) for _ in range(4)]
    feats = [torch.randn(B, H.shape[1], 64, device=dev()) for H, _ in groups]
    pfeat = torch.randn(B, N * (N + 1) // 2, 64, device=dev())
    dense = ops.agg_scatter_grouped([(ft, H, o, False) for ft, o, (H, _) in zip(feats, oris, groups)]
                                    + [(pfeat, None, oris[3], True)], 1.0)
    got = ops.agg_scatter_grouped([(ft, H, o, False, m) for ft, o, (H, m) in zip(feats, oris, groups)]
                                  + [(pfeat, None, oris[3], True)], 1.0)
    assert len(got) == len(dense) == 4
    for g, (a, b) in enumerate(zip(got, dense)):
        assert torch.equal(a, b), f"group {g}"


# ---- training -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,scale,nmp", [(3, 20, 2, 1), (2, 50, 8, 1), (2, 33, 33, 1), (2, 17, 5, 2)])
def test_hyper_module_gradients_in_mask_form(B, N, scale, nmp, monkeypatch):
    """tests/test_backward_gpu.py `test_hyper_module_gradients` under the mask form, with that file's gates (2e-3 of
    max|grad| on any batch, 2e-5 on clean scenes, against torch autograd on the CPU oracle), and what was launched: per
    round the forward's node -> edge launch, gather and scatter and the backward's two gathers and one scatter all carry
    a word; the module builds its masks once per forward; no dense gather runs."""
    from groupnet_amd import _lib, ops
    from oracle import ms_hgnn_oracle as O
    from test_backward_gpu import TOL_ANY, TOL_CLEAN, _grad_compare, _modules      # noqa: F401  (the gates live there)
    assert (TOL_ANY, TOL_CLEAN) == (2e-3, 2e-5)
    monkeypatch.delenv("GN_N2E_ROWS", raising=False)
    _, hyper = _modules(100 + N, nmp)
    hyper.scale = scale
    h = torch.randn(B, N, 64)
    corr = O.affinity(h)
    U = [torch.rand(s) for s in O.noise_shapes(B, N, scale, nmp)]
    Hs, log, forwards = {}, [], []

    def oracle_fwd(state, hh, nz):
        c = corr if hh.shape[0] == B else O.affinity(hh.detach())
        nf, fac, H = O.ms_hgnn_hyper_forward(state, hh, c, scale, nz, nmp_layers=nmp, decomposed=True)
        Hs["ref"], Hs["corr"] = H, c
        return nf, fac

    def hip_fwd(x, nz):
        forwards.append(x.shape[0])
        nf, fac, H = hyper(x, Hs["corr"].to(x.device), noise_u=nz)
        assert torch.equal(H.cpu(), Hs["ref"])
        return nf, fac

    ops.set_incidence_form("mask")
    try:
        with monkeypatch.context() as mp:
            _spy(mp, log)
            hip, _ = _grad_compare(f"hyper, mask form, B={B} N={N} s={scale} nmp={nmp}", hyper, oracle_fwd, hip_fwd, h, U,
                                   40 * nmp)
        assert hip["spatial_embedding.weight"] is None and hip["edge_aggregation_list.0.mlp.layers.0.weight"] is None
        F = len(forwards)                                    # whole batch, and the clean scenes alone when some are not
        assert F >= 1
        n2e, gat, sca = _of(log, "gn_node2edge_masks"), _of(log, "gn_agg_gather"), _of(log, "gn_agg_scatter")
        assert len(n2e) == F * nmp and all(e[2] == 1 for e in n2e) and _of(log, "gn_node2edge") == []
        if N == 50:
            assert all(e[1] == 2 for e in n2e)                # E = 50 >= 24: the row form, reading the word
        assert len(gat) == F * nmp * (1 + 2) and all(e == ("gn_agg_gather", _lib.K_AGG_GATHER_MASK, 1) for e in gat)
        assert len(sca) == F * nmp * (1 + 1) and all(e == ("gn_agg_scatter", None, 1) for e in sca)
        assert len(_of(log, "gn_incidence_masks")) == F
        # one training forward with fixed noise in each form: the same bits
        x = h.to(dev()).requires_grad_(True)
        nz = [u.to(dev()) for u in U]
        c = corr.to(dev())
        log_m, log_d = [], []
        with monkeypatch.context() as mp:
            _spy(mp, log_m)
            nf_m, fac_m, H_m = hyper(x, c, noise_u=nz)
        ops.set_incidence_form("dense")
        with monkeypatch.context() as mp:
            _spy(mp, log_d)
            nf_d, fac_d, H_d = hyper(x, c, noise_u=nz)
        assert nf_m.requires_grad and nf_d.requires_grad
        assert torch.equal(nf_m, nf_d) and torch.equal(fac_m, fac_d) and torch.equal(H_m, H_d)
        assert len(_of(log_m, "gn_node2edge_masks")) == nmp and _of(log_d, "gn_node2edge_masks") == []
        assert all(e[2] == 0 for e in log_d if e[2] is not None) and _of(log_d, "gn_incidence_masks") == []
    finally:
        ops.set_incidence_form(None)


def _sgd_step(blk, f, tgt, noise, monkeypatch):
    """One eager SGD step (lr 0.05) -> (loss, launch log)."""
    log = []
    opt = torch.optim.SGD(blk.parameters(), lr=0.05)
    opt.zero_grad()
    with monkeypatch.context() as mp:
        _spy(mp, log)
        out, _ = blk(f, noise_u=noise)
        loss = ((out - tgt) ** 2).mean()
        loss.backward()
    opt.step()
    return loss.detach().clone(), log


def test_block_training_step_in_mask_form(monkeypatch, form):
    """One SGD step of the block from the same weights in each form: the loss bit-equal (the forward is deterministic), the
    updated parameters within 1e-5 (1 + max|p|) — the bound tests/test_backward_gpu.py
    `test_graphed_train_step_matches_eager_and_learns` uses for the split-K atomics of the weight gradients.  The masks come
    out of the one fused affinity + top-k launch: no builder launch."""
    from groupnet_amd import _lib
    from groupnet_amd.multiscale import MultiScaleHGNN
    monkeypatch.delenv("GN_N2E_ROWS", raising=False)
    B, N, scales = 4, 17, [2, 5, 17]
    S = len(scales)
    torch.manual_seed(31)
    blk_d = MultiScaleHGNN(scales).to(dev()).train()
    blk_m = copy.deepcopy(blk_d)
    start = [p.detach().clone() for p in blk_d.parameters()]
    f = torch.randn(B, N, 64, device=dev())
    tgt = torch.randn(B, N, blk_d.out_features, device=dev())
    noise = [[torch.rand(s, device=dev())] for s in blk_d.noise_shapes(B, N)]
    form("dense")
    loss_d, log_d = _sgd_step(blk_d, f, tgt, noise, monkeypatch)
    form("mask")
    loss_m, log_m = _sgd_step(blk_m, f, tgt, noise, monkeypatch)
    assert torch.equal(loss_m, loss_d)
    for (name, pm), (_, pd) in zip(blk_m.named_parameters(), blk_d.named_parameters()):
        assert float((pm - pd).abs().max()) <= 1e-5 * (1.0 + float(pd.abs().max())), name
    assert max(float((p - q).abs().max()) for p, q in zip(blk_m.parameters(), start)) > 0.0      # the step did step
    assert len(_of(log_m, "gn_affinity_topk")) == 1 and _of(log_m, "gn_incidence_masks") == []
    # forward: the S hyper groups carry words beside the pairwise group; backward: two gathers, one scatter
    assert _of(log_m, "gn_node2edge_masks") == [("gn_node2edge_masks", 0, S)] and _of(log_m, "gn_node2edge") == []
    assert _of(log_m, "gn_agg_gather") == [("gn_agg_gather", _lib.K_AGG_GATHER_MASK, S)] * 3
    assert _of(log_m, "gn_agg_scatter") == [("gn_agg_scatter", None, S)] * 2
    assert _of(log_d, "gn_node2edge_masks") == [] and all(e[2] == 0 for e in log_d if e[2] is not None)


def test_past_encoder_training_forward_in_mask_form(monkeypatch, form):
    """`PastEncoder` in train mode (dropout 0): the training path draws its masks from the fused launch as the block's does;
    outputs bit-equal between the forms."""
    from groupnet_amd.past_encoder import PastEncoder
    monkeypatch.delenv("GN_N2E_ROWS", raising=False)
    B, N, T = 4, 17, 5
    torch.manual_seed(41)
    enc = PastEncoder(types.SimpleNamespace(hidden_dim=64, hyper_scales=[5, 17], past_length=T)).to(dev()).train()
    enc.pos_encoder.dropout.p = 0.0
    x = (torch.randn(B * N, T, 4) * 5).to(dev())

    def run():
        log = []
        torch.manual_seed(42)             # the encoder draws its own (host) noise: the same stream for both forms
        with monkeypatch.context() as mp:
            _spy(mp, log)
            out, new_H = enc(x, B, N)
        return out, new_H, log
    form("dense")
    out_d, H_d, log_d = run()
    form("mask")
    out_m, H_m, log_m = run()
    assert out_m.requires_grad and out_d.requires_grad
    assert torch.equal(out_m, out_d) and torch.equal(H_m, H_d)
    assert _of(log_m, "gn_node2edge_masks") == [("gn_node2edge_masks", 0, 2)] and _of(log_d, "gn_node2edge_masks") == []
    assert _of(log_m, "gn_incidence_masks") == [] and len(_of(log_m, "gn_affinity_topk")) == 1
    out_m.sum().backward()                # the backward runs in the same form
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in enc.parameters())


def test_graphed_training_step_in_mask_form(form):
    """`GraphedTrainStep` captured in mask form: the first replay against the same step run eagerly in mask form (loss within
    1e-6 relative, weights within 1e-5 (1 + max|p|): the comparison of tests/test_backward_gpu.py
    `test_graphed_train_step_matches_eager_and_learns`), then three more replays reduce the loss."""
    import groupnet_amd as G
    from groupnet_amd.graphs import GraphedTrainStep
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(3)
    B, N = 16, 17
    blk = MultiScaleHGNN([2, 5, 17]).to(dev()).train()
    ref = copy.deepcopy(blk)
    f = torch.randn(B, N, 64, device=dev())
    tgt = torch.randn(B, N, blk.out_features, device=dev())
    loss_fn = lambda out, H, t: ((out - t) ** 2).mean()
    form("mask")
    step = GraphedTrainStep(blk, torch.optim.SGD(blk.parameters(), lr=0.05), loss_fn, B, N,
                            target_shapes=[tuple(tgt.shape)], seed=11, warmup=2)
    # the warm-up steps trained `blk`; restart both from the same weights
    blk.load_state_dict(ref.state_dict())
    G.MS_HGNN_batch.invalidate_weight_caches(blk)
    l0 = float(step(f, tgt))
    opt = torch.optim.SGD(ref.parameters(), lr=0.05)
    counter = torch.zeros(1, dtype=torch.int64, device=dev())
    G.set_noise_mode("device", seed=11, offset=0, counter=counter)
    try:
        out, _ = ref(f)
        loss = loss_fn(out, None, tgt)
        loss.backward()
        opt.step()
    finally:
        G.set_noise_mode("host")
    assert abs(float(loss) - l0) <= 1e-6 * max(1.0, abs(l0))
    for (n1, p1), (_, p2) in zip(blk.named_parameters(), ref.named_parameters()):
        assert float((p1 - p2).abs().max()) <= 1e-5 * (1.0 + float(p2.abs().max())), n1
    losses = [l0] + [float(step()) for _ in range(3)]
    assert losses[-1] < losses[0]
