"""The bit-mask form of a hyperedge incidence (ABI 37), host side only — no kernel is launched: the new symbols and the
trailing descriptor fields exist, the gather's plan names the mask kernel and packs scenes by its own tile, the
launchers refuse N > 64 and mixed forms before anything is launched, the Python switch defaults to dense, and the numpy
statement of the two masks (tests/incidence_mask_cases.py, what the GPU tests compare the kernels with) round-trips
through H."""
import ctypes

import numpy as np
import pytest

from incidence_mask_cases import np_dense_from_cols, np_dense_from_rows, np_masks, random_incidence

P = ctypes.c_void_p
OK, ERR_NULL, ERR_SHAPE, ERR_ALIGN = 0, -1, -2, -4
kGsMinWgs = 2048            # workgroups a launch keeps when it packs scenes (gn_graph.hip)


def _lib():
    from groupnet_amd import _lib as L
    return L, L.load()


def _gather_plan(groups, B, N, twin=False):
    L, lib = _lib()
    arr = (L.GatherGroup * len(groups))(*[L.GatherGroup(**g) for g in groups])
    plan = L.LaunchPlan()
    rc = (lib.gn_agg_gather_plan_bf16 if twin else lib.gn_agg_gather_plan_f32)(arr, len(groups), B, N, ctypes.byref(plan))
    return rc, plan


def _scatter(groups, B, N, divisor=1.0):
    L, lib = _lib()
    arr = (L.ScatterGroup * len(groups))(*[L.ScatterGroup(**g) for g in groups])
    return lib.gn_agg_scatter_f32(arr, len(groups), B, N, divisor, P(0))


def test_symbols_and_trailing_fields():
    L, lib = _lib()
    from groupnet_amd import ops
    assert lib.gn_abi_version() == L.ABI_VERSION >= 37
    assert hasattr(lib, "gn_incidence_masks_f32") and "gn_incidence_masks_f32" in L.SIGNATURES
    # trailing: a descriptor filled by field name without the mask stays the dense / pairwise form
    assert L.GatherGroup._fields_[-1][0] == "rowmask" and L.ScatterGroup._fields_[-1][0] == "colmask"
    assert L.GatherGroup(ori=16, eo=16, E=4).rowmask is None and L.ScatterGroup(feat=16).colmask is None
    assert len(L.SIGNATURES["gn_affinity_topk_f32"][1]) == len(L.SIGNATURES["gn_affinity_topk_bf16"][1]) == 12
    assert lib.gn_kernel_name(L.K_AGG_GATHER) == b"agg_gather_kernel"
    assert lib.gn_kernel_name(L.K_AGG_GATHER_MASK) == b"agg_gather_mask_kernel"
    assert lib.gn_kernel_name(L.K_LAST + 1) is None
    for name in ("IncidenceMasks", "incidence_masks", "set_incidence_form", "incidence_form"):
        assert hasattr(ops, name), name


@pytest.mark.parametrize("twin", [False, True])
def test_gather_plan_names_the_mask_kernel(twin):
    L, _ = _lib()
    B, N = 6, 50
    masked = [dict(ori=16, eo=16, E=N, rowmask=32), dict(ori=16, eo=16, E=N, rowmask=32), dict(ori=16, eo=16, E=1, rowmask=32)]
    pair = dict(ori=16, eo=16, E=N * (N + 1) // 2, sym=1)
    rc, plan = _gather_plan(masked + [pair], B, N, twin)
    assert rc == OK and plan.kernel == L.K_AGG_GATHER_MASK and plan.precision == int(twin)
    assert plan.G == 1 and plan.TE == N and list(plan.grid) == [B, 1, 3]
    assert plan.dyn_lds == N * 64 * 4 + N * 8                 # the scene's ori rows and one word per hyperedge
    assert list(plan.pos[:4]) == [0, 1, 2, -1] and plan.pre_grid[3] > 0 and list(plan.wgs[:4]) == [B, B, B, 0]
    # H may stay in the descriptor (it is not read): still the mask form
    rc, plan = _gather_plan([dict(ori=16, eo=16, H=16, E=N, rowmask=32)], B, N, twin)
    assert rc == OK and plan.kernel == L.K_AGG_GATHER_MASK
    # ... and without masks the dense kernel with its own tile, as before
    rc, plan = _gather_plan([dict(ori=16, eo=16, H=16, E=N)], B, N, twin)
    assert rc == OK and plan.kernel == L.K_AGG_GATHER and plan.dyn_lds == N * 64 * 4 + N * N * 4


@pytest.mark.parametrize("N,nh", [(17, 3), (17, 1), (33, 2), (50, 4), (64, 1), (1, 1)])
def test_gather_plan_packs_scenes_by_the_mask_tile(N, nh):
    """G doubles while the doubled tile (ori rows + Emax words per scene) stays <= 24 KiB and the grid keeps kGsMinWgs
    workgroups — the dense rule on the smaller tile."""
    L, _ = _lib()
    per = N * 64 * 4 + N * 8
    for B in (1, 5, 683, 1367, 2731, 4096, 8191, 70001):
        G = 1
        while G < 16 and 2 * G * per <= 24 * 1024 and -(-B // (2 * G)) * nh >= kGsMinWgs:
            G *= 2
        rc, plan = _gather_plan([dict(ori=16, eo=16, E=N, rowmask=32)] * nh, B, N)
        assert rc == OK and plan.kernel == L.K_AGG_GATHER_MASK
        assert (plan.G, plan.dyn_lds, list(plan.grid)) == (G, G * per, [-(-B // G), 1, nh]), (B, N, nh)
        assert list(plan.spw[:nh]) == [G] * nh


def test_shape_form_and_pointer_errors_do_not_launch():
    _, lib = _lib()
    g = dict(ori=16, eo=16, E=4, rowmask=32)
    assert _gather_plan([g], 2, 64)[0] == OK
    assert _gather_plan([g], 2, 65)[0] == ERR_SHAPE                                         # a word holds 64 members
    assert _gather_plan([dict(g, sym=1)], 2, 17)[0] == ERR_SHAPE
    assert _gather_plan([dict(g, rowmask=36)], 2, 17)[0] == ERR_ALIGN
    assert _gather_plan([g, dict(ori=16, eo=16, H=16, E=4)], 2, 17)[0] == ERR_SHAPE           # mixed forms
    assert _gather_plan([g, dict(ori=16, eo=16, E=17 * 17)], 2, 17)[0] == OK                  # pairwise beside masks
    s = dict(feat=16, ori=16, out=16, E=4, colmask=32)
    assert _scatter([s], 2, 65) == ERR_SHAPE
    assert _scatter([dict(s, E=65)], 2, 17) == ERR_SHAPE
    assert _scatter([dict(s, sym=1)], 2, 17) == ERR_SHAPE
    assert _scatter([dict(s, colmask=36)], 2, 17) == ERR_ALIGN
    assert _scatter([s, dict(feat=16, ori=16, out=16, H=16, E=4)], 2, 17) == ERR_SHAPE       # mixed forms
    assert _scatter([dict(s, feat=0)], 2, 17) == ERR_NULL
    # builder
    assert lib.gn_incidence_masks_f32(P(16), 2, 65, 17, P(16), P(16), P(0), P(0)) == ERR_SHAPE
    assert lib.gn_incidence_masks_f32(P(16), 2, 17, 65, P(16), P(16), P(0), P(0)) == ERR_SHAPE
    assert lib.gn_incidence_masks_f32(P(16), 0, 17, 17, P(16), P(16), P(0), P(0)) == ERR_SHAPE
    assert lib.gn_incidence_masks_f32(P(0), 2, 17, 17, P(16), P(16), P(0), P(0)) == ERR_NULL
    assert lib.gn_incidence_masks_f32(P(16), 2, 17, 17, P(0), P(16), P(0), P(0)) == ERR_NULL
    assert lib.gn_incidence_masks_f32(P(16), 2, 17, 17, P(16), P(24), P(0), P(0)) == ERR_ALIGN
    # fused emission: both lists or none, N <= 64
    Hs, ks = (P * 1)(16), (ctypes.c_int * 1)(2)
    rows, cols = (P * 1)(16), (P * 1)(16)
    assert lib.gn_affinity_topk_f32(P(16), P(0), Hs, ks, 1, 2, 65, 64, None, rows, cols, P(0)) == ERR_SHAPE
    assert lib.gn_affinity_topk_f32(P(16), P(0), Hs, ks, 1, 2, 17, 64, None, rows, None, P(0)) == ERR_NULL
    assert lib.gn_affinity_topk_bf16(P(16), P(0), Hs, ks, 1, 2, 17, 64, None, rows, (P * 1)(0), P(0)) == ERR_NULL
    assert lib.gn_affinity_topk_f32(P(16), P(0), Hs, ks, 1, 2, 17, 64, None, (P * 1)(24), cols, P(0)) == ERR_ALIGN


def test_the_switch_defaults_to_dense(monkeypatch):
    from groupnet_amd import ops
    from groupnet_amd.MS_HGNN_batch import masks_apply
    monkeypatch.delenv("GN_INC_MASKS", raising=False)
    assert ops.incidence_form() == "dense" and not masks_apply(50)
    monkeypatch.setenv("GN_INC_MASKS", "1")                   # read per call
    assert ops.incidence_form() == "mask"
    assert [masks_apply(N) for N in (11, 16, 17, 50, 64, 65)] == [False, False, True, True, True, False]
    try:
        ops.set_incidence_form("dense")                       # an explicit choice wins over the environment
        assert ops.incidence_form() == "dense"
        monkeypatch.delenv("GN_INC_MASKS")
        ops.set_incidence_form("mask")
        assert ops.incidence_form() == "mask"
        with pytest.raises(ValueError):
            ops.set_incidence_form("sparse")
    finally:
        ops.set_incidence_form(None)
    assert ops.incidence_form() == "dense"


@pytest.mark.parametrize("B,E,N", [(3, 1, 1), (5, 17, 17), (4, 33, 33), (2, 64, 64), (2, 1, 64), (7, 50, 50)])
def test_numpy_statement_round_trips(B, E, N):
    H = random_incidence(B, E, N, seed=B * 100 + N).numpy()
    row, col = np_masks(H)
    assert row.shape == (B, E) and col.shape == (B, N) and row.dtype == col.dtype == np.int64
    assert np.array_equal(np_dense_from_rows(row, N), H) and np.array_equal(np_dense_from_cols(col, E), H)
    assert row[0, 0] == 0 and col[0, N - 1] == 0                                      # empty row, empty column
    assert int(row[1, E - 1]) == (-1 if N == 64 else (1 << N) - 1)                    # full row (bit 63: negative int64)
    # other weights than 1 set the same bits: the masks say "non-zero", the builder's flag says "not binary"
    H2 = H.copy()
    H2[H2 != 0] = 2.0
    assert all(np.array_equal(a, b) for a, b in zip(np_masks(H2), (row, col)))
