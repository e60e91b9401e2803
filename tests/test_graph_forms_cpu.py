"""The stage that builds the graph — cosine affinity, then the top-k incidence — at its form edges, without a GPU and
without a launch: what the case table of tests/test_graph_forms_gpu.py reaches (tests/launch_forms.py `graph_forms`, the
tests' own statement of the launchers' arithmetic), and that statement and `groupnet_amd.ops.graph_form` against the C
library at every switch point.

The library is asked through its plan queries (`gn_affinity_plan_f32`, `gn_topk_incidence_plan_f32`,
`gn_affinity_topk_plan_f32`, `gn_node_mlp_plan_f32`) with aligned placeholder addresses: GN_OK and the planned kernel,
grid and LDS where a launch would follow, the launcher's error code where it would not."""
import ctypes
import os
import subprocess
import sys

import pytest

from launch_forms import (AFF_LDS_BUDGET, AFF_TAIL_LDS, AFFINITY_CASES, AFFINITY_D_CASES, ENGINE_CASES, FUSED_CASES,
                          PLACEHOLDER, TOPK_CASES, affinity_tile, graph_forms, largest_fused_n, topk_bands)

GN_OK, GN_ERR_LDS = 0, -6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from groupnet_amd import _lib as L
    return L, L.load()


def test_case_table_reaches_every_form():
    """The shapes of the GPU tests reach all three forms, both sides of both switch points, every regime of the stand-alone
    top-k launcher's band size, and the ragged bands and panels of the banded affinity."""
    forms = {(B, N): graph_forms(B, N) for B, N in FUSED_CASES + ENGINE_CASES + [(B, N) for B, N, D in AFFINITY_CASES]}
    assert {f["form"] for f in forms.values()} == {"tail", "fused", "banded"}
    by_n = {N: f["form"] for (B, N), f in forms.items()}
    assert (by_n[40], by_n[41], by_n[112], by_n[113]) == ("tail", "fused", "fused", "banded")
    for cases in (FUSED_CASES, ENGINE_CASES):
        assert {40, 41} <= {N for _, N in cases}
    assert {112, 113} <= {N for _, N in ENGINE_CASES} and {112, 113} <= {N for _, N, _ in AFFINITY_CASES}
    # the switch points are where the formulas put them, and the largest fused tile is the one the issue names
    assert largest_fused_n(64, budget=AFF_TAIL_LDS) == 40 and largest_fused_n(64) == 112
    assert (largest_fused_n(64, 20), largest_fused_n(64, 40), largest_fused_n(128)) == (107, 103, 99)
    assert affinity_tile(112) == 130824 and max(f["tile"] for f in forms.values() if f["form"] == "fused") == 130824
    assert {(N, D) for _, N, D in AFFINITY_D_CASES} >= {(11, 4), (11, 36), (11, 128), (99, 128), (100, 128)}
    assert [graph_forms(B, N, D)["form"] for B, N, D in AFFINITY_D_CASES if N > 11] == ["fused", "banded"]

    # stand-alone top-k: (RB, remainder) per case as the launcher's arithmetic gives them
    bands = {c: topk_bands(*c) for c in TOPK_CASES}
    assert {c: (b[0], b[2]) for c, b in bands.items()} == {(1024, 11): (11, 0), (1024, 113): (113, 0), (1024, 200): (81, 38),
                                                         (300, 200): (41, 36), (3, 200): (6, 2), (2, 113): (8, 1)}
    cap = lambda N: (AFF_LDS_BUDGET // 2) // (4 * N)
    assert any(RB == N and n == 1 for (B, N), (RB, n, rem) in bands.items())                    # all N rows in one band
    assert any(RB == cap(N) < N and rem for (B, N), (RB, n, rem) in bands.items())              # the LDS cap, short last band
    assert any(8 < RB < min(cap(N), N) and rem for (B, N), (RB, n, rem) in bands.items())       # halved, with a remainder
    assert any(RB < 8 for RB, n, rem in bands.values())
    assert any(RB == 8 and rem == 1 for RB, n, rem in bands.values())
    # the engine's banded cases agree with the direct ones (graph_forms reports the same arithmetic)
    assert graph_forms(2, 113)["topk"] == bands[(2, 113)] and graph_forms(1, 113)["topk"] == (8, 15, 1)

    # banded affinity: a last band of one row, a short last 64-column panel, and the exact shape
    banded = [graph_forms(B, N, D) for B, N, D in AFFINITY_CASES if graph_forms(B, N, D)["form"] == "banded"]
    last = [f["aff_last"] for f in banded]
    assert last == [(1, 49), (1, 1), (8, 8), (16, 64)]
    assert [f["aff_grid"] for f in banded] == [(8, 2), (9, 2), (13, 1), (16, 3)]


def _name(plan):
    return _lib()[1].gn_kernel_name(plan.kernel).decode()


def _fused_args(N, D, x_dim=0, mask_scales=0):
    """The arguments of gn_affinity_topk_f32 / its plan query up to `colmask_list`, placeholder addresses throughout."""
    L, lib = _lib()
    P = PLACEHOLDER
    n = max(1, mask_scales)
    Hl, kl = (ctypes.c_void_p * n)(*[P] * n), (ctypes.c_int * n)(*[1] * n)
    ex = L.BlockExtras(f_out=P, f_out_ld=D)
    if x_dim:
        ex.x_raw, ex.x_dim, ex.M, ex.c, ex.f_contig = P, x_dim, P, P, P
    words = (ctypes.c_void_p * n)(*[P] * n) if mask_scales else None
    return (P, None, Hl, kl, n, 1, N, D, ctypes.byref(ex), words, words), ex


def _fused_rc(N, D, x_dim=0, mask_scales=0):
    """(return code, plan) of gn_affinity_topk_plan_f32 for placeholder addresses."""
    L, lib = _lib()
    args, keep = _fused_args(N, D, x_dim, mask_scales)
    plan = L.LaunchPlan()
    return lib.gn_affinity_topk_plan_f32(*args, ctypes.byref(plan)), plan


@pytest.mark.parametrize("D,x_dim,mask_scales", [(64, 0, 0), (64, 20, 0), (64, 40, 0), (4, 0, 0), (128, 0, 0), (1024, 0, 0),
                                                 (1024, 0, 8)])
def test_fused_launch_budget_is_the_one_python_states(D, x_dim, mask_scales):
    """The largest N whose tile fits answers GN_OK with that tile as the launch's LDS, N + 1 answers GN_ERR_LDS — from the
    plan query and from the launcher entry itself, which launches nothing there; `graph_forms` and `ops.graph_form` say the
    same.  (1024, 0, 8): with mask lists — the mask words of eight scales move the switch point from 30 | 31 to 29 | 30, so
    the case reads the mask term and not only the tile."""
    from groupnet_amd import ops
    _, lib = _lib()
    N = largest_fused_n(D, x_dim, mask_scales)
    if (D, x_dim) == (64, 0):
        assert N == 112
    if D == 1024:
        assert N == (29 if mask_scales else 30)
    (rc, plan), (rc1, _) = _fused_rc(N, D, x_dim, mask_scales), _fused_rc(N + 1, D, x_dim, mask_scales)
    assert (rc, rc1) == (GN_OK, GN_ERR_LDS)
    assert plan.dyn_lds == affinity_tile(N, D, x_dim, mask_scales) and list(plan.grid) == [1, 1, 1]
    assert _name(plan) == ("affinity_topk_masks_kernel" if mask_scales else "affinity_topk_kernel")
    args, keep = _fused_args(N + 1, D, x_dim, mask_scales)
    assert lib.gn_affinity_topk_f32(*args, None) == GN_ERR_LDS
    scales = [1] * mask_scales
    for n, fits in ((N, True), (N + 1, False)):
        assert (ops.graph_form(n, D, x_dim, mask_scales) != "banded") is fits
        assert (graph_forms(1, n, D, x_dim, bool(mask_scales), scales)["form"] != "banded") is fits


def _tail_rc(N, x_dim=0, D=64, B=3):
    """(return code, plan) of the node stage's plan query with an affinity job of placeholder addresses."""
    L, lib = _lib()
    P = PLACEHOLDER
    g = (L.NodeGroup * 1)(L.NodeGroup(x=P, Wx=P, bias=P, xp=P, pq=P))
    Hl, kl = (ctypes.c_void_p * 1)(P), (ctypes.c_int * 1)(1)
    ex = L.BlockExtras(f_out=P, f_out_ld=D)
    if x_dim:
        ex.x_raw, ex.x_dim, ex.M, ex.c, ex.f_contig = P, x_dim, P, P, P
    job = L.AffinityJob(f=P, H_list=Hl, k_list=kl, n_scales=1, B=B, N=N, D=D, extras=ctypes.pointer(ex))
    plan = L.LaunchPlan()
    return lib.gn_node_mlp_plan_f32(g, 1, B * N, ctypes.byref(job), ctypes.byref(plan)), plan


@pytest.mark.parametrize("x_dim,N", [(0, 40), (20, 37)])
def test_tail_budget_is_the_one_python_states(x_dim, N):
    """The node stage takes the job up to N (40; 37 with 20 raw inputs per agent) and refuses N + 1 with GN_ERR_LDS — the
    plan query and the launcher entry alike; `ops.graph_form` — what `AffinityTail.fits_tail` asks — and `graph_forms` say
    the same, raw inputs counted."""
    from groupnet_amd import ops
    L, lib = _lib()
    assert lib.gn_affinity_tail_lds_limit() == AFF_TAIL_LDS
    assert N == largest_fused_n(64, x_dim, budget=AFF_TAIL_LDS)
    (rc, plan), (rc1, _) = _tail_rc(N, x_dim), _tail_rc(N + 1, x_dim)
    assert (rc, rc1) == (GN_OK, GN_ERR_LDS)
    assert plan.dyn_lds == affinity_tile(N, 64, x_dim) and _name(plan) == "node_stage_kernel"
    # the launcher entry at N + 1: refused before anything is launched
    P = PLACEHOLDER
    g = (L.NodeGroup * 1)(L.NodeGroup(x=P, Wx=P, bias=P, xp=P, pq=P))
    Hl, kl = (ctypes.c_void_p * 1)(P), (ctypes.c_int * 1)(1)
    ex = L.BlockExtras(x_raw=P, x_dim=x_dim, M=P, c=P, f_contig=P) if x_dim else L.BlockExtras()
    job = L.AffinityJob(f=P, H_list=Hl, k_list=kl, n_scales=1, B=3, N=N + 1, D=64, extras=ctypes.pointer(ex))
    assert lib.gn_node_mlp_affinity_f32(g, 1, 3 * (N + 1), ctypes.byref(job), None) == GN_ERR_LDS
    for n, fits in ((N, True), (N + 1, False)):
        assert (ops.graph_form(n, 64, x_dim) == "tail") is fits
        assert (graph_forms(3, n, 64, x_dim)["form"] == "tail") is fits


def test_graph_form_is_the_tests_statement_everywhere():
    """`ops.graph_form` against `graph_forms` over every N up to beyond the last switch point, with and without raw inputs
    and mask words."""
    from groupnet_amd import _lib as L, ops
    with pytest.raises(L.GroupNetHipError):
        ops.graph_form(65, 64, 0, 1)
    for x_dim, ms in ((0, 0), (20, 0), (0, 3), (0, 8)):
        for N in range(1, 65 if ms else 120):      # (mask words: N <= 64, else the query raises as the launch would)
            assert ops.graph_form(N, 64, x_dim, ms) == graph_forms(1, N, 64, x_dim, bool(ms), [1] * ms)["form"], (N, x_dim, ms)


def _topk_plan(B, N):
    L, lib = _lib()
    P = PLACEHOLDER
    Hl, kl = (ctypes.c_void_p * 1)(P), (ctypes.c_int * 1)(2)
    plan = L.LaunchPlan()
    return lib.gn_topk_incidence_plan_f32(P, Hl, kl, 1, B, N, ctypes.byref(plan)), plan


def test_topk_plan_is_the_band_arithmetic_python_states():
    """`topk_bands` against gn_topk_incidence_plan_f32 for the GPU cases and the engine's banded cases: rows per band in
    TE, grid (bands, B), a band of rows as the LDS; GN_ERR_LDS, before any division, where not one row fits."""
    for B, N in TOPK_CASES + [(B, N) for B, N in ENGINE_CASES if graph_forms(B, N)["form"] == "banded"] + [(1, 16384)]:
        rc, plan = _topk_plan(B, N)
        RB, bands, rem = topk_bands(B, N)
        assert rc == GN_OK and _name(plan) == "topk_incidence_kernel", (B, N)
        assert (plan.TE, list(plan.grid), plan.dyn_lds) == (RB, [bands, B, 1], RB * N * 4), (B, N)
    for N in (16385, 32768):
        assert topk_bands(1, N) is None and _topk_plan(1, N)[0] == GN_ERR_LDS


def test_affinity_plan_is_the_form_python_states():
    """`graph_forms` against gn_affinity_plan_f32 for every stand-alone affinity case: the fused kernel on (B) workgroups
    with the fused tile, or the banded kernel on `aff_grid` with 16 band rows and a 64-column panel at stride D + 4."""
    L, lib = _lib()
    P = PLACEHOLDER
    for B, N, D in AFFINITY_CASES + AFFINITY_D_CASES:
        plan = L.LaunchPlan()
        assert lib.gn_affinity_plan_f32(P, P, B, N, D, ctypes.byref(plan)) == GN_OK
        form = graph_forms(B, N, D)
        if form["form"] == "banded":
            assert _name(plan) == "affinity_banded_kernel" and tuple(plan.grid) == form["aff_grid"] + (1,), (B, N, D)
            assert plan.dyn_lds == 80 * (D + 4) * 4
        else:
            assert _name(plan) == "affinity_topk_kernel" and list(plan.grid) == [B, 1, 1], (B, N, D)
            assert plan.dyn_lds == affinity_tile(N, D) == form["tile"]


_TOPK_CHILD = """
import ctypes, sys
from groupnet_amd import _lib as L
lib = L.load()
P = 4096
Hl, kl = (ctypes.c_void_p * 1)(P), (ctypes.c_int * 1)(2)
print(*[lib.gn_topk_incidence_f32(P, Hl, kl, 1, 1, N, None) for N in (16385, 32768)])
"""


def test_topk_entry_refuses_rows_beyond_its_band():
    """gn_topk_incidence_f32 stages whole rows of corr in 64 KiB: N = 16 384 is the last N a band of one row holds.  At
    N = 16 385 and 32 768 the entry answers GN_ERR_LDS before it sizes a band (the band size would be 0, and the grid is a
    division by it).  Asked in a child process: a regression dies of SIGFPE there and fails here."""
    assert topk_bands(1, 16384) == (1, 16384, 0) and topk_bands(1, 16385) is None and topk_bands(1, 32768) is None
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in [os.environ.get("PYTHONPATH")] if p]))
    r = subprocess.run([sys.executable, "-c", _TOPK_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-500:])
    assert r.stdout.split() == [str(GN_ERR_LDS)] * 2, r.stdout
