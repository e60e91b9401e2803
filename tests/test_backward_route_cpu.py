"""`groupnet_amd.route.backward_round_route` — the forms `backward.round_backward` follows — over its whole input grid
against the rules as `round_backward` stated them inline before the route existed, and its one limit against the C library
(no GPU, no launch).  Each rule below is one expression of the former function, written out again here; a predicate
edited in the route fails in this file."""
import importlib.util
import itertools
import sys

import pytest

from groupnet_amd import route as R
from launch_forms import PLACEHOLDER

NS = (1, 16, 60, 61, 140, 141, 150, 1024)
D = 64


def scene_fits(N):
    """The LDS rule of the per-scene node->edge backward as backward.py wrote it out (twice)."""
    return (4 * N * D + 64 + 16 * N) * 4 <= 150 * 1024


def pairwise_tuples():
    return [p for n in range(1, 5) for p in itertools.product((False, True), repeat=n)]


def test_the_round_route_is_the_former_inline_rules():
    n = 0
    for N, pairwise in itertools.product(NS, pairwise_tuples()):
        got = R.backward_round_route(N, pairwise)
        fits = scene_fits(N)
        syms = [pw and fits for pw in pairwise]                      # sym = Hx is None and scene_fits
        kept = all(sym or not pw for sym, pw in zip(syms, pairwise))    # all(c["sym"] or c["H"] is not None and tr.H is not None)
        grouped = fits                                               # scene_form (every module has the round's B and N)
        assert (got.kept, got.n2e_grouped) == (kept, grouped), (N, pairwise)
        assert [pw and got.pair_rows for pw in pairwise] == syms, (N, pairwise)
        assert got.pair_rows == fits                                 # (also where no module is pairwise: nobody reads it)
        n += 1
    assert n == len(NS) * (2 + 4 + 8 + 16)


def test_the_limit_is_the_largest_n_that_fits():
    assert scene_fits(R.N2E_BWD_SCENE_MAX_N) and not scene_fits(R.N2E_BWD_SCENE_MAX_N + 1)
    assert all(scene_fits(N) == (N <= R.N2E_BWD_SCENE_MAX_N) for N in range(1, 2049))
    bytes_at = lambda N: (4 * N * D + 64 + 16 * N) * 4
    assert (bytes_at(140), bytes_at(141), R.N2E_BWD_SCENE_MAX_N) == (152576, 153664, 140)


def test_the_library_draws_the_same_line():
    """Both launchers test the budget before anything touches a device: one past the limit the grouped entry, and the
    per-module entry asked for pair rows (no incidence to fall back on), answer GN_ERR_LDS.  Placeholder addresses, never
    dereferenced; neither entry is called at N <= the limit, where it would launch."""
    from groupnet_amd import _lib as L
    lib, P = L.load(), PLACEHOLDER
    N = R.N2E_BWD_SCENE_MAX_N + 1
    pairs = N * (N + 1) // 2
    group = dict(xp=P, pq=P, w2=P, b2=P, dedges=P, dxp=P, dpq=P, dw2=P, db2=P)
    arr = (L.N2EBwdGroup * 2)(L.N2EBwdGroup(H=None, E=pairs, sym=1, **group), L.N2EBwdGroup(H=P, E=3, sym=0, **group))
    assert lib.gn_node2edge_bwd_grouped_f32(arr, 2, 1, N, None) == L.GN_ERR_LDS
    assert lib.gn_node2edge_bwd_f32(P, P, None, P, P, P, P, P, P, P, 1, N, pairs, 1, None) == L.GN_ERR_LDS


def test_the_route_is_cached_frozen_and_pure(monkeypatch):
    R.backward_round_route.cache_clear()
    r = R.backward_round_route(11, (True, False))
    assert isinstance(r, R.BackwardRound) and R.backward_round_route(11, (True, False)) is r
    with pytest.raises(Exception):
        r.kept = False                                              # frozen
    # a leaf: route.py loads with no torch to import
    monkeypatch.setitem(sys.modules, "torch", None)
    spec = importlib.util.spec_from_file_location("route_alone", R.__file__)
    alone = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, "route_alone", alone)      # dataclasses looks the module up by name
    spec.loader.exec_module(alone)
    assert alone.backward_round_route(141, (True, False)) == alone.BackwardRound(False, False, False)
