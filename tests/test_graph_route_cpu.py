"""`groupnet_amd.route.graph_stage_route` — the graph stage `multiscale.build_graphs` follows — over its whole input grid
against the rules as the three call sites stated them before the route existed (no GPU, no library load).  Each rule
below is one expression of such a site, written out again here; a predicate edited in the route fails in this file."""
import importlib.util
import itertools
import sys

import pytest

from groupnet_amd import route as R

FORMS = ("tail", "fused", "banded")              # what ops.graph_form answers
SCALES = (0, 1, 2, 3, 8)
ROWS = (33, 32767, 32768, 51200)                 # B*N around the fork threshold
BOOLS = (False, True)


def grid(*axes):
    return itertools.product(*axes)


def fields(r):
    return dict(kind=r.kind, masks=r.masks, fork=r.fork, deferred=r.deferred, own_copy=r.own_copy,
                ask_closing=r.ask_closing, H_cat=r.H_cat)


def test_the_block_forward():
    """`MultiScaleHGNN.forward`, inference."""
    n = 0
    for S, form, rows, masked, ragged, grouped, affinity_tail, capturing in grid(SCALES, FORMS, ROWS, BOOLS, BOOLS, BOOLS,
                                                                                BOOLS, BOOLS):
        facts = R.StageFacts(grouped=grouped, latency_form=affinity_tail, capturing=capturing, embed=False, may_defer=True)
        got = R.graph_stage_route(S, form, rows, masked=masked, ragged=ragged, training=False, facts=facts)
        want_masks = masked and not ragged                      # masks_apply(N) and counts is None
        fused = bool(S) and form != "banded"
        if fused:
            fork = grouped and rows >= 32768 and capturing      # ... and f.is_cuda and the stream is capturing
            deferred = grouped and not fork and affinity_tail and not want_masks
            want = dict(kind=R.FUSED, masks=want_masks, fork=fork, deferred=deferred, own_copy=False, H_cat=True)
        elif S:
            want = dict(kind=R.BANDED, masks=False, fork=False, deferred=False, own_copy=True, H_cat=True)
        else:
            want = dict(kind=R.NONE, masks=False, fork=False, deferred=False, own_copy=True, H_cat=False)
        want["ask_closing"] = grouped and affinity_tail         # fuse_closing=self.affinity_tail, grouped forwards only
        assert fields(got) == want, (S, form, rows, masked, ragged, facts)
        n += 1
    assert n == len(SCALES) * 3 * len(ROWS) * 32


def test_the_training_forward():
    """`multiscale_autograd`: the job is launched at once, nothing is written into a final, the caller bumps the counter."""
    for S, form, rows, masked, grouped, latency, capturing, may_defer in grid(SCALES, FORMS, ROWS, BOOLS, BOOLS, BOOLS,
                                                                             BOOLS, BOOLS):
        facts = R.StageFacts(grouped=grouped, latency_form=latency, capturing=capturing, embed=False, may_defer=may_defer)
        got = R.graph_stage_route(S, form, rows, masked=masked, ragged=False, training=True, facts=facts)
        want_masks = masked                                     # masks_apply(N)
        if S and form != "banded":
            want = dict(kind=R.FUSED, masks=want_masks, H_cat=True)
        elif S:
            want = dict(kind=R.BANDED, masks=False, H_cat=True)
        else:
            want = dict(kind=R.NONE, masks=False, H_cat=False)
        want.update(fork=False, deferred=False, own_copy=False, ask_closing=False)
        assert fields(got) == want, (S, form, rows, masked, facts)
        with pytest.raises(NotImplementedError):
            R.graph_stage_route(S, form, rows, masked=masked, ragged=True, training=True, facts=facts)


def test_the_encoders():
    """`_TrajectoryEncoder._encode`, eval: launched at once, never the tail, never the closing stage."""
    for S, form, rows, masked, grouped, latency, capturing in grid((0, 1, 2, 3), FORMS, ROWS, BOOLS, BOOLS, BOOLS, BOOLS):
        facts = R.StageFacts(grouped=grouped, latency_form=latency, capturing=capturing, embed=True, may_defer=False)
        got = R.graph_stage_route(S, form, rows, masked=masked, ragged=False, training=False, facts=facts)
        if form == "banded":                                    # not self.fused_front_end_fits(N, T)
            # copy + counter_add, then `topk_incidence(affinity(f)) if S else []`
            want = dict(kind=R.BANDED if S else R.NONE, masks=False, own_copy=True)
        else:
            want_masks = S > 0 and masked                       # S > 0 and masks_apply(N)
            want = dict(kind=R.FUSED, masks=want_masks, own_copy=False)         # `scales or [N]`
        want.update(fork=False, deferred=False, ask_closing=False, H_cat=S > 1)  # want_H_cat = S > 1
        assert fields(got) == want, (S, form, rows, masked, facts)


def test_the_ragged_rules():
    """A ragged forward never asks for masks; its job is still handed on where the block defers."""
    facts = R.StageFacts(grouped=True, latency_form=True, capturing=False, embed=False, may_defer=True)
    for masked in BOOLS:
        r = R.graph_stage_route(3, "fused", 33, masked=masked, ragged=True, training=False, facts=facts)
        assert (r.kind, r.masks, r.deferred, r.ask_closing) == (R.FUSED, False, True, True)
        assert not R.graph_stage_masks(3, masked, True)
    assert R.graph_stage_masks(3, True, False) and not R.graph_stage_masks(0, True, False)


def test_the_route_is_cached_frozen_and_pure(monkeypatch):
    import os
    facts = R.StageFacts(grouped=True, latency_form=True, capturing=False, embed=False, may_defer=True)
    ask = lambda: R.graph_stage_route(3, "tail", 33, masked=False, ragged=False, training=False,
                                      facts=R.StageFacts(*facts))

    def refuse(*a, **k):
        raise AssertionError("the route reached outside its arguments")

    monkeypatch.setattr(os.environ, "get", refuse)
    monkeypatch.setattr(os, "getenv", refuse)
    R.graph_stage_route.cache_clear()
    r = ask()
    assert isinstance(r, R.GraphStage) and ask() is r           # equal arguments: the same object
    with pytest.raises(Exception):
        r.fork = True                                           # frozen
    # a leaf: route.py loads with no torch to import
    monkeypatch.setitem(sys.modules, "torch", None)
    spec = importlib.util.spec_from_file_location("route_alone", R.__file__)
    alone = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, "route_alone", alone)      # dataclasses looks the module up by name
    spec.loader.exec_module(alone)
    with pytest.raises(ImportError):
        import torch  # noqa: F401
    assert fields(alone.graph_stage_route(3, "tail", 33, masked=False, ragged=False, training=False,
                                          facts=alone.StageFacts(*facts))) == fields(r)
