"""`groupnet_amd.route.message_passing_route` — the route `run_message_passing` follows — against tests/launch_forms.py,
the tests' own statement of the rules (no GPU, no library load): what `expected_forms` and `launch_descriptors` say a
forward passes to its launches is what the route tells the engine to pass.  A predicate edited in the route fails here;
tests/test_launch_plan_cpu.py holds the same statement against the launchers' plans."""
import itertools

import pytest

from groupnet_amd import route as R
from launch_forms import K_HYPER, K_PAIR, expected_forms, launch_descriptors

SWEEP_N = (3, 11, 16, 17, 50, 64, 65)
MODES = (("f16x3", "fp32"), ("bf16x6", "fp32"), ("fp32", "fp32"), ("f16x3", "bf16"))
B = 3                                   # B does not enter the route
DEFAULT = R.Knobs(fuse_pool=True, pool_max_n=16, node_form=True, masked=False)
PAIR, HYPER = (True, K_PAIR), (False, K_HYPER)


def ask(N, modules, precision="f16x3", dtype="fp32", training=False, knobs=DEFAULT, closing_asked=True):
    return R.message_passing_route(N, tuple(modules), twin=dtype == "bf16", training=training,
                                   matrix16=precision != "fp32", knobs=knobs, closing_asked=closing_asked)


def stated(N, scales, precision, dtype, training, block):
    """What launch_forms states about a forward, in the route's terms: per module (pooled in the edge kernel, first
    layer per node, source, closing input), the modules of the node2edge / gather / scatter launches, closing asked."""
    kw = dict(B=B, N=N, scales=scales, precision=precision, dtype=dtype, training=training, block=block, with_pair=block)
    forms, d = expected_forms(**kw), launch_descriptors(**kw)
    mods = []
    for g, e, a, m in zip(forms["groups"], d["edge"], d["agg"], d["mlp2"][0]):
        assert bool(a.node_form) == g["node_form"]
        if a.A:
            source = R.PAIR_NODE if a.node_form else R.PAIR
        elif a.eo:
            source = R.EO
        elif a.sym:
            source = R.SCENE if a.node_form else R.TWIN_PAIR
        else:
            assert a.ori and a.H
            source = R.FUSED_GATHER
        closing = R.SCATTER if m.x else (R.SCATTER_SPEC if m.E else R.NODE_AGG)
        assert m.x or (m.feat and m.ori)
        mods.append((bool(e.pool_N), bool(a.A), source, closing))
    launches = dict(node2edge=tuple(i for i, e in enumerate(d["edge"]) if not e.pool_N),
                    gather=tuple(i for i, a in enumerate(d["agg"]) if a.eo),
                    scatter=tuple(i for i, m in enumerate(d["mlp2"][0]) if m.x))
    for k, arr in (("node2edge", d["n2e"]), ("gather", d["gather"]), ("scatter", d["scatter"])):
        assert len(launches[k]) == (0 if arr is None else len(arr))      # the launch's own descriptor array
    assert bool(launches["node2edge"] and any(x.H for x in d["n2e"])) == (forms["n2e"] is not None)
    assert bool(launches["gather"]) == (forms["gather_spw"] is not None)
    assert bool(launches["scatter"]) == (forms["scatter"] is not None)
    # The closing stage: the route asks wherever the launchers' rules can take it, and the launcher's plan has the last
    # word.  At B = 3 no launch-size rule refuses, so on the 16-bit cores "asked" is "fused"; on the fp32 cores the route
    # asks at the same sizes and `ops.agg_mlp_closing` declines (the route does not look at the precision for this).
    as16 = expected_forms(**{**kw, "precision": "f16x3"})["fused_closing"] if precision == "fp32" else forms["fused_closing"]
    assert not forms["fused_closing"] or as16
    return mods, launches, as16


def check(N, scales, precision, dtype, training, block):
    where = (N, scales, precision, dtype, training, block)
    mods, launches, asked = stated(N, scales, precision, dtype, training, block)
    rt = ask(N, ([PAIR] if block else []) + [HYPER] * len(scales), precision, dtype, training, closing_asked=block)
    got = [(m.pool_in_edge_kernel, m.first_layer, m.source, m.closing_input) for m in rt.modules]
    assert got == mods, (where, got, mods)
    assert [m.node_form for m in rt.modules] == [s in (R.PAIR_NODE, R.SCENE) for _, _, s, _ in mods], where
    assert dict(node2edge=rt.node2edge, gather=rt.gather, scatter=rt.scatter) == launches, (where, rt)
    assert rt.ask_closing == asked and not rt.masks, (where, rt)


@pytest.mark.parametrize("precision,dtype", MODES, ids=[p if d == "fp32" else d for p, d in MODES])
def test_route_over_the_size_sweep(precision, dtype):
    n = 0
    for N, training in itertools.product(SWEEP_N, (False, True)):
        if training and dtype == "bf16":
            continue            # the twins are forward-only
        check(N, [2, min(5, N), N], precision, dtype, training, block=True)
        for s in (2, min(5, N), N):
            check(N, [s], precision, dtype, training, block=False)      # one MS_HGNN_hyper through the module API
        n += 1
    assert n == len(SWEEP_N) * (1 if dtype == "bf16" else 2)


def test_the_twins_do_not_train():
    with pytest.raises(NotImplementedError):
        ask(11, [PAIR], dtype="bf16", training=True)


def test_closing_is_asked_only_when_the_caller_asks():
    assert ask(11, [PAIR, HYPER]).ask_closing and not ask(11, [PAIR, HYPER], closing_asked=False).ask_closing


def test_node_form_switch():
    off = DEFAULT._replace(node_form=False)
    for N in (3, 16):
        assert ask(N, [PAIR]).modules[0].source == R.PAIR_NODE
        m = ask(N, [PAIR], knobs=off).modules[0]
        assert (m.source, m.first_layer, m.closing_input) == (R.PAIR, True, R.SCATTER_SPEC)
    for N in (3, 64):
        assert ask(N, [PAIR], dtype="bf16").modules[0].source == R.SCENE
        m = ask(N, [PAIR], dtype="bf16", knobs=off).modules[0]
        assert (m.source, m.first_layer) == (R.TWIN_PAIR, False)
        assert m.closing_input == (R.SCATTER_SPEC if N <= 16 else R.SCATTER)
    assert ask(64, [PAIR], dtype="bf16", knobs=off).scatter == (0,)


def test_pooling_switches():
    mods = [PAIR, HYPER, HYPER]
    assert ask(11, mods).node2edge == ()
    for dtype in ("fp32", "bf16"):
        off = ask(11, mods, dtype=dtype, knobs=DEFAULT._replace(fuse_pool=False))
        assert off.node2edge == (0, 1, 2) and not any(m.pool_in_edge_kernel for m in off.modules)
        zero = ask(11, mods, dtype=dtype, knobs=DEFAULT._replace(pool_max_n=0))
        assert zero.node2edge == (1, 2)
        assert [m.pool_in_edge_kernel for m in zero.modules] == [True, False, False]
    # nothing else moves with them
    strip = lambda rt: [(m.first_layer, m.source, m.closing_input) for m in rt.modules]
    assert strip(ask(11, mods)) == strip(ask(11, mods, knobs=DEFAULT._replace(fuse_pool=False, pool_max_n=0)))


def test_many_edge_types_keep_the_pair_form():
    assert ask(11, [(True, 12)]).modules[0].source == R.PAIR_NODE
    m = ask(11, [(True, 13)]).modules[0]
    assert (m.source, m.first_layer, m.closing_input) == (R.PAIR, True, R.SCATTER_SPEC)


def test_masks_are_read_in_their_range_when_every_hyper_module_has_them():
    mods = [PAIR, HYPER, HYPER]
    # `masked`: the mask form is on AND every hyper module came with its masks (the engine fills it at call time)
    on = DEFAULT._replace(masked=True)
    for training in (False, True):
        for N in (17, 64):
            assert ask(N, mods, training=training, knobs=on).masks
            assert not ask(N, mods, training=training).masks
        for N in (16, 65):
            assert not ask(N, mods, training=training, knobs=on).masks
    assert [R.masks_in_range(N) for N in (1, 16, 17, 64, 65)] == [False, False, True, True, False]
    # the masks change who reads the incidence, not which launches run
    for N in (17, 64):
        a, b = ask(N, mods, knobs=on), ask(N, mods)
        assert (a.modules, a.node2edge, a.gather, a.scatter) == (b.modules, b.node2edge, b.gather, b.scatter)


def test_the_route_is_pure(monkeypatch):
    """No library, no environment, no torch.cuda: everything the route needs is an argument."""
    import os

    import torch

    from groupnet_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("the route reached outside its arguments")

    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(os.environ, "get", refuse)
    monkeypatch.setattr(os, "getenv", refuse)
    monkeypatch.setattr(torch.cuda, "is_available", refuse)
    monkeypatch.setattr(torch.cuda, "current_device", refuse)
    R.message_passing_route.cache_clear()
    rt = ask(17, [PAIR, HYPER, HYPER])
    assert isinstance(rt, R.Route) and rt.gather == (1, 2) and rt.scatter == (0, 1, 2)
    assert ask(17, [PAIR, HYPER, HYPER]) is rt          # memoised
    with pytest.raises(Exception):
        rt.masks = True                                  # frozen
