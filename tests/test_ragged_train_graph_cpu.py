"""The host side of ragged training from a captured graph ("Ragged batches", Training from a captured
graph): the signatures of `GraphedTrainStep`, the scope that is the capture's opt-in, and the helper's own rules.  No
GPU, the library is never loaded."""
import inspect

import pytest
import torch

import agent_subset_cases as AS
import ragged_train_graph_cases as TG


def test_signatures():
    from groupnet_amd.graphs import GraphedMultiScale, GraphedTrainStep
    init = inspect.signature(GraphedTrainStep.__init__).parameters
    assert list(init)[-1] == "ragged" and init["ragged"].default is False
    assert list(init)[:9] == ["self", "block", "optimizer", "loss_fn", "B", "N", "target_shapes", "seed", "warmup"]
    call = inspect.signature(GraphedTrainStep.__call__).parameters
    assert list(call) == ["self", "f", "targets", "n_agents", "agent_mask"]
    assert call["targets"].kind is inspect.Parameter.VAR_POSITIONAL
    for name in ("n_agents", "agent_mask"):
        assert call[name].kind is inspect.Parameter.KEYWORD_ONLY and call[name].default is None
    assert callable(GraphedTrainStep.status)
    # the eval graph's face is what it was
    assert list(inspect.signature(GraphedMultiScale.__call__).parameters) == ["self", "f", "n_agents", "agent_mask"]
    assert list(inspect.signature(GraphedMultiScale.__init__).parameters)[-1] == "ragged"


def _answers(M):
    return M.ragged_training(), M.trains_empty_slots(), M.ragged_grad_refusals(True, 11), M.ragged_grad_refusals(True, 141)


@pytest.fixture
def switched_off():
    from groupnet_amd import MS_HGNN_batch as M
    prev = M._RAGGED_TRAINING
    M.set_ragged_training(False)
    yield M
    M._RAGGED_TRAINING = prev


def test_the_scope_is_the_opt_in(switched_off):
    M = switched_off
    outside = _answers(M)
    assert outside == (False, False, dict(grad=True, large=False), dict(grad=True, large=False))
    with M.ragged_train_graph_scope():
        assert M.ragged_training() and M.trains_empty_slots()
        assert not any(M.ragged_grad_refusals(True, 11).values())                   # refuses nothing
        assert M.ragged_grad_refusals(True, 141) == dict(grad=False, large=True)    # ... but the size
        assert not any(M.ragged_grad_refusals(False, 141).values())
        with pytest.raises(NotImplementedError):
            M.refuse_ragged(**M.ragged_grad_refusals(True, 141))
        with pytest.raises(NotImplementedError):
            M.refuse_ragged(listall=True)
        with pytest.raises(ValueError):
            M.refuse_ragged(handed_in=True)
    assert _answers(M) == outside
    with pytest.raises(NotImplementedError):
        M.refuse_ragged(**M.ragged_grad_refusals(True, 11))


def test_the_scope_closes_on_an_exception_and_nests(switched_off):
    M = switched_off
    outside = _answers(M)
    with pytest.raises(KeyError):
        with M.ragged_train_graph_scope():
            raise KeyError("inside")
    assert _answers(M) == outside
    with M.ragged_train_graph_scope():
        with M.ragged_train_graph_scope():
            assert M.trains_empty_slots()
        assert M.trains_empty_slots() and M.ragged_training()       # the inner exit leaves the outer scope open
        with pytest.raises(KeyError):
            with M.ragged_train_graph_scope():
                raise KeyError("inner")
        assert M.trains_empty_slots()
    assert _answers(M) == outside
    # with the switch on, the scope changes nothing about plain counts and still is what admits empty slots
    M.set_ragged_training(True)
    assert M.ragged_training() and not M.trains_empty_slots()
    with M.ragged_train_graph_scope():
        assert M.trains_empty_slots()
    assert not M.trains_empty_slots()


def test_the_environment_is_read_outside_the_scope_only(monkeypatch):
    from groupnet_amd import MS_HGNN_batch as M
    prev = M._RAGGED_TRAINING
    M.set_ragged_training(None)
    try:
        monkeypatch.setenv("GN_RAGGED_TRAINING", "0")
        assert not M.ragged_training()
        with M.ragged_train_graph_scope():
            assert M.ragged_training()
        assert not M.ragged_training()
    finally:
        M._RAGGED_TRAINING = prev


def test_host_validation_is_shared_and_comes_first():
    """`graphs._checked_counts`: what both graphed classes run before anything is copied or launched."""
    from groupnet_amd import graphs
    B, N = 3, 5
    holder = object()
    assert graphs._checked_counts(None, B, N, "cuda", None, None) is None
    assert graphs._checked_counts(holder, B, N, "cuda", [5, 0, 1], None) == [5, 0, 1]
    assert graphs._checked_counts(holder, B, N, "cuda", torch.tensor([1, 2, 3]), None) == [1, 2, 3]
    mask = torch.ones(B, N, dtype=torch.bool)
    for args in ((None, [1, 2, 3], None), (None, None, mask), (holder, [1, 2, 3], mask), (holder, [1, 2], None),
                 (holder, [1, 2, N + 1], None), (holder, [1, 2, -1], None), (holder, [1.0, 2, 3], None),
                 (holder, None, mask), (holder, None, mask.float())):
        with pytest.raises(ValueError):
            graphs._checked_counts(args[0], B, N, "cuda", args[1], args[2])
    with pytest.raises(ValueError):
        graphs._status(None)
    with pytest.raises(ValueError):
        graphs._counts_holder("x", B, N, "cuda", lambda: None)
    assert graphs._counts_holder(False, B, N, "cuda", lambda: 1 / 0) is None          # not ragged: nothing is asked


def test_shapes_and_replays_of_the_helper():
    for s in TG.SHAPES:
        assert s.replays[1] is None and s.replays[2] == (s.N,) * s.B
        assert all(len(c) == s.B and all(1 <= v <= s.N for v in c) for c in s.replays if c is not None)
        used = TG.counts_in_force(s.replays)
        assert used[1] == used[0] and len(set(used)) == 3
        assert all(sc <= s.N for sc in s.scales)
    assert TG.BY_ID["n7"].scales == (3, 7) and TG.BY_ID["n17"].N > 16 and TG.BY_ID["n6_nmp2"].nmp == 2
    assert len(TG.EMPTY_COUNTS) == TG.BY_ID["n7"].B and TG.EMPTY_COUNTS.count(0) == 2
    v = TG.prefix_valid(TG.EMPTY_COUNTS, 7)
    assert v.sum(dim=1).tolist() == list(TG.EMPTY_COUNTS) and bool(v[0].all()) and not bool(v[1].any())
    masks = TG.subset_masks(AS.BY_ID["n7"]["mask"])
    for m in masks:                                     # holes: not every scene is a prefix
        counts = m.sum(dim=1)
        assert any(not bool(m[b, :int(c)].all()) for b, c in enumerate(counts))


def test_losses_of_the_helper_ignore_invalid_rows():
    s = TG.BY_ID["n7"]
    f, t = TG.features(s, 128)
    final = torch.cat([f, torch.randn(s.B, s.N, 128)], dim=-1)
    valid = TG.prefix_valid(TG.EMPTY_COUNTS, s.N)
    spoiled = final.clone()
    spoiled[~valid] = float("nan")
    loss = TG.MaskedMSE()
    a, b = loss(final, None, t, valid), loss(spoiled, None, t, valid)
    assert torch.equal(a, b) and bool(torch.isfinite(a))
    assert torch.equal(loss.seen[0][valid], spoiled[valid]) and loss.seen[2] is valid
    assert float(TG.MaskedMSE()(spoiled, None, t, torch.zeros_like(valid))) == 0.0
    # the linear loss reads every position: on zeros at invalid positions it is the sum over the real agents, and its
    # gradient there is the target
    zeroed = final.clone()
    zeroed[~valid] = 0
    zeroed.requires_grad_(True)
    dot = TG.PaddedDot()
    v = dot(zeroed, None, t, valid)
    assert torch.allclose(v, (final[..., 64:] * t)[valid].sum(), rtol=1e-5)
    v.backward()
    assert torch.equal(zeroed.grad[..., 64:], t) and bool(zeroed.grad[~valid][..., 64:].any())
