"""The tables of tests/graph_lifetime_cases.py, checked without a GPU: the family table names every parameter of a block
and of an encoder exactly once, and every single-family change moves the float64 oracle's output by at least 100 x TOL —
so that "the replay differs from the pre-change output" and "the replay equals the eager forward" in
tests/test_graph_lifetime_gpu.py cannot both hold for a refresh that missed the family's images."""
import pytest
import torch

import graph_lifetime_cases as L


def _names(model):
    return [n for n, _ in model.named_parameters()]


@pytest.mark.parametrize("cfg_id", ["f16x3-latency", "nmp2", "mask-standalone", "encoder"])
def test_family_table_names_every_parameter_exactly_once(cfg_id):
    cfg = L.CONFIG_BY_ID[cfg_id]
    names = _names(L.make_model(cfg))
    assert len(names) == len(set(names)) > 100
    for n in names:
        assert len(L.families_of(n)) == 1, (n, [f.id for f in L.families_of(n)])
    # every family of the table exists in some configuration, and the one-type families touch one type's layer only
    used = {L.families_of(n)[0].id for n in names}
    want = {f.id for f in L.FAMILIES if (not f.nmp2 or cfg.nmp > 1) and (not f.top or cfg.kind == "encoder")}
    assert used == want
    for tag, fam, members in L.family_changes(cfg, names):
        if fam.one_type is not None:
            assert len(members) == 2 * cfg.nmp and all(f".agg_mlp.{L.AGG_TYPE}." in m for m in members), tag
    # the changes of item 5 cover every live family the configuration has, for the pairwise and for one hyper module
    tags = {t for t, _, _ in L.family_changes(cfg, names)}
    for f in L.FAMILIES:
        if f.id in want and not f.dead:
            assert all(f"{m or 'front'}:{f.id}" in tags for m in ([None] if f.top else L.modules_under_test(cfg))), f.id


def test_configurations_and_training_cases_as_the_issue_lists_them():
    got = [(c.id, c.B, c.N, c.scales, c.nmp) for c in L.CONFIGS]
    assert got == [("f16x3-latency", 5, 11, (2, 5, 11), 1), ("f16x3-throughput", 5, 11, (2, 5, 11), 1),
                   ("bf16x6", 5, 11, (2, 5, 11), 1), ("fp32", 5, 11, (2, 5, 11), 1), ("bf16-storage", 5, 11, (2, 5, 11), 1),
                   ("mask-standalone", 3, 17, (4, 17), 1), ("nmp2", 3, 7, (3, 7), 2), ("ragged", 5, 11, (2, 5, 11), 1),
                   ("encoder", 3, 11, (5, 11), 1)]
    assert L.CONFIG_BY_ID["f16x3-latency"].tail is True and L.CONFIG_BY_ID["f16x3-throughput"].tail is False
    ragged = L.CONFIG_BY_ID["ragged"]
    assert len(ragged.counts) == ragged.B and len(set(ragged.counts)) > 2 and max(ragged.counts) == ragged.N
    assert [(c.opt, c.B, c.N, c.scales, c.nmp) for c in L.TRAIN_CASES] == [
        ("sgd", 6, 11, (2, 5, 11), 1), ("adam", 4, 7, (3, 7), 2), ("sgd0", 3, 17, (4, 17), 1)]
    assert L.TRAIN_K == 4 and L.SPREAD_MARGIN == 8 and L.STALE_POWER == 10 and L.ORACLE_MARGIN == 4
    assert [(c.B, c.N, c.scales) for c in L.SIDE_CASES] == [(512, 11, (2, 5, 11)), (64, 50, (2, 4, 8, 16))]
    for c in L.SIDE_CASES:
        vs = [L.side_counts(c, i) for i in range(L.SIDE_GRAPHS)]
        assert all(1 <= min(v) and max(v) <= c.N and len(set(v)) > 2 for v in vs) and len({tuple(v) for v in vs}) == 4


def test_philox_noise_is_one_contiguous_module_major_span():
    cfg = L.CONFIG_BY_ID["nmp2"]
    shapes = L.noise_shapes(cfg, 6, 10)
    noise, draws = L.philox_noise(shapes, cfg.nmp, L.SEED, 40)
    assert draws == sum(b * e * k for b, e, k in shapes) * cfg.nmp
    flat = torch.cat([u.reshape(-1) for us in noise for u in us])
    assert torch.equal(flat, torch.from_numpy(L.O.philox_uniform(draws, L.SEED, 40)))


@pytest.mark.parametrize("cfg_id", ["f16x3-latency", "mask-standalone", "nmp2", "encoder"])
def test_every_single_family_change_is_visible(cfg_id):
    """One configuration per distinct (model, shape) of part A — the other block configurations share the first one's
    model, inputs and noise.  Every live family's change moves the float64 oracle by >= 100 x TOL = 1e-3; a change of the
    parameters nothing reads moves it by exactly nothing."""
    cfg = L.CONFIG_BY_ID[cfg_id]
    model = L.make_model(cfg)
    x = L.make_inputs(cfg)
    noise, _ = L.philox_noise(L.noise_shapes(cfg, *L.edge_types(model, cfg.kind)), cfg.nmp, L.SEED, 0)
    params = dict(model.named_parameters())
    with torch.no_grad():
        base = L.oracle64(cfg, model.state_dict(), x, noise)
        for dead in (False, True):
            for tag, fam, members in L.family_changes(cfg, list(params), dead=dead):
                with L.scaled(params, members, fam.factor):
                    moved = float((L.oracle64(cfg, model.state_dict(), x, noise) - base).abs().max())
                print(f"{cfg.id} {tag}: x{fam.factor} moves the oracle by {moved:.3e}")
                assert (moved == 0.0) if dead else (moved >= L.VISIBLE), (tag, moved)
