"""Ragged batches at launch sizes (tests/ragged_size_cases.py) without a device: the plan the library answers for every
launch tests/test_ragged_sizes_gpu.py makes, held against the case table and against the rules restated beside
tests/launch_forms.py's; the condition on the counts; the condition on the inputs; the count-class oracle against the
per-scene oracle of tests/ragged_cases.py; and the proof that the inputs can tell: taking a workgroup's first count on
the ORACLE's side moves a checked output by more than ten gates."""
import ctypes

import pytest
import torch

import ragged_cases as C
import ragged_size_cases as S
from launch_forms import CAPPED_GRID, state64
from oracle import ms_hgnn_oracle as O

P = 4096            # an aligned non-NULL "device address": a plan query tests addresses, it never reads through them


def lib():
    from groupnet_amd import _lib
    return _lib, _lib.load()


def test_case_table():
    assert [(c["id"], c["N"], c["B"], c["scales"], c["stage_scales"]) for c in S.CASES] == [
        ("n7-b2050", 7, 2050, [2, 5, 7], [1, 2, 3, 4, 5, 6, 7, 7]), ("n17-b1030", 17, 1030, [2, 5, 17], None),
        ("n50-b521", 50, 521, [2, 4, 8, 16], None), ("n17-b1930", 17, 1930, [2, 5, 17], None)]
    for c in S.CASES:
        n = c["counts"]
        assert len(n) == c["B"] and n[0] == c["N"] and n[-1] == 1 and all(1 <= v <= c["N"] for v in n)
        assert sorted(set(n)) == list(range(1, c["N"] + 1))              # every count occurs
    assert {(c, g, f) for c, g, f, _ in S.N2E_LAUNCHES} == set(S.N2E_REACHES)


# ---------------------------------------------------------------------------------------------------------------------
# plan queries
# ---------------------------------------------------------------------------------------------------------------------
def _n2e_query(stem, B, N, pair, Es, switch, monkeypatch):
    L, lb = lib()
    if switch is None:
        monkeypatch.delenv("GN_N2E_ROWS", raising=False)
    else:
        monkeypatch.setenv("GN_N2E_ROWS", switch)
    gs = []
    if pair is not None:
        gs.append(L.N2EGroup(xp=P, pq=P, w2=P, edges=P, b2=P, E=N * (N + 1) // 2 if pair == "sym" else N * N,
                             sym=int(pair == "sym")))
    gs += [L.N2EGroup(xp=P, pq=P, H=P, w2=P, edges=P, b2=P, E=E) for E in Es]
    plan = L.LaunchPlan()
    fn = getattr(lb, "gn_node2edge_ragged_plan_" + stem)
    assert fn((L.N2EGroup * len(gs))(*gs), len(gs), B, N, P, ctypes.byref(plan)) == L.GN_OK
    assert lb.gn_kernel_name(plan.kernel) == b"node2edge_ragged_kernel"
    return plan, len(gs)


def assert_n2e_plan(plan, n, want, where):
    """A gn_node2edge_ragged_plan_* plan says what `want` (ragged_size_cases.n2e_plan) says."""
    got = dict(variant=plan.variant, spw=list(plan.spw[:n]), wgs=list(plan.wgs[:n]), xcd=plan.xcd, grid=plan.grid[0])
    assert got == {k: want[k] for k in got}, (where, got, want)
    assert list(plan.grid[1:]) == [1, 1], where
    assert plan.SGh == want["SGh"] and plan.grid[0] - sum(plan.wgs[:n]) == want["padding"], where
    assert (plan.EBh == 0) == bool(plan.variant), where


N2E_RUNS = [(c, g, f, d) for c, g, f, ds in S.N2E_LAUNCHES for d in ds]


@pytest.mark.parametrize("case_id,groups,form,dtype", N2E_RUNS, ids=[f"{c}-{g or 'alone'}-{f}-{d}" for c, g, f, d in N2E_RUNS])
def test_node2edge_launches_reach_the_table(case_id, groups, form, dtype, monkeypatch):
    """Every node->edge launch of the GPU file: the library's plan is the restated rule's, and both say what the case
    table names — scenes per workgroup, the scenes left to the last workgroup, the form, the XCD remap."""
    case = S.BY_ID[case_id]
    B, N = case["B"], case["N"]
    SG, last, rows = S.N2E_REACHES[(case_id, groups, form)]
    want = S.launch_plan(case_id, groups, form)
    if groups is None:
        plan, n = _n2e_query("bf16" if dtype == "bf16" else "f32", B, N, "sym" if form == "pair-sym" else "ord", [], None,
                             monkeypatch)
    else:
        plan, n = _n2e_query("bf16" if dtype == "bf16" else "f32", B, N, None,
                             S.hyper_rows(N, S.groups_of(case, groups)["scales"]), S.SWITCH[form], monkeypatch)
    assert_n2e_plan(plan, n, want, (case_id, groups, form))
    assert list(plan.spw[:n]) == [SG] * n and plan.variant == rows and plan.xcd == 1
    if groups is not None:
        assert plan.SGh == SG
    if case_id == "n7-b2050":
        assert plan.grid[0] > sum(plan.wgs[:n])                                  # padding blocks of the remap (wg < 0)
    if last is not None:
        assert B % SG == last and last < SG                                      # a short last workgroup
    print(f"\n{case_id} {groups} {form} {dtype}: spw {SG}, last {B % SG or SG}, variant {plan.variant}, xcd {plan.xcd}, "
          f"grid {plan.grid[0]} for {sum(plan.wgs[:n])} workgroups, SGh {plan.SGh}, EBh {plan.EBh}, lds {plan.dyn_lds}")


@pytest.mark.parametrize("case_id", sorted({c for c, *_ in S.BLOCKS}))
@pytest.mark.parametrize("stem", ["f32", "bf16"])
def test_block_launch_packs_scenes_too(case_id, stem, monkeypatch):
    """The node->edge launch of the whole block (the pairwise group and the hyper groups in one): scenes per workgroup of
    both kinds as the rules say, more than one, remapped."""
    case = S.BY_ID[case_id]
    B, N = case["B"], case["N"]
    Es = S.hyper_rows(N, case["scales"])
    for pair in ("sym", "ord"):
        plan, n = _n2e_query(stem, B, N, pair, Es, None, monkeypatch)
        want = S.n2e_plan(B, N, pair, Es, None)
        assert_n2e_plan(plan, n, want, (case_id, pair))
        assert min(plan.spw[:n]) > 1 and plan.xcd == 1
        assert set(plan.spw[:n]) <= set(S.planned_scenes_per_wg(case_id))


@pytest.mark.parametrize("case_id", ["n7-b2050", "n17-b1030"])
def test_topk_launches_rank_a_whole_scene_per_band(case_id):
    """The banded top-k with RB = N (one band per scene: B >= 1024), which the small ragged cases never reach (RB = 8);
    the fused launch is one workgroup per scene at every size."""
    L, lb = lib()
    case = S.BY_ID[case_id]
    B, N = case["B"], case["N"]
    assert B >= 1024
    plan = L.LaunchPlan()
    for scales in {tuple(case["scales"]), tuple(case["stage_scales"] or case["scales"])}:
        n = len(scales)
        Hl, kl = (ctypes.c_void_p * n)(*[P] * n), (ctypes.c_int * n)(*scales)
        assert lb.gn_topk_incidence_ragged_plan_f32(P, Hl, kl, n, B, N, P, ctypes.byref(plan)) == L.GN_OK
        assert lb.gn_kernel_name(plan.kernel) == b"topk_incidence_ragged_kernel"
        assert plan.TE == N and list(plan.grid) == [1, B, 1] and plan.dyn_lds == 4 * N * N
        for stem in ("f32", "bf16"):
            fn = getattr(lb, "gn_affinity_topk_ragged_plan_" + stem)
            assert fn(P, P, Hl, kl, n, B, N, 64, None, P, ctypes.byref(plan)) == L.GN_OK
            assert lb.gn_kernel_name(plan.kernel) == b"affinity_topk_ragged_kernel" and list(plan.grid) == [B, 1, 1]
    # one scene fewer than 1024 and the band is halved: the shape the small cases run
    assert lb.gn_topk_incidence_ragged_plan_f32(P, Hl, kl, n, 1023, 17, P, ctypes.byref(plan)) == L.GN_OK
    assert plan.TE == 9


def test_scatter_launch_strides():
    """n17-b1930: B N 32 items exceed the 4096 x 256 of the capped grid, and the second pass holds VALID rows (a loop that
    does not stride leaves them unwritten)."""
    L, lb = lib()
    case = S.BY_ID["n17-b1930"]
    B, N = case["B"], case["N"]
    g = (L.ScatterGroup * 5)(L.ScatterGroup(feat=P, ori=P, out=P, E=N * (N + 1) // 2, sym=1),
                             L.ScatterGroup(feat=P, ori=P, out=P, E=N * N),
                             L.ScatterGroup(feat=P, H=P, ori=P, out=P, E=N), L.ScatterGroup(feat=P, H=P, ori=P, out=P, E=N),
                             L.ScatterGroup(feat=P, H=P, ori=P, out=P, E=1))
    plan = L.LaunchPlan()
    for stem in ("f32", "bf16"):
        for divisor in (0.0, 1.0):
            assert getattr(lb, "gn_agg_scatter_ragged_plan_" + stem)(g, 5, B, N, divisor, P, ctypes.byref(plan)) == L.GN_OK
            assert lb.gn_kernel_name(plan.kernel) == b"agg_scatter_ragged_kernel"
            assert list(plan.grid) == [CAPPED_GRID, 5, 1] and CAPPED_GRID == 4096
    first_pass = CAPPED_GRID * 256                  # items: (scene, node, 4 of 128 features)
    assert B * N * 32 > first_pass
    rows = torch.arange(first_pass // 32, B * N)     # the node rows of the later passes
    assert first_pass % 32 == 0 and int(S.valid_nodes(case).reshape(-1)[rows].sum()) >= 8


# ---------------------------------------------------------------------------------------------------------------------
# counts and inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_workgroups_mix_counts_in_both_directions():
    """For every planned number of scenes per workgroup, at least MIN_SIDE workgroups hold a later scene with a larger
    count than their first, and at least MIN_SIDE one with a smaller: the first count is wrong both ways."""
    assert S.planned_scenes_per_wg("n7-b2050") == [4, 6, 8, 15] and S.planned_scenes_per_wg("n17-b1030") == [2, 3]
    assert S.planned_scenes_per_wg("n50-b521") == [2]
    for case in S.CASES:
        for SG in S.planned_scenes_per_wg(case["id"]):
            up, down = S.mixed_workgroups(case["counts"], SG)
            print(f"{case['id']} SG {SG}: {up} workgroups with a larger later count, {down} with a smaller")
            assert up >= S.MIN_SIDE and down >= S.MIN_SIDE, (case["id"], SG, up, down)


def test_mixed_member_counts_share_a_wave():
    """n17-b1030 in the row form (3 scenes per workgroup, E = 17 / 17 / 1 rows per scene): the scale-N group's waves hold
    rows of more than 16 members beside rows of at most 16 — the general loop, with mixed counts inside a wave."""
    case = S.BY_ID["n17-b1030"]
    SG = S.N2E_REACHES[("n17-b1030", "block", "rows")][0]
    cnt = case["counts"]
    mixed = sum(1 for b0 in range(0, case["B"], SG)
                if max(cnt[b0:b0 + SG]) > 16 and min(cnt[b0:b0 + SG]) <= 5)
    assert mixed >= 16, mixed


@pytest.mark.parametrize("case", S.CASES, ids=[c["id"] for c in S.CASES])
def test_every_scene_keeps_its_selections_apart(case):
    """No valid row of any top-k scale has its k-th and (k+1)-th affinity closer than MIN_GAP, for the fp32 inputs and for
    their bf16 roundings: the cap on rows left out of an incidence comparison is zero."""
    print(f"{case['id']}: scenes redrawn after draw 0, 1, ...: {S.redraws(case['id'])} of {case['B']}")
    assert len(S.redraws(case["id"])) <= S.DRAWS and S.redraws(case["id"])[-1] == 0
    for bf16 in (False, True):
        h, _ = S.inputs(case["id"], bf16)
        gap = float(S.scene_gaps(case, h).min())
        print(f"{case['id']} {'bf16' if bf16 else 'fp32'}: smallest gap {gap:.2e}")
        assert gap >= C.MIN_GAP
        sample = dict(case, counts=case["counts"][:24], B=24)            # the per-scene statement of the same condition
        assert C.min_gap(sample, h[:24]) >= float(S.scene_gaps(case, h)[:24].min()) - 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def _assert_class_oracle_is_the_scene_oracle(case, h, U, scenes):
    _, sp, shs = C.cpu_block(case)
    N, seen = case["N"], 0
    for n, idx in S.classes(case, scenes):
        feats, facs, Hs = S.class_oracle(sp, shs, case, h, U, n, idx)
        for r, b in enumerate(idx.tolist()):
            f1, c1, H1 = C.scene_oracle(sp, shs, case, h, U, b)
            for i in range(1 + len(case["scales"])):
                assert float((feats[i][r] - f1[i]).abs().max()) <= 1e-12, (b, i)
                assert float((facs[i][r] - c1[i]).abs().max()) <= 1e-12, (b, i)
            assert all(torch.equal(Hs[i][r:r + 1], H1[i]) for i in range(len(Hs))), b
            seen += 1
    return seen


def test_class_oracle_is_the_scene_oracle():
    """The count-class oracle equals `ragged_cases.scene_oracle` scene by scene: on case n7 of tests/ragged_cases.py and
    on 24 seeded scenes of n7-b2050 (features and factors to 1e-12, incidences equal); and the embedded forms hold those
    values at the rows a scene owns and zeros elsewhere."""
    small = C.BY_ID["n7"]
    h, U = C.inputs(small)
    assert _assert_class_oracle_is_the_scene_oracle(small, h, U, None) == small["B"]
    case = S.BY_ID["n7-b2050"]
    h, U = S.inputs(case["id"])
    gen = torch.Generator().manual_seed(24)
    scenes = sorted({0, case["B"] - 1} | set(torch.randperm(case["B"], generator=gen)[:22].tolist()))
    assert _assert_class_oracle_is_the_scene_oracle(case, h, U, scenes) == 24
    feats, facs, scale = S.block_oracle(case["id"])
    _, sp, shs = C.cpu_block(case)
    for b in scenes:
        n = case["counts"][b]
        f1, c1, H1 = C.scene_oracle(sp, shs, case, h, U, b)
        assert float((feats[b, :n] - torch.cat(f1, dim=-1)).abs().max()) <= 1e-12 and not feats[b, n:].any()
        assert float((facs[0][b, C.pair_index(7, n)] - c1[0]).abs().max()) <= 1e-12
        assert int((facs[0][b] != 0).any(-1).sum()) == n * n
        for i, s in enumerate(case["scales"]):
            assert float((facs[1 + i][b, :c1[1 + i].shape[0]] - c1[1 + i]).abs().max()) <= 1e-12
            assert torch.equal(S.padded_incidence(case, h, s)[b], C.padded_incidence(dict(case, counts=[n], B=1), h[b:b + 1], s)[0])
    assert torch.equal(S.padded_corr(case, h)[scenes], torch.stack(
        [C.padded_corr(dict(case, counts=[case["counts"][b]], B=1), h[b:b + 1])[0] for b in scenes]))


def test_embedded_node2edge_oracle_is_the_scene_oracle():
    """The node->edge references of the GPU file (hyper groups, ordered and symmetric pairs) against `ragged_cases.
    node2edge64` of single scenes, and their masks of owned rows."""
    case = S.BY_ID["n7-b2050"]
    N = case["N"]
    h, _ = S.inputs(case["id"])
    _, sp, shs = C.cpu_block(case)
    hyper = S.hyper_n2e_oracle(case, h, shs)
    ordered, sym = S.pair_n2e_oracle(case, h, sp, False), S.pair_n2e_oracle(case, h, sp, True)
    for kind, ref in (("ord", ordered), ("sym", sym), *zip(case["scales"], hyper)):
        assert torch.equal((ref != 0).any(-1), S.valid_rows(case, kind)), kind
    for b in (0, 1, 2, 3, 1027, case["B"] - 2, case["B"] - 1):
        n = case["counts"][b]
        corr = C.scene_corr(h, b, n)
        for ref, st, s in zip(hyper, shs, case["scales"]):
            one = C.node2edge64(st, h[b:b + 1, :n], C.scene_incidence(corr, s, N))
            assert float((ref[b, :one.shape[0]] - one).abs().max()) <= 1e-12
        one = C.node2edge64(sp, h[b:b + 1, :n], O.pairwise_incidence(n, 1))
        assert float((ordered[b, C.pair_index(N, n)] - one).abs().max()) <= 1e-12
        rows, src = S.sym_rows(N, n)
        assert float((sym[b, rows] - one[src]).abs().max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# seeded flaws: the inputs can tell
# ---------------------------------------------------------------------------------------------------------------------
def _flaw_moves(case, h, states, incidences, SG, bigger, n_scenes=12):
    """The largest change of a node->edge row over up to `n_scenes` scenes whose workgroup's first count is larger
    (`bigger`) / smaller than their own, when the softmax takes that first count.  states / incidences: per group the
    module's state and a function (corr (m, n, n), n) -> H."""
    first = S.first_counts(case["counts"], SG)
    scenes = [b for b, (own, f) in enumerate(zip(case["counts"], first)) if (f > own if bigger else f < own)][:n_scenes]
    assert len(scenes) == n_scenes
    worst = 0.0
    for n, idx in S.classes(case, scenes):
        x, corr = h[idx, :n].double(), S.class_corr(h, idx, n)
        nv = torch.tensor([first[b] for b in idx.tolist()])
        for st, make in zip(states, incidences):
            H = make(corr, n).double()
            right = S.node2edge_counted(state64(st), x, H, torch.full_like(nv, n))
            assert float((right - O.node2edge(state64(st), x, H, 0, True)[0]).abs().max()) <= 1e-12
            worst = max(worst, float((right - S.node2edge_counted(state64(st), x, H, nv)).abs().max()))
    return worst


@pytest.mark.parametrize("case_id,groups,form", sorted(S.N2E_REACHES, key=str), ids=lambda v: str(v))
def test_first_count_of_the_workgroup_is_a_visible_flaw(case_id, groups, form):
    """Each body's flaw — `n_valid[b0]` for `n_valid[b0 + s]` — applied to the oracle's side at the launch's own scenes per
    workgroup: some checked row moves by more than ten gates, in both directions."""
    case = S.groups_of(S.BY_ID[case_id], groups) if groups else S.BY_ID[case_id]
    h, _ = S.inputs(case_id)
    _, sp, shs = C.cpu_block(case)
    SG = S.N2E_REACHES[(case_id, groups, form)][0]
    if groups is None:
        states, inc = [sp], [lambda corr, n: O.pairwise_incidence(n, corr.shape[0])]
    else:
        states = shs
        inc = [lambda corr, n, s=s: S.class_incidence(corr, s, case["N"]) for s in case["scales"]]
    for bigger in (True, False):
        moved = _flaw_moves(case, h, states, inc, SG, bigger)
        print(f"{case_id} {groups} {form} SG {SG}, first count {'larger' if bigger else 'smaller'}: moves {moved:.2e}")
        assert moved > 10 * C.TOL
