"""CPU checks of tests/scene_isolation_cases.py: the case table reaches every route value and puts a checked scene
across a row-block edge of every group, the float64 oracle itself isolates scenes (the property the GPU tests rest
on), and the batch builders build what they say."""
import math

import pytest
import torch

import scene_isolation_cases as C
from launch_forms import block64, expected_forms, hyper_incidence
from oracle import ms_hgnn_oracle as O
from test_bf16_gpu import safe_rows
from test_launch_forms_gpu import MAX_NEAR_TIE


case_route = C.case_route      # the engine's knobs as the engine reads them


def all_batches(case):
    out = dict(C.batches(case["B"]))
    if case["dtype"] == "fp32" and case["precision"] == "f16x3":
        out.update(C.zero_neighbour_batches(case["B"]))
    return out


def test_every_case_takes_the_route_its_id_names_and_the_table_reaches_every_route_value():
    from groupnet_amd import route as R
    seen = dict(source=set(), closing=set(), pool=set(), launches=set(), masks=set())
    for case in C.CASES:
        rt, want = case_route(case), case["route"]
        kinds = "p" + "h" * len(case["scales"])
        for m, k in zip(rt.modules, kinds):
            got = (m.source, m.closing_input, m.pool_in_edge_kernel)
            assert got == want["pair" if k == "p" else "hyper"], (case["id"], k, got)
            seen["source"].add(m.source)
            seen["closing"].add(m.closing_input)
            seen["pool"].add(m.pool_in_edge_kernel)
        for name in ("node2edge", "gather", "scatter"):
            idx = tuple(i for i, k in enumerate(kinds) if k in want[name])
            assert getattr(rt, name) == idx, (case["id"], name, getattr(rt, name))
            if idx:
                seen["launches"].add(name)
        assert (rt.masks, rt.ask_closing) == (want["masks"], want["ask_closing"]), case["id"]
        seen["masks"].add(rt.masks)
    assert seen["source"] == {R.PAIR, R.PAIR_NODE, R.SCENE, R.TWIN_PAIR, R.FUSED_GATHER, R.EO}
    assert seen["closing"] == {R.NODE_AGG, R.SCATTER_SPEC, R.SCATTER}
    assert seen["pool"] == {True, False}
    assert seen["launches"] == {"node2edge", "gather", "scatter"}
    assert True in seen["masks"]


def row_counts(case):
    """(name, rows per scene) of everything the kernels cut into 32-row blocks: the node rows, every group's edge rows
    (the unordered pairs of the pairwise graph) and the ordered pairwise edges of the Gumbel stage."""
    B, N = case["B"], case["N"]
    groups = expected_forms(B, N, case["scales"], case["precision"], case["dtype"])["groups"]
    assert len(groups) == 1 + len(case["scales"])
    return [("node rows", N)] + [(g["name"], g["E"]) for g in groups] + [("ordered pairs", N * N)]


def case_batches(case):
    return all_batches(case) if case["route"] is not None else {"train": C.train_mags(case["B"])}


@pytest.mark.parametrize("case", C.CASES + C.TRAIN_CASES, ids=C.CASE_IDS + [c["id"] for c in C.TRAIN_CASES])
def test_a_checked_scene_straddles_a_row_block_of_every_group(case):
    """In every batch, for the node rows and every group whose rows fill more than one block, a CHECKED scene shares a
    32-row block with a neighbour at an inner block edge (scene_isolation_cases.across_an_inner_edge: scene 0 starting
    row 0 does not count)."""
    B, N = case["B"], case["N"]
    rows = row_counts(case)
    assert not C.straddle_gaps(case, case_batches(case), rows)
    assert any(B * r > 32 for _, r in rows)       # (n2: 18 node rows in one block; its 36 ordered pair rows fill two)
    assert B * N > 32 or case["id"] == "n2"       # more than one node row block everywhere but at 16 scenes per block
    assert (B * N) % 32 != 0                      # ... the last one ragged


def test_the_straddling_check_fails_when_the_poison_sits_on_the_straddling_scenes(monkeypatch):
    """N = 11, B = 7: only the scenes 2 and 5 cross a node row block; N = 17, B = 5: the scenes 1 and 3; N = 2, B = 9:
    only scene 8 starts the second block of ordered pair rows."""
    by_id = {c["id"]: c for c in C.CASES}
    assert C.across_an_inner_edge(7, 11) == [2, 5] and C.across_an_inner_edge(5, 17) == [1, 3]
    assert C.across_an_inner_edge(5, 16) == [1, 2, 3, 4] and C.across_an_inner_edge(9, 4) == [7, 8]
    assert C.across_an_inner_edge(9, 2) == [] and C.across_an_inner_edge(3, 50) == [0, 1, 2]
    for cid, moved, where in (("n11-f16x3", ((2, 5), (2, 5)), {("overflow", "node rows"), ("nonfinite", "node rows")}),
                              ("n17-dense", ((3,), (1, 3)), {("nonfinite", "node rows")}),
                              ("n2", ((7, 8), (7, 8)), {("overflow", "ordered pairs"), ("nonfinite", "ordered pairs")})):
        monkeypatch.setattr(C, "poison_positions", lambda B, moved=moved: moved)
        gaps = set(C.straddle_gaps(by_id[cid], case_batches(by_id[cid]), row_counts(by_id[cid])))
        assert where <= gaps, (cid, gaps)


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


_ISOLATES = set()      # cases that differ in the matrix path or the incidence form alone share their oracle


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_the_oracle_itself_isolates_scenes(case):
    """block64 on the whole poisoned batch, the non-finite and the overflowing scenes left in, against block64 scene by
    scene: every checked scene agrees to 1e-12 of its own scale (float64: a GEMM row's bits may depend on its position
    in the call, its value on nothing but the row)."""
    cid = case["id"]
    B, scales, nmp = case["B"], case["scales"], case["nmp"]
    key = (B, case["N"], tuple(scales), nmp, case["dtype"], case["seed"])
    if key in _ISOLATES:
        return
    _ISOLATES.add(key)
    _, sp, shs = C.cpu_block(case)
    h0, U = C.base_inputs(case)
    for name in ("nonfinite", "overflow"):
        mags = C.batches(B)[name]
        h = C.scaled(case, h0, mags)
        with torch.no_grad():
            out, facs = block64(sp, shs, scales, h, None, U[0], U[1:], torch.arange(B), nmp)
            if name == "nonfinite":        # (1e24 overflows fp32 hidden rows, not float64's)
                for b in (b for b in range(B) if not C.is_checked(mags[b])):
                    assert not bool(torch.isfinite(out[b, :, 64:]).all()), "the poison did not reach the oracle"
            for b in C.checked(mags):
                one, fone = block64(sp, shs, scales, h, None, U[0], U[1:], torch.tensor([b]), nmp)
                assert bool(torch.isfinite(one).all())
                for i in range(1 + len(scales)):
                    cols = slice(64 * (1 + i), 64 * (2 + i))
                    assert _rel(out[b:b + 1, :, cols], one[..., cols]) <= 1e-12, (cid, name, b, i)
                    assert float((facs[i][b:b + 1] - fone[i]).abs().max()) <= 1e-12, (cid, name, b, i)


def test_permutations_have_no_fixed_point():
    for case in C.CASES:
        p = C.derangement(case["B"], case["seed"])
        assert sorted(p.tolist()) == list(range(case["B"])) and not bool((p == torch.arange(case["B"])).any())
        assert torch.equal(C.derangement(case["B"], case["seed"]), p)      # seeded


def test_mixed_batches_hold_every_magnitude_class():
    """B >= 7: the one mixed batch holds every class.  Smaller B cannot (five classes, an ordinary scene among them,
    in three or five scenes beside a poisoned one or two): the case's mixed batches together do, and each holds an
    ordinary scene and one that is not."""
    for B in sorted({c["B"] for c in C.CASES}):
        bs = C.batches(B)
        mixed = [m for n, m in bs.items() if n.startswith("mixed")]
        assert len(mixed) == {3: 3, 5: 2, 7: 1, 9: 1}[B]
        seen = set()
        for mags in mixed:
            ks = {C.klass(m) for m in mags}
            assert "ordinary" in ks and len(ks) >= 2, (B, mags)
            assert B < 7 or ks == set(C.MIXED_CLASSES)
            assert all(m == 0.0 or m >= 1.0 for m in mags)       # no magnitude below 1
            seen |= ks
        assert seen == set(C.MIXED_CLASSES), (B, seen)
        assert {C.klass(m) for m in bs["overflow"]} >= {"overflow", "ordinary"}
        assert {C.klass(m) for m in bs["nonfinite"]} >= {"nan", "inf", "ordinary"}
        for name in ("overflow", "nonfinite"):
            assert len(C.checked(bs[name])) >= B - 2, (B, name)
        assert all(len(C.checked(m)) == B for n, m in bs.items() if n not in ("overflow", "nonfinite"))
        for mags in C.zero_neighbour_batches(B).values():
            assert {C.klass(m) for m in mags} == {"ordinary", "zero"}
    for case in C.TRAIN_CASES:
        mags = C.train_mags(case["B"])
        assert all(math.isfinite(m) for m in mags) and {C.klass(m) for m in mags} >= {"ordinary", "3e3"}


def test_scaled_builds_what_the_magnitudes_say():
    case = C.CASES[0]
    h0, U = C.base_inputs(case)
    mags = C.batches(case["B"])["nonfinite"]
    h = C.scaled(case, h0, mags)
    for b, m in enumerate(mags):
        if math.isnan(m):
            assert bool(torch.isnan(h[b]).all())
        elif math.isinf(m):
            assert int(torch.isinf(h[b]).sum()) == 2 and float(h[b].nan_to_num(posinf=0, neginf=0).abs().max()) > 0
            assert float(h[b].max()) == math.inf and float(h[b].min()) == -math.inf
        else:
            assert torch.equal(h[b], h0[b] * m)
    assert [len(u) for u in U] == [case["nmp"]] * (1 + len(case["scales"]))
    assert U[0][0].shape == (case["B"], case["N"] ** 2, C.K_PAIR) and U[-1][0].shape == (case["B"], 1, C.K_HYPER)
    twin = C.CASES[C.CASE_IDS.index("n50-bf16")]
    h16 = C.scaled(twin, C.base_inputs(twin)[0], C.batches(3)["mixed0"])
    assert torch.equal(h16, h16.bfloat16().float())


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_the_seeds_keep_the_incidence_free_of_near_ties(case):
    """The GPU tests compare a scene's incidence bit for bit with the oracle's fp32 ranking.  fp32 storage: no row of a
    checked scene may be a near-tie (all-zero scenes aside, whose one big tie has a defined winner); bf16 storage leaves
    near-tie rows out, and the oracle alone must stay inside the cap on their share."""
    h0, _ = C.base_inputs(case)
    for name, mags in all_batches(case).items():
        h = C.scaled(case, h0, mags)
        scenes = torch.tensor([b for b in C.checked(mags) if mags[b] != 0.0])
        corr = O.affinity(h[scenes])
        unsafe = total = 0
        for s in case["scales"]:
            ok = safe_rows(corr, s)
            unsafe, total = unsafe + int((~ok).sum()), total + ok.numel()
            if s != case["N"]:
                H = hyper_incidence(h, scenes, s)
                assert bool((H.sum(-1) == s).all()) and torch.equal(H, O.topk_incidence(corr, s))
        if case["dtype"] == "bf16":
            assert unsafe <= MAX_NEAR_TIE * total, (case["id"], name, unsafe, total)
        else:
            assert unsafe == 0, (case["id"], name, unsafe, total)


_CONDITION = {}      # (shape, rounds, seed) -> worst figure: cases that differ in the matrix path alone share their scenes


@pytest.mark.parametrize("case", [c for c in C.CASES if c["dtype"] == "fp32"],
                         ids=[c["id"] for c in C.CASES if c["dtype"] == "fp32"])
def test_the_seeds_keep_every_large_scene_well_conditioned(case):
    """scene_isolation_cases.LARGE_CONDITION: on every large checked scene the fp32 oracle alone is within half the GPU
    test's gate (2e-5 of the scene's and module's max|ref|) of the float64 oracle."""
    key = (case["B"], case["N"], tuple(case["scales"]), case["nmp"], case["seed"])
    if key not in _CONDITION:
        _, sp, shs = C.cpu_block(case)
        h0, U = C.base_inputs(case)
        worst, seen = 0.0, set()
        for mags in C.batches(case["B"]).values():
            h = C.scaled(case, h0, mags)
            for b in C.checked(mags):
                if C.is_ordinary(mags[b]) or (b, mags[b]) in seen:
                    continue
                seen.add((b, mags[b]))
                one = torch.tensor([b])
                Hs = [hyper_incidence(h, one, s) for s in case["scales"]]
                with torch.no_grad():
                    out64, _ = block64(sp, shs, case["scales"], h, Hs, U[0], U[1:], one, case["nmp"])
                    feats32, _ = C.oracle32(sp, shs, h, Hs, U, b, case["nmp"])
                for i, x in enumerate(feats32):
                    worst = max(worst, _rel(x.double(), out64[..., 64 * (1 + i):64 * (2 + i)]))
        assert len({m for _, m in seen}) == 3
        _CONDITION[key] = worst
    print(f"\n{case['id']}: fp32 oracle vs float64 oracle on the large scenes, worst {_CONDITION[key]:.1e} of max|ref|")
    assert _CONDITION[key] <= C.LARGE_CONDITION * C.TOL_LARGE


@pytest.mark.parametrize("case", C.TRAIN_CASES, ids=[c["id"] for c in C.TRAIN_CASES])
def test_the_training_seeds_leave_enough_clean_scenes(case):
    clean = C.train_clean_scenes(case)
    print(f"\n{case['id']}: clean ordinary scenes {clean.tolist()}")
    assert len(clean) >= case["min_clean"]


def test_the_tail_oracle_on_the_oracles_own_edge_features_is_the_oracle():
    """scene_isolation_cases.head_and_tail64 (the gate of a large scene on bf16 storage): fed the float64 oracle's own
    fac x dist — folded to unordered pairs as the kernels hold them, for the pairwise module — it returns the oracle's
    node features, and softmax(y / tau) is the oracle's distribution."""
    from launch_forms import state64
    case = C.CASES[C.CASE_IDS.index("n17-dense")]
    N, b = case["N"], 1          # the 1e6 scene of the first mixed batch
    _, sp, shs = C.cpu_block(case)
    h0, U = C.base_inputs(case)
    h = C.scaled(case, h0, C.batches(case["B"])["mixed0"])
    one = torch.tensor([b])
    Hs = [hyper_incidence(h, one, s) for s in case["scales"]]
    with torch.no_grad():
        out, facs = block64(sp, shs, case["scales"], h, Hs, U[0], U[1:], one)
        for i, st in enumerate([sp, *shs]):
            H = None if i == 0 else Hs[i - 1]
            Hd = O.pairwise_incidence(N, 1, torch.float64) if H is None else H.double()
            edges, _ = O.node2edge(state64(st), h[one].double(), Hd, 0, True)
            ef, dist = O.edge_mlp_gumbel(state64(st), "nmp_mlp_start", edges, U[i][0][one].double())
            if i == 0:
                ii, jj = torch.triu_indices(N, N)
                sym = ef[:, ii * N + jj] + ef[:, jj * N + ii]        # (the self-loop twice: its incidence weight folded in)
                ef = C.ordered_edge_feat(sym, N)
            y, nf = C.head_and_tail64(st, h, H, U[i], ef, b)
            assert _rel(nf, out[..., 64 * (1 + i):64 * (2 + i)]) <= 1e-12, i
            assert float((torch.softmax(y / O.GUMBEL_TAU, -1) - dist).abs().max()) <= 1e-12 and torch.equal(dist, facs[i])
            # the bf16 restatement of the head: close to y, not equal, and it leaves some edge determined
            y16 = C.head_y16(st, h, H, U[i], b)
            det, winner, e_emu = C.determined_edges(y, y16)
            assert 0 < e_emu <= 0.1 * float(y.abs().max()) and bool(det.any())
            assert bool((y.argmax(-1)[det] == y16.argmax(-1)[det]).all()) and torch.equal(winner[..., 0], y.argmax(-1))
