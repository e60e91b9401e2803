"""Test helper: ragged batches (`n_agents=`) at the batch sizes where the launchers pack several scenes into a workgroup
(tests/test_ragged_sizes_cpu.py checks the cases, the inputs and the oracle; tests/test_ragged_sizes_gpu.py runs them).
Pure torch on the CPU; the library is never loaded.

Why.  A ragged plan is its plain twin except `kernel`, and the plain plans choose their work shape by launch size: scenes
per workgroup of the node->edge bodies, the XCD remap, the band height of the top-k, the stride of the scatter.  The
cases of tests/ragged_cases.py run at B = 2 ... 6, where every workgroup holds ONE scene: the three places where a
body reads `n_valid[b0 + s]` only ever saw s == 0 there.  The cases below are the smallest batches that reach the other
shapes (`n2e_plan` and its rules restate the launchers' arithmetic; the CPU test holds them against the library's plan
queries), with counts drawn so that a workgroup's first count is wrong for its later scenes in both directions.

The oracle.  A scene's valid block is what the module computes for that scene ALONE at its own size (INTEGRATION.md,
"Ragged batches"), so all scenes of one count n form an ordinary batch of n-agent scenes: the existing float64 oracle runs
ONCE PER DISTINCT COUNT on h[idx_n, :n] — every scene of the batch is covered, not a sample — with the noise gathered at
the padded indices and the incidence ranked on the fp32 affinity exactly as `ragged_cases.scene_oracle` does per scene
(the CPU test holds the two against each other).

The inputs.  N(0,1) features; each scene's are the first of at most DRAWS seeded draws for which every valid row keeps
MIN_GAP between its k-th and (k+1)-th affinity at every top-k scale of the case, for the fp32 values and for their bf16
roundings: no row of any incidence comparison is left out.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import torch

import ragged_cases as C
from launch_forms import CAPPED_GRID, cdiv, pair_count, state64, xcd_grid
from oracle import ms_hgnn_oracle as O

DRAWS = 16          # seeded draws a scene may take to keep its selections MIN_GAP apart
MIN_SIDE = 32       # workgroups that must hold a later scene with a larger count than their first, and with a smaller


def _counts(N: int, B: int, seed: int) -> List[int]:
    """A seeded draw from 1..N; scene 0 has N agents, the last scene one."""
    gen = torch.Generator().manual_seed(4000 + seed)
    c = torch.randint(1, N + 1, (B,), generator=gen).tolist()
    c[0], c[-1] = N, 1
    return c


def _case(id, N, B, scales, seed, what, stage_scales=None):
    return dict(id=id, N=N, B=B, counts=_counts(N, B, seed), scales=list(scales), seed=seed, what=what,
                stage_scales=None if stage_scales is None else list(stage_scales))


CASES = [
    _case("n7-b2050", 7, 2050, [2, 5, 7], 11,
          "pairwise 4 scenes per workgroup, the last one 2; three hyper groups banded 4 / rows 6; eight hyper groups "
          "banded 8 (last 2) / rows 15 (last 10); XCD remap with padding blocks; top-k of a whole scene per band",
          stage_scales=[1, 2, 3, 4, 5, 6, 7, 7]),
    _case("n17-b1030", 17, 1030, [2, 5, 17], 13,
          "pairwise 2 scenes per workgroup; rows 3 (last 1) with the 17-member scale-N edge beside short rows in one "
          "wave; banded 2; top-k band of N rows"),
    _case("n50-b521", 50, 521, [2, 4, 8, 16], 15, "row form chosen by size, 2 scenes per workgroup, the last one 1"),
    _case("n17-b1930", 17, 1930, [2, 5, 17], 17, "the ragged scatter strides: B N 32 > 4096 x 256"),
]
BY_ID = {c["id"]: c for c in CASES}


def staged(case: Dict) -> Dict:
    """The case with its stage-level hyper groups (`stage_scales`) as its scales."""
    return dict(case, scales=case["stage_scales"], id=case["id"] + "-stage")


def groups_of(case: Dict, groups: str) -> Dict:
    return staged(case) if groups == "stage" else case


# ---------------------------------------------------------------------------------------------------------------------
# the launchers' rules, restated (gn_graph.hip: n2e_pair_shape, node2edge_plan, topk_plan, capped_grid)
# ---------------------------------------------------------------------------------------------------------------------
N2E_STAGE_MAX = 32 * 1024        # staged x' / pq rows of a workgroup of the pairwise and the banded body
N2E_ROWS_STAGE_MAX = 56 * 1024   # ... of the row body
N2E_ROW_PAIRS = 128              # lane pairs (hyperedge rows) of a row-form workgroup
N2E_MIN_WGS = 1024               # workgroups the hyper groups keep while scenes are packed
N2E_PAIR_MIN_WGS = 512           # ... a pairwise group
N2E_ROWS_MIN_E, N2E_ROWS_MIN_ROWS, N2E_ROWS_MAX_N = 24, 49152, 64     # the row form by launch size


def _n2e_scene_bytes(N: int) -> int:
    return N * (64 + 64 + 1) * 4                # x' rows and pq rows padded to 65 floats


def pair_scenes_per_wg(B: int, N: int) -> int:
    SG = 1
    while SG < 8 and 2 * SG * _n2e_scene_bytes(N) <= N2E_STAGE_MAX and cdiv(B, 2 * SG) >= N2E_PAIR_MIN_WGS:
        SG *= 2
    return SG


def pair_bands(B: int, E: int, SG: int) -> int:
    bands = 1
    while bands < 64 and SG * E // (bands * 2) >= 2048 and cdiv(B, SG) * bands < 2048:
        bands *= 2
    return bands


def banded_scenes_per_wg(B: int, N: int, nh: int) -> int:
    SG = 1
    while SG < 8 and 2 * SG * _n2e_scene_bytes(N) <= N2E_STAGE_MAX and cdiv(B, 2 * SG) * nh >= N2E_MIN_WGS:
        SG *= 2
    return SG


def rows_scenes_per_wg(B: int, N: int, nh: int, maxE: int) -> int:
    scene = 2 * N * (64 + 4) * 4                # x' and pq rows at a pitch of 68 floats
    SG = 1
    while ((SG + 1) * maxE <= N2E_ROW_PAIRS and (SG + 1) * scene <= N2E_ROWS_STAGE_MAX
           and cdiv(B, SG + 1) * nh >= N2E_MIN_WGS):
        SG += 1
    return SG


def n2e_plan(B: int, N: int, pair: Optional[str], Es: Sequence[int], switch: Optional[str]) -> Dict:
    """What gn_node2edge_* plans for one launch: pair — None, "sym" or "ord" (one pairwise group, first); Es — the
    hyperedge rows per scene of the hyper groups; switch — GN_N2E_ROWS ("0", "1", None: by launch size).
    -> {"variant" (1: row form), "SGh", "spw" (per group), "wgs" (per group), "xcd", "grid"}."""
    spw, wgs = [], []
    if pair is not None:
        SG = pair_scenes_per_wg(B, N)
        spw.append(SG)
        wgs.append(cdiv(B, SG) * pair_bands(B, pair_count(N) if pair == "sym" else N * N, SG))
    variant, SGh = 0, 1
    if Es:
        nh, maxE = len(Es), max(Es)
        by_size = maxE >= N2E_ROWS_MIN_E or B * sum(Es) >= N2E_ROWS_MIN_ROWS
        if N <= N2E_ROWS_MAX_N and switch != "0" and (by_size or switch == "1"):
            variant, SGh = 1, rows_scenes_per_wg(B, N, nh, maxE)
        else:
            SGh = banded_scenes_per_wg(B, N, nh)
        spw += [SGh] * nh
        wgs += [cdiv(B, SGh)] * nh
    grid = xcd_grid(wgs)
    return dict(variant=variant, SGh=SGh, spw=spw, wgs=wgs, xcd=int(sum(wgs) >= 64), grid=grid, padding=grid - sum(wgs))


def hyper_rows(N: int, scales: Sequence[int]) -> List[int]:
    return [C.n_edges(N, s) for s in scales]


# the node->edge launches of tests/test_ragged_sizes_gpu.py: (case, groups — "stage": the case's stage-level hyper groups,
# "block": its block's, None: the pairwise graph alone —, form, storage types)
N2E_LAUNCHES = [
    ("n7-b2050", "stage", "banded", ("fp32", "bf16")), ("n7-b2050", "stage", "rows", ("fp32",)),
    ("n7-b2050", "block", "banded", ("fp32",)), ("n7-b2050", "block", "rows", ("fp32",)),
    ("n7-b2050", None, "pair", ("fp32", "bf16")), ("n7-b2050", None, "pair-sym", ("fp32",)),
    ("n17-b1030", "block", "banded", ("fp32",)), ("n17-b1030", "block", "rows", ("fp32", "bf16")),
    ("n17-b1030", None, "pair", ("fp32",)), ("n17-b1030", None, "pair-sym", ("fp32",)),
    ("n50-b521", "block", "rows-by-size", ("fp32",)),
]
SWITCH = {"banded": "0", "rows": "1", "rows-by-size": None, "pair": None, "pair-sym": None}

# what each launch must reach: scenes per workgroup, scenes of the last workgroup (None: not named), row form
N2E_REACHES = {
    ("n7-b2050", "stage", "banded"): (8, 2, 0), ("n7-b2050", "stage", "rows"): (15, 10, 1),
    ("n7-b2050", "block", "banded"): (4, 2, 0), ("n7-b2050", "block", "rows"): (6, 4, 1),
    ("n7-b2050", None, "pair"): (4, 2, 0), ("n7-b2050", None, "pair-sym"): (4, 2, 0),
    ("n17-b1030", "block", "banded"): (2, None, 0), ("n17-b1030", "block", "rows"): (3, 1, 1),
    ("n17-b1030", None, "pair"): (2, None, 0), ("n17-b1030", None, "pair-sym"): (2, None, 0),
    ("n50-b521", "block", "rows-by-size"): (2, 1, 1),
}


def launch_plan(case_id: str, groups: Optional[str], form: str) -> Dict:
    """`n2e_plan` of one of N2E_LAUNCHES."""
    case = BY_ID[case_id]
    B, N = case["B"], case["N"]
    if groups is None:
        return n2e_plan(B, N, "sym" if form == "pair-sym" else "ord", [], None)
    return n2e_plan(B, N, None, hyper_rows(N, groups_of(case, groups)["scales"]), SWITCH[form])


def planned_scenes_per_wg(case_id: str) -> List[int]:
    """Every scenes-per-workgroup value > 1 a launch of the case is planned with (the block's launches included)."""
    case = BY_ID[case_id]
    B, N = case["B"], case["N"]
    sgs = {launch_plan(c, g, f)["spw"][0] for c, g, f, _ in N2E_LAUNCHES if c == case_id}
    if any(c == case_id for c, *_ in BLOCKS):            # the block's launch: pairwise + hyper groups, banded or by size
        sgs.update(n2e_plan(B, N, "sym", hyper_rows(N, case["scales"]), None)["spw"])
        sgs.update(n2e_plan(B, N, "ord", hyper_rows(N, case["scales"]), None)["spw"])
    return sorted(s for s in sgs if s > 1)


# the whole-block runs: (case, matrix path, storage)
BLOCKS = [("n7-b2050", "f16x3", "fp32"), ("n7-b2050", "bf16x6", "fp32"), ("n7-b2050", "fp32", "fp32"),
          ("n7-b2050", "f16x3", "bf16"), ("n17-b1030", "f16x3", "fp32")]


def mixed_workgroups(counts: Sequence[int], SG: int) -> Tuple[int, int]:
    """(workgroups of SG consecutive scenes that hold a later scene with a LARGER count than their first, ... with a
    SMALLER one): a body that took its workgroup's first count is then wrong in both directions."""
    up = down = 0
    for b0 in range(0, len(counts), SG):
        first, rest = counts[b0], counts[b0 + 1:b0 + SG]
        up += any(c > first for c in rest)
        down += any(c < first for c in rest)
    return up, down


def first_counts(counts: Sequence[int], SG: int) -> List[int]:
    """Per scene the count of the first scene of its workgroup of SG scenes (the seeded flaw)."""
    return [counts[b - b % SG] for b in range(len(counts))]


def topk_scales(case: Dict) -> List[int]:
    """Every top-k scale the case ranks (block and stage level), the scale N — one hyperedge of all agents — left out."""
    return sorted({s for s in case["scales"] + (case["stage_scales"] or []) if s != case["N"]})


# ---------------------------------------------------------------------------------------------------------------------
# count classes
# ---------------------------------------------------------------------------------------------------------------------
def classes(case: Dict, scenes: Optional[Sequence[int]] = None) -> List[Tuple[int, torch.Tensor]]:
    """[(n, the scenes with n agents)] over the batch (or over `scenes`), n ascending."""
    cnt = torch.tensor(case["counts"])
    sel = torch.arange(case["B"]) if scenes is None else torch.as_tensor(list(scenes), dtype=torch.long)
    return [(int(n), sel[cnt[sel] == n]) for n in torch.unique(cnt[sel]).tolist()]


def class_corr(h: torch.Tensor, idx: torch.Tensor, n: int) -> torch.Tensor:
    """The fp32 affinity (m, n, n) of the scenes idx, each alone at its n agents."""
    return O.affinity(h[idx, :n].float())


def class_incidence(corr: torch.Tensor, s: int, N: int) -> torch.Tensor:
    """`ragged_cases.scene_incidence` of a whole class: corr (m, n, n) -> (m, 1, n) of ones for s == N, else (m, n, n) with
    the top-min(s, n) of every row."""
    m, n = corr.shape[0], corr.shape[1]
    if s == N:
        return torch.ones(m, 1, n)
    k = min(max(int(s), 1), n)
    return torch.zeros(m, n, n).scatter(2, corr.topk(k, dim=2).indices, 1)


def scene_gaps(case: Dict, h: torch.Tensor) -> torch.Tensor:
    """(B,) per scene the smallest gap between the k-th and (k+1)-th affinity over its valid rows and every top-k scale
    (k = min(s, n) < n; inf where no row has a selection to keep apart)."""
    out = torch.full((case["B"],), float("inf"))
    for n, idx in classes(case):
        v = torch.sort(class_corr(h, idx, n), dim=-1, descending=True).values
        for s in topk_scales(case):
            k = min(max(s, 1), n)
            if k < n:
                out[idx] = torch.minimum(out[idx], (v[..., k - 1] - v[..., k]).amin(dim=-1))
    return out


@functools.lru_cache(maxsize=None)
def _features(case_id: str) -> Tuple[torch.Tensor, Tuple[int, ...]]:
    """(h (B, N, 64) fp32, scenes redrawn per draw): every scene keeps the first draw whose fp32 values AND bf16 roundings
    keep MIN_GAP at every valid row."""
    case = BY_ID[case_id]
    B, N = case["B"], case["N"]
    h, need, redrawn = None, torch.ones(B, dtype=torch.bool), []
    for d in range(DRAWS):
        gen = torch.Generator().manual_seed(1000 + case["seed"] + 100003 * d)
        cand = torch.randn(B, N, 64, generator=gen)
        h = cand if h is None else torch.where(need[:, None, None], cand, h)
        gap = torch.minimum(scene_gaps(case, h), scene_gaps(case, h.bfloat16().float()))
        need = gap < C.MIN_GAP
        redrawn.append(int(need.sum()))
        if not need.any():
            return h, tuple(redrawn)
    raise AssertionError(f"{case_id}: {int(need.sum())} scenes found no draw in {DRAWS} (raise DRAWS)")


def redraws(case_id: str) -> Tuple[int, ...]:
    """Scenes still too close after draw 0, 1, ... (the last entry is 0)."""
    return _features(case_id)[1]


@functools.lru_cache(maxsize=None)
def inputs(case_id: str, bf16: bool = False):
    """(h (B, N, 64), U: per module of the case's block, pairwise first, one uniform tensor of the PADDED shape).  bf16: h
    rounded to bf16 (as fp32 values).  Shared, never written to."""
    case = BY_ID[case_id]
    h = _features(case_id)[0]
    gen = torch.Generator().manual_seed(2000 + case["seed"])
    U = [[torch.rand(shp, generator=gen)] for shp in C.noise_shapes(case)]
    return (h.bfloat16().float() if bf16 else h), U


def valid_nodes(case: Dict) -> torch.Tensor:
    """(B, N) bool: n < n_b."""
    return torch.arange(case["N"])[None, :] < torch.tensor(case["counts"])[:, None]


def valid_rows(case: Dict, kind) -> torch.Tensor:
    """(B, E) bool, the rows a scene owns: kind "ord" — ordered pairs i*N + j with i, j < n_b; "sym" — unordered pairs;
    an int s — the hyperedge rows of a scale-s module (e < n_b, or the single row of scale N)."""
    N, v = case["N"], valid_nodes(case)
    if kind == "ord":
        return (v[:, :, None] & v[:, None, :]).reshape(case["B"], N * N)
    if kind == "sym":
        iu = torch.triu_indices(N, N)
        return v[:, iu[0]] & v[:, iu[1]]
    return torch.ones(case["B"], 1, dtype=torch.bool) if kind == N else v


def sym_rows(N: int, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rows of the symmetric form p(i, j) = i N - i (i - 1) / 2 + (j - i), the ordered edges i*n + j of an n-agent scene)
    of the pairs i <= j < n, row-major."""
    iu = torch.triu_indices(n, n)
    i, j = iu[0], iu[1]
    return i * N - i * (i - 1) // 2 + (j - i), i * n + j


def padded_incidence(case: Dict, h: torch.Tensor, s: int) -> torch.Tensor:
    """(B, E, N): every scene's contract incidence embedded in zeros (`ragged_cases.padded_incidence`, by count class)."""
    N = case["N"]
    out = torch.zeros(case["B"], C.n_edges(N, s), N)
    for n, idx in classes(case):
        H = class_incidence(class_corr(h, idx, n), s, N)
        out[idx, :H.shape[1], :n] = H
    return out


def padded_corr(case: Dict, h: torch.Tensor) -> torch.Tensor:
    out = torch.zeros(case["B"], case["N"], case["N"])
    for n, idx in classes(case):
        out[idx, :n, :n] = class_corr(h, idx, n)
    return out


def with_garbage(case: Dict, t: torch.Tensor, valid: torch.Tensor, seed: int = 77, scale: float = 100.0) -> torch.Tensor:
    """t with every position outside `valid` (a bool mask over t's leading dims) replaced by N(0,1) x scale."""
    gen = torch.Generator().manual_seed(seed + case["seed"])
    g = torch.randn(t.shape, generator=gen) * scale
    return torch.where(valid.reshape(valid.shape + (1,) * (t.dim() - valid.dim())), t, g)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 oracle by count class
# ---------------------------------------------------------------------------------------------------------------------
def _class_noise(U_mod: List[torch.Tensor], idx: torch.Tensor, N: int, n: int, pairwise: bool) -> List[torch.Tensor]:
    """`ragged_cases.scene_noise` of a whole class, in float64."""
    out = []
    for u in U_mod:
        ub = u[idx]
        if pairwise:
            ub = ub[:, C.pair_index(N, n)]
        elif ub.shape[1] != 1:
            ub = ub[:, :n]
        out.append(ub.double())
    return out


def class_oracle(sp, shs, case: Dict, h: torch.Tensor, U, n: int, idx: torch.Tensor, nmp: int = 1):
    """The scenes idx (all of n agents) as one batch of n-agent scenes, in float64 -> (node features per module
    (m, n, 64), factors per module, incidences per scale (m, e, n)): `ragged_cases.scene_oracle` of every scene at once."""
    N = case["N"]
    hb = h[idx, :n].double()
    with torch.no_grad():
        nf, fac = O.ms_hgnn_pairwise_forward(state64(sp), hb, _class_noise(U[0], idx, N, n, True), nmp, decomposed=True)
        feats, facs, Hs = [nf], [fac], []
        corr = class_corr(h, idx, n)
        for sh, s, Um in zip(shs, case["scales"], U[1:]):
            H = class_incidence(corr, s, N)
            nf, fac = O._message_passing(state64(sh), hb, H.double(), _class_noise(Um, idx, N, n, False), nmp, True, None)
            feats.append(nf)
            facs.append(fac)
            Hs.append(H)
    return feats, facs, Hs


@functools.lru_cache(maxsize=None)
def block_oracle(case_id: str, bf16: bool = False):
    """The whole block on EVERY scene, embedded in zeros: (features (B, N, 64 (1 + S)) float64, factors per module
    (B, E, K) float64, per module the largest |feature|).  Computed once and shared (never written to)."""
    case = BY_ID[case_id]
    B, N, S = case["B"], case["N"], len(case["scales"])
    _, sp, shs = C.cpu_block(case)
    h, U = inputs(case_id, bf16)
    feats = torch.zeros(B, N, 64 * (1 + S), dtype=torch.float64)
    facs = [torch.zeros(u[0].shape, dtype=torch.float64) for u in U]
    for n, idx in classes(case):
        f, fc, _ = class_oracle(sp, shs, case, h, U, n, idx)
        feats[idx, :n] = torch.cat(f, dim=-1)
        facs[0][idx[:, None], C.pair_index(N, n)[None, :]] = fc[0]
        for i in range(1, 1 + S):
            facs[i][idx, :fc[i].shape[1]] = fc[i]
    scale = [float(feats[..., 64 * i:64 * (i + 1)].abs().max()) for i in range(1 + S)]
    return feats, facs, scale


def _n2e64(state, hb: torch.Tensor, H: torch.Tensor, chunk: int = 64) -> torch.Tensor:
    """`O.node2edge` in float64 on a class, a few scenes at a time (the hidden tensor is (m, E, n, 32))."""
    s64 = state64(state)
    with torch.no_grad():
        return torch.cat([O.node2edge(s64, hb[i:i + chunk].double(), H[i:i + chunk].double(), 0, True)[0]
                          for i in range(0, hb.shape[0], chunk)])


def hyper_n2e_oracle(case: Dict, h: torch.Tensor, shs, scenes: Optional[Sequence[int]] = None) -> List[torch.Tensor]:
    """Per hyper group of `case` the float64 `O.node2edge` rows of every scene (or of `scenes`), embedded in zeros:
    [(B, E, 64)] (rows of scenes outside `scenes` stay zero: compare the chosen scenes only)."""
    B, N = case["B"], case["N"]
    out = [torch.zeros(B, C.n_edges(N, s), 64, dtype=torch.float64) for s in case["scales"]]
    for n, idx in classes(case, scenes):
        corr = class_corr(h, idx, n)
        for ref, sh, s in zip(out, shs, case["scales"]):
            r = _n2e64(sh, h[idx, :n], class_incidence(corr, s, N))
            ref[idx, :r.shape[1]] = r
    return out


def pair_n2e_oracle(case: Dict, h: torch.Tensor, sp, sym: bool) -> torch.Tensor:
    """The pairwise graph's float64 `O.node2edge` rows of every scene, embedded in zeros: (B, N N, 64) at the ordered
    rows i*N + j, or (B, N (N + 1) / 2, 64) at the rows of the symmetric form."""
    B, N = case["B"], case["N"]
    out = torch.zeros(B, pair_count(N) if sym else N * N, 64, dtype=torch.float64)
    for n, idx in classes(case):
        r = _n2e64(sp, h[idx, :n], O.pairwise_incidence(n, len(idx)))
        rows, src = sym_rows(N, n) if sym else (C.pair_index(N, n), torch.arange(n * n))
        out[idx[:, None], rows[None, :]] = r[:, src]
    return out


def node2edge_counted(state, x: torch.Tensor, H: torch.Tensor, nv: torch.Tensor) -> torch.Tensor:
    """Node -> edge pooling of the scenes x (m, n, 64) with incidence H (m, E, n), the softmax running over nv[b] nodes
    instead of n: nv[b] - |members| non-members add exp(0 - max) each, and zero enters the maximum iff one exists — where
    the per-scene count enters the kernels' arithmetic.  nv == n is `O.node2edge`; a wrong nv is the seeded flaw."""
    with torch.no_grad():
        xp = O.mlp(state, "node2edge_start_mlp.0", x)
        W1, b1 = state["attention_mlp.0.layers.0.weight"], state["attention_mlp.0.layers.0.bias"]
        W2, b2 = state["attention_mlp.0.layers.1.weight"], state["attention_mlp.0.layers.1.bias"]
        P = torch.nn.functional.linear(xp, W1[:, :64], b1)
        Q = torch.nn.functional.linear(torch.matmul(H, xp), W1[:, 64:])
        att = torch.matmul(torch.relu(P[:, None] + Q[:, :, None]), W2[0]) + b2[0]
        member = H != 0
        others = (nv.reshape(-1, 1) - member.sum(-1)).clamp(min=0).to(x.dtype)         # (m, E)
        v = (att * H).masked_fill(~member, float("-inf"))
        mx = v.amax(dim=-1)
        mx = torch.where(others > 0, mx.clamp(min=0), mx)
        ex = torch.exp(v - mx[..., None])
        total = ex.sum(-1) + others * torch.exp(-mx)
        return torch.matmul(ex / total[..., None] * H, xp)
