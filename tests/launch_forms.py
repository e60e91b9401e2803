"""Test helper: which kernel forms the launchers pick at a given launch size, a scene sampler that aims at the
boundaries of those forms, and a float64 oracle evaluated on the sampled scenes only.

Why.  The launchers choose a work shape by launch size (waves per row block, scenes per workgroup, fused or unfused
closing stage, ...).  A full CPU oracle of a batch large enough to select the large-launch forms costs seconds to
minutes; scenes are independent, so the oracle runs on a sample of ~32-64 scenes while the HIP path runs the whole
batch, and the sampled rows are compared.  `expected_forms` states the launchers' rules in plain Python so that a test
can say which form a case reaches (tests/test_launch_forms_cpu.py checks that the case table reaches every value) and
a kernel trace can confirm it (the aggregation kernel's grid).
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import torch

from oracle import ms_hgnn_oracle as O

K_PAIR, K_HYPER = 6, 10          # edge types (MS_HGNN_batch.py: MS_HGNN_oridinary / MS_HGNN_hyper)
NODE_FORM_MAX_N, NODE_FORM_MAX_K = 16, 12      # route.NODE_FORM_MAX_N / NODE_FORM_MAX_K (ops re-exports the kernel limits)
SCENE_FORM_MAX_N = 64                          # route.SCENE_FORM_MAX_N
FUSED_MAX_N = 16                 # route._FUSED_GATHER_MAX_N / _FUSED_SCATTER_MAX_N / ops.POOL_MAX_N
BOTTLENECK = 64                  # the closing MLP's output width of every case that does not name one
IMAGE_MAX_DOUT = 64              # weights.closing_mlp / gn_mlp2_*: the bf16-core kernels (and bf16 storage) end here
ONE_TILE_MAX_DOUT = 32           # mlp2_plan: one 32-wide output tile up to here; the fused closing stage starts above it
RB2_MIN_PAIRS = 2048             # gn_mlp_mfma.hip rb2_min_pairs() without the test knob
GS_MIN_WGS = 2048                # gn_graph.hip kGsMinWgs
GS_LDS_BUDGET = 128 * 1024       # gn_graph.hip kLdsBudget
GS_TILE_MAX = 24 * 1024          # gn_graph.hip gs_scenes_per_wg: the tile of a workgroup that packs several scenes
SCATTER_PAIRS_MAX_N, SCATTER_PAIRS_MIN_B = 64, 256      # agg_scatter_pairs_kernel: 16 N <= 256 x 4 items, B fills the chip
CAPPED_GRID = 256 * 16           # gn_graph.hip capped_grid: workgroups of a grid-stride launch


def pair_count(N: int) -> int:
    return N * (N + 1) // 2


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def xcd_grid(counts: Sequence[int]) -> int:
    """Workgroups of a launch whose groups are dealt over the 8 XCDs in sections (gn_common.hpp gn_xcd_grid)."""
    total = sum(counts)
    if len(counts) > 32 or total < 64:      # (GN_MAX_SECTIONS = 32)
        return total
    worst = 0
    for x in range(8):
        worst = max(worst, sum((W * (x + 1) >> 3) - (W * x >> 3) for W in counts))
    return 8 * worst


def agg_wpr(rows: int, K: int) -> int:
    """Waves per 32-row block of the typed aggregation (gn_mlp_mfma.hip agg_launch: `wpr = blocks32 >= 768 ? 1 : ...`)."""
    b32 = cdiv(rows, 32)
    return 1 if b32 >= 768 else (2 if b32 >= 128 and K >= 2 else (4 if K >= 4 else 1))


def gs_scenes_per_wg(per_scene: int, B: int, nh: int) -> int:
    """Scenes per workgroup of a staged gather / scatter launch of nh groups: doubled while the doubled tile stays within
    GS_TILE_MAX and the grid keeps GS_MIN_WGS workgroups, 16 at most."""
    G = 1
    while G < 16 and 2 * G * per_scene <= GS_TILE_MAX and cdiv(B, 2 * G) * nh >= GS_MIN_WGS:
        G *= 2
    return G


def scatter_forms(B: int, N: int, groups: Sequence[Dict], pairs_switch: bool = True) -> Optional[Dict]:
    """The launches of one gn_agg_scatter_* call (gn_graph.hip scatter_plan, restated).  groups: [{"E", "sym" (the
    unordered pairs of the pairwise graph), "H" (a hyper group with a dense incidence), "colmask" (... in mask form)}];
    pairs_switch: GN_SCATTER_PAIRS is not 0.
    -> {"own": {group: (kernel, grid)} — launched on their own, in group order: the pairs kernel (one workgroup per scene)
    iff sym, 16 N <= 1024, B >= 256 and the switch; else the direct kernel, which also takes a hyper group whose feat rows
    and H, E (64 + N) floats, exceed 64 KiB —, "pos": per group its position in the staged launch or -1, "kernel" (None
    without staged groups), "grid", "G", "Emax", "dyn_lds"}; None for dense and mask hyper groups in one call (refused)."""
    get = lambda g, k: bool(g.get(k))
    n_mask = sum(get(g, "colmask") for g in groups)
    if n_mask and any(get(g, "H") and not get(g, "colmask") for g in groups):
        return None
    own, pos, nh = {}, [], 0
    for i, g in enumerate(groups):
        if get(g, "colmask") or (get(g, "H") and g["E"] * (64 + N) * 4 <= GS_LDS_BUDGET // 2):
            pos.append(nh)
            nh += 1
            continue
        pos.append(-1)
        if (not get(g, "H") and get(g, "sym") and N <= SCATTER_PAIRS_MAX_N and B >= SCATTER_PAIRS_MIN_B and pairs_switch):
            own[i] = ("agg_scatter_pairs_kernel", B)
        else:
            own[i] = ("agg_scatter_direct_kernel", min(max(cdiv(B * N * 32, 256), 1), CAPPED_GRID))
    out = dict(own=own, pos=pos, kernel=None, grid=None, G=0, Emax=0, dyn_lds=0)
    if nh:
        Emax = max(g["E"] for g, q in zip(groups, pos) if q >= 0)
        per_scene = Emax * 256 + (N * 8 if n_mask else Emax * N * 4)
        G = gs_scenes_per_wg(per_scene, B, nh)
        out.update(kernel="agg_scatter_mask_kernel" if n_mask else "agg_scatter_kernel", grid=(cdiv(B, G), nh), G=G,
                   Emax=Emax, dyn_lds=G * per_scene)
    return out


def assert_scatter_plan(sf: Dict, plan, where) -> None:
    """A gn_agg_scatter_plan_* plan says what `sf` (scatter_forms) says."""
    from groupnet_amd import _lib as L
    name = lambda k: L.load().gn_kernel_name(k).decode()
    n = len(sf["pos"])
    assert plan.n_groups == n and list(plan.pos[:n]) == sf["pos"], (where, list(plan.pos[:n]))
    for i in range(n):
        if i in sf["own"]:
            assert (name(plan.pre_kernel[i]), plan.pre_grid[i], plan.wgs[i], plan.spw[i]) == (*sf["own"][i], 0, 0), (where, i)
        else:
            assert (plan.pre_kernel[i], plan.pre_grid[i], plan.wgs[i], plan.spw[i]) == (0, 0, sf["grid"][0], sf["G"]), (where, i)
    if sf["kernel"] is None:
        assert plan.kernel == 0, where
    else:
        assert (name(plan.kernel), tuple(plan.grid), plan.G, plan.TE, plan.dyn_lds) == (
            sf["kernel"], sf["grid"] + (1,), sf["G"], sf["Emax"], sf["dyn_lds"]), (where, sf)


def module_types(scales: Sequence[int], with_pair: bool = True, types: Optional[Sequence[int]] = None) -> List[int]:
    """Edge types K per module in group order (the pairwise module first where present): `types` as given — one K per
    module — or the reference's 6 / 10."""
    n = int(with_pair) + len(scales)
    if types is None:
        return ([K_PAIR] if with_pair else []) + [K_HYPER] * len(scales)
    assert len(types) == n, f"types: one K per module ({n}), got {tuple(types)}"
    return [int(k) for k in types]


def mlp2_form(dout: int, rows: int, n_groups: int, precision: str = "f16x3", dtype: str = "fp32", fused_input: bool = True,
              wide_hyper: bool = False, xs: Optional[bool] = None, dh: int = 128):
    """(kernel, tiles[2]) of one closing-MLP launch (gn_mlp_mfma.hip mlp2_plan), None where the launcher refuses it.
    dout: the output width; rows x n_groups: the launch size; fused_input: a group forms its input rows itself
    (ScatterSpec / NodeAggSpec) or keeps its activations; wide_hyper: a fused scatter over more than 16 hyperedges; xs:
    GN_MLP2_XS as a bool (None: unset).  Up to IMAGE_MAX_DOUT the 16-bit cores (and bf16 storage) run mlp2_xs_kernel /
    mlp2_x_kernel by launch size, instantiated with one output tile up to ONE_TILE_MAX_DOUT and with two above it; the
    fp32 cores run the 4-waves-per-block split kernel on a small launch of plain rows (dh = 128) and mlp2_kernel
    otherwise, neither instantiated by output tiles (0).  Beyond IMAGE_MAX_DOUT there is no image: fp32 storage runs
    mlp2_kernel whatever the matrix path (the split kernel holds two output tiles), bf16 storage is refused."""
    twin = dtype == "bf16"
    b32 = cdiv(rows, 32)
    if dout > IMAGE_MAX_DOUT:
        return None if twin else ("mlp2_kernel", 0)
    if twin or precision != "fp32":
        small = (b32 * n_groups <= 1536) if xs is None else xs
        return ("mlp2_xs_kernel" if small and not wide_hyper else "mlp2_x_kernel"), (1 if dout <= ONE_TILE_MAX_DOUT else 2)
    return ("mlp2_split_kernel" if dh == 128 and b32 * n_groups <= 1024 and not fused_input else "mlp2_kernel"), 0


def expected_forms(B: int, N: int, scales: Sequence[int], precision: str = "f16x3", dtype: str = "fp32",
                   training: bool = False, block: bool = True, with_pair: bool = True,
                   types: Optional[Sequence[int]] = None, bottleneck: int = BOTTLENECK) -> Dict:
    """The forms the launchers pick for one forward of the multiscale block (`block=True`, latency form: closing fused
    where allowed) or of the same modules launched one by one through the module API (`block=False`: no fused closing).
    precision: ops.precision() of the fp32 entry points ('f16x3' | 'bf16x6' | 'fp32'); dtype: 'fp32' | 'bf16' storage.

    Returns {"groups": [per module: {"name", "E", "K", "rows", "node_form", "wpr", "spw"}], "fused_closing",
    "agg_kernel", "agg_wgs", "agg_grid" (of the launch of the groups that are not in the twins' scene form), "agg_pos"
    (per module its position in that launch, -1 for the scene form), "scene_grid",
    "mlp2", "mlp2_tiles", "mlp2_refused", "n2e", "gather_spw", "scatter" (scatter_forms of the stand-alone scatter)};
    "scene_grid" / "mlp2" / "n2e" / "gather_spw" / "scatter" are None where that launch does not run.
    with_pair=False: the hyper modules alone (one MS_HGNN_hyper through the module API).
    types: the edge types K of every module in group order, (K_pair, K_hyper, ...) (default: 6 and 10).
    bottleneck: the output width of the closing MLP of the last round (default 64): the fused closing stage exists for
    32 < bottleneck <= 64 only, the closing launch's kernel is `mlp2_form`'s; "mlp2_refused": bf16 storage beyond 64, which
    the launcher refuses ("mlp2" is None there although the forward would need the launch).

    These rules restate the launchers' plan functions independently of them: tests/test_launch_plan_cpu.py holds the two
    against each other through the library's plan queries (no GPU), and a kernel trace of tests/test_launch_forms_gpu.py's
    forward cases shows the aggregation grid `agg_grid` (and the scene form's `scene_grid`) for every case."""
    twin = dtype == "bf16"
    xm = twin or precision != "fp32"            # bf16-core images (ops.BF16X6) or the twins
    mods = ([("pair", None)] if with_pair else []) + [(f"hyper{s}", s) for s in scales]
    groups = []
    for (name, s), Km in zip(mods, module_types(scales, with_pair, types)):
        if s is None:
            E, K = pair_count(N), Km
            # route.message_passing_route: the pair form's node form (the 16-bit-core images, N <= NODE_FORM_MAX_N ...) on
            # fp32 storage, the scene form (N <= SCENE_FORM_MAX_N) on the twins (ops.node_form_enabled() is on by default)
            node = (N <= SCENE_FORM_MAX_N) if twin else (xm and N <= NODE_FORM_MAX_N and K <= NODE_FORM_MAX_K)
        else:
            E, K, node = (1 if s == N else N), Km, False
        rows = B * E
        groups.append(dict(name=name, E=E, K=K, rows=rows, node_form=node, wpr=1 if node else agg_wpr(rows, K), spw=0))
    hyp = [g for g in groups if g["name"] != "pair"]
    # ops.closing_fusable + the route's `ask_closing` (and agg_launch's own checks): fp32 results on the 16-bit cores,
    # N <= 16, the pairwise group in its node form, every hyper group with E <= 16 and more than one wave per row block
    # (below 768 row blocks; K >= 4 below 128 row blocks, K >= 2 from there on)
    fused = (block and with_pair and not training and not twin and xm and N <= FUSED_MAX_N and groups[0]["node_form"]
             and all(g["E"] <= 16 and g["wpr"] > 1 for g in hyp)
             and ONE_TILE_MAX_DOUT < bottleneck <= IMAGE_MAX_DOUT)      # (closing_chain is built for two output tiles)
    if fused:
        for g in hyp:       # agg_launch: `spw = (128 / wpr) / E`, capped at node_cap / N nodes
            g["spw"] = min((128 // g["wpr"]) // g["E"], (160 if g["E"] == 1 else 64) // N)
    # the twins' scene form (node form without the per-node first layer) runs in a launch of its own, one workgroup per
    # 32 nodes of a scene (agg_launch: agg_scene_kernel), ahead of the launch of the other groups
    scene_grid = None
    main = groups
    if twin and groups[0]["node_form"]:
        scene_grid, main = B * cdiv(N, 32), groups[1:]
    wgs = []
    for g in main:
        if g["node_form"]:
            wgs.append(cdiv(B * N, 32))
        elif g["spw"]:
            wgs.append(cdiv(B, g["spw"]))
        else:
            wgs.append(cdiv(cdiv(g["rows"], 32) * g["wpr"], 4))
    # the groups' order inside that launch (agg_plan's `cost`): longest waves first — types x layers of a wave's share,
    # the node form last —, equal costs in the caller's order
    cost = lambda g: 1 if g["node_form"] else g["K"] * (1 if g["name"] == "pair" and not twin else 2) * 4 // g["wpr"]
    by_cost = sorted(range(len(main)), key=lambda i: -cost(main[i]))
    agg_pos = [-1] * (len(groups) - len(main)) + [by_cost.index(i) for i in range(len(main))]
    if twin and sum(cdiv(cdiv(g["rows"], 32), 2) for g in main) >= RB2_MIN_PAIRS:
        agg_kernel = "agg_rb2_kernel"
        wgs = [cdiv(cdiv(g["rows"], 32), 8) for g in main]
        grid = xcd_grid(wgs)
    elif xm:
        agg_kernel, grid = "agg_x_kernel", xcd_grid(wgs)
    else:
        agg_kernel, grid = "agg_mlp_kernel", sum(wgs)
    # closing MLP launch (gn_mlp_mfma.hip mlp2_plan); din = 128, dh = 128, dout = bottleneck.  Its input rows are formed in
    # the kernel up to N = 16 (a fused scatter: never the fp32 cores' split kernel) and kept in training
    mlp2 = mlp2_tiles = None
    refused = False
    if not fused:
        form = mlp2_form(bottleneck, B * N, len(groups), precision, dtype, fused_input=N <= FUSED_MAX_N or training)
        refused = form is None
        if form is not None:
            mlp2, mlp2_tiles = form
    # node -> edge pooling of the hyper modules (gn_graph.hip node2edge_launch): launched for training, the fp32 cores and
    # N > POOL_MAX_N (the route's `node2edge` launch); row form when `maxE >= 24 || hyper_rows >= 49152`
    n2e = None
    if hyp and (training or not xm or N > FUSED_MAX_N):
        hyper_rows = sum(g["rows"] for g in hyp)
        n2e = "rows" if N <= 64 and (max(g["E"] for g in hyp) >= 24 or hyper_rows >= 49152) else "banded"
    # stand-alone gather of the hyper modules for N > 16 (gn_graph.hip gather_launch): scenes per workgroup
    gather_spw = None
    if hyp and N > FUSED_MAX_N:
        Emax, nh = max(g["E"] for g in hyp), len(hyp)
        per_scene = N * 64 * 4 + Emax * N * 4
        gather_spw = gs_scenes_per_wg(per_scene, B, nh) if per_scene <= GS_LDS_BUDGET else 1
    # stand-alone scatter for N > 16 (the route's `scatter` launch): exactly the groups whose aggregation wrote per-edge
    # features, i.e. that are not in node form
    scatter = None
    rest = [g for g in groups if not g["node_form"]]
    if rest and N > FUSED_MAX_N:
        scatter = scatter_forms(B, N, [dict(E=g["E"], sym=g["name"] == "pair", H=g["name"] != "pair") for g in rest])
    return dict(scatter=scatter, groups=groups, fused_closing=fused, agg_kernel=agg_kernel, agg_wgs=sum(wgs), agg_grid=grid,
                agg_pos=agg_pos, scene_grid=scene_grid, mlp2=mlp2, mlp2_tiles=mlp2_tiles, mlp2_refused=refused, n2e=n2e,
                gather_spw=gather_spw)


# ---------------------------------------------------------------------------------------------------------------------
# the graph stage: cosine affinity + top-k incidence
# ---------------------------------------------------------------------------------------------------------------------
AFF_TAIL_LDS = 24 * 1024         # gn_mlp_mfma.hip kAffTailLds: a scene tile the node stage's tail workgroups may take
AFF_LDS_BUDGET = 128 * 1024      # gn_graph.hip kLdsBudget: ... and the stand-alone fused launch
AFF_BAND_ROWS, AFF_PANEL_COLS = 16, 64      # affinity_banded_kernel: rows of a workgroup's band, columns of a staged panel
TOPK_MIN_WGS = 1024              # gn_topk_incidence_f32 halves its band while the launch has fewer workgroups ...
TOPK_MIN_RB = 8                  # ... and more than this many rows per band


def affinity_tile(N: int, D: int = 64, x_dim: int = 0, mask_scales: int = 0) -> int:
    """LDS bytes of one scene of the fused affinity + top-k code (gn_affinity.hpp affinity_fused_lds: rows at stride
    D + 4, the pad to 8 bytes, 64-bit ranking keys, the raw inputs of the embedding form; affinity_mask_lds: the row and
    column words of every scale of a launch that emits masks)."""
    tile = N * (D + 4) * 4 + 8 + N * N * 8 + N * x_dim * 4
    return tile + (8 + 2 * mask_scales * N * 8 if mask_scales else 0)


def topk_bands(B: int, N: int):
    """(RB, bands, N % RB) of gn_topk_incidence_f32: RB rows of corr per workgroup — as many as half the LDS budget
    holds, at most N, halved (rounding up) while the launch has fewer than 1024 workgroups and RB > 8.  None where the
    entry refuses N (not one row fits)."""
    RB = (AFF_LDS_BUDGET // 2) // (4 * N)
    if RB == 0:
        return None
    RB = min(RB, N)
    while RB > TOPK_MIN_RB and B * cdiv(N, RB) < TOPK_MIN_WGS:
        RB = (RB + 1) // 2
    return RB, cdiv(N, RB), N % RB


def graph_forms(B: int, N: int, D: int = 64, x_dim: int = 0, masks: bool = False, scales: Sequence[int] = ()) -> Dict:
    """Which form builds the graph of B scenes of N agents with D features (x_dim raw inputs per agent in the embedding
    form; masks: the launch also emits the bit-mask form of every scale of `scales`):
      "tail"   — tail workgroups of the node-stage launch (no masks; tile within AFF_TAIL_LDS),
      "fused"  — the stand-alone fused launch (tile, mask words included, within AFF_LDS_BUDGET),
      "banded" — affinity_banded_kernel + topk_incidence_kernel.
    -> {"form", "tile" (bytes, of the fused code), "aff_grid" ((cdiv(N,16), B)), "aff_last" ((rows of the last band,
    columns of the last panel)), "topk" ((RB, bands, N % RB))}; the last three are None unless the form is "banded".
    Restates the launchers' arithmetic; tests/test_graph_forms_cpu.py holds it against the library without a launch."""
    tile = affinity_tile(N, D, x_dim, len(scales) if masks else 0)
    if not masks and tile <= AFF_TAIL_LDS:
        form = "tail"
    elif tile <= AFF_LDS_BUDGET:
        form = "fused"
    else:
        form = "banded"
    out = dict(form=form, tile=tile, aff_grid=None, aff_last=None, topk=None)
    if form == "banded":
        out.update(aff_grid=(cdiv(N, AFF_BAND_ROWS), B),
                   aff_last=((N - 1) % AFF_BAND_ROWS + 1, (N - 1) % AFF_PANEL_COLS + 1), topk=topk_bands(B, N))
    return out


def largest_fused_n(D: int = 64, x_dim: int = 0, mask_scales: int = 0, budget: int = AFF_LDS_BUDGET) -> int:
    """The largest N whose tile is within `budget` (the tile grows with N)."""
    N = 1
    while affinity_tile(N + 1, D, x_dim, mask_scales) <= budget:
        N += 1
    return N


# the cases of tests/test_graph_forms_gpu.py (tests/test_graph_forms_cpu.py checks what they reach)
# gn_affinity_f32 alone, (B, N, D): the ragged banded shapes, the existing exact one, the largest fused tile, the first N
# beyond the tail; other D at a small N and at the switch pair of D = 128
AFFINITY_CASES = [(2, 113, 64), (2, 129, 64), (1, 200, 64), (3, 256, 64), (2, 112, 64), (2, 41, 64)]
AFFINITY_D_CASES = [(2, 11, 4), (2, 11, 36), (2, 11, 128), (2, 99, 128), (2, 100, 128)]
# gn_topk_incidence_f32 alone, (B, N): one band of all N rows (twice), the LDS cap with a short last band, a halved band
# with a remainder, RB < 8, RB = 8 with a last band of one row
TOPK_CASES = [(1024, 11), (1024, 113), (1024, 200), (300, 200), (3, 200), (2, 113)]
# the fused launch through ops.affinity_topk, (B, N), and the block through the engine
FUSED_CASES = [(3, 40), (3, 41), (3, 112)]
ENGINE_CASES = [(3, 40), (3, 41), (1, 112), (1, 113)]


# gn_agg_scatter_* once per planned form (tests/test_graph_forms_gpu.py), at the smallest shapes that reach it:
# (B, N, groups, storage types, what the plan must say: the kernel of the group's own launch, or the staged kernel and G).
# groups: one letter per group — s: the unordered pairs, o: the ordered pairs, h: a hyper group (E = N, dense H), m: the
# same in mask form.  B = 4095 (one group) and 3265 (ten groups) are the first B that pack 2 and 16 scenes per workgroup;
# both leave ONE scene to the last workgroup.
SCATTER_GPU_CASES = [
    (256, 11, "s", ("fp32", "bf16"), ("agg_scatter_pairs_kernel", 0)), (256, 64, "s", ("fp32", "bf16"), ("agg_scatter_pairs_kernel", 0)),
    (255, 11, "s", ("fp32",), ("agg_scatter_direct_kernel", 0)), (256, 65, "s", ("fp32",), ("agg_scatter_direct_kernel", 0)),
    (3, 11, "o", ("fp32",), ("agg_scatter_direct_kernel", 0)), (2, 100, "h", ("fp32",), ("agg_scatter_direct_kernel", 0)),
    (2, 99, "h", ("fp32",), ("agg_scatter_kernel", 1)), (4095, 3, "h", ("fp32",), ("agg_scatter_kernel", 2)),
    (3265, 3, "h" * 10, ("fp32", "bf16"), ("agg_scatter_kernel", 16)),
    (4095, 3, "m", ("fp32", "bf16"), ("agg_scatter_mask_kernel", 2)), (3265, 3, "m" * 10, ("fp32", "bf16"), ("agg_scatter_mask_kernel", 16)),
]


def scatter_case_groups(N: int, spec: str) -> List[Dict]:
    """The `scatter_forms` groups of a SCATTER_GPU_CASES letter string."""
    kinds = dict(s=dict(E=pair_count(N), sym=True), o=dict(E=N * N), h=dict(E=N, H=True), m=dict(E=N, colmask=True))
    return [kinds[c] for c in spec]


PLACEHOLDER = 4096      # a 16-aligned non-NULL "device address": a plan query tests addresses, it never dereferences them


def launch_descriptors(B: int, N: int, scales: Sequence[int], precision: str = "f16x3", dtype: str = "fp32",
                       training: bool = False, block: bool = True, with_pair: bool = True,
                       types: Optional[Sequence[int]] = None, bottleneck: int = BOTTLENECK) -> Dict:
    """The C-ABI descriptor arrays the engine passes for the last round of such a forward (arguments as `expected_forms`),
    with the node-form, PoolSpec and closing decisions as `expected_forms` states them and PLACEHOLDER for every device
    address (tests/test_route_cpu.py holds `route.message_passing_route`, which the engine follows, against them).  -> {"twin", "edge": arr, "agg": arr (closing MLP in a launch of its own), "agg_closing": arr
    (the closing stage in the aggregation launch), "mlp2": (arr, rows, din, dh, dout, ldy, N, divisor), "n2e": arr or None,
    "gather": arr or None, "scatter": arr or None}; the group order is that of expected_forms' "groups".  bottleneck: the
    closing MLP's output width — its bf16-core images exist up to IMAGE_MAX_DOUT (weights.closing_mlp), and beyond it the
    engine passes none (ops.mlp2_grouped)."""
    from groupnet_amd import _lib as L
    P = PLACEHOLDER
    twin = dtype == "bf16"
    xm = twin or precision != "fp32"
    X = P if xm else 0                              # bf16-core images
    Hh = P if (precision == "f16x3" and not twin) else 0      # fp16 two-part images
    forms = expected_forms(B, N, scales, precision, dtype, training, block, with_pair, types, bottleneck)
    groups = forms["groups"]
    d = int(bottleneck)
    X2, H2 = (X, Hh) if d <= IMAGE_MAX_DOUT else (0, 0)      # the closing MLP's images
    n = len(groups)
    small = N <= FUSED_MAX_N
    pool = not training and xm                      # pooling in the edge kernel (PoolSpec), before the N limit of hyper groups
    edge, agg, aggc, mlp2, n2e, gather, scatter = [], [], [], [], [], [], []
    for g in groups:
        pair, E, K, rows = g["name"] == "pair", g["E"], g["K"], g["rows"]
        common = dict(bias=P, edge_feat=P, rows=rows, K=K, Wx=X, Wh=Hh, W=P, sym_N=N if pair else 0, dist=P)
        if pool and (pair or small):
            edge.append(L.EdgeGroup(xp=P, pq=P, w2=P, b2=P, pool_N=N, pool_H=0 if pair else P, pool_E=0 if pair else E,
                                    **common))
        else:
            edge.append(L.EdgeGroup(edges=P, **common))
            n2e.append(L.N2EGroup(xp=P, pq=P, H=0 if pair else P, w2=P, edges=P, b2=P, E=E, sym=int(pair)))
        base = dict(edge_feat=P, W=P, b1=P, b2=P, rows=rows, K=K)
        if pair and not twin:
            a = dict(E=E, N=N, sym=1, A=P, W2x=X, W2h=Hh, node_form=int(g["node_form"]))
        elif pair or small:
            a = dict(ori=P, H=0 if pair else P, E=E, N=N, sym=int(pair), W12x=X, W12h=Hh, node_form=int(g["node_form"]))
        else:
            a = dict(eo=P, W12x=X, W12h=Hh)
            gather.append(L.GatherGroup(ori=P, H=P, eo=P, E=E, sym=0))
        agg.append(L.AggGroup(feat=P, **base, **a))
        aggc.append(L.AggGroup(**base, **{**a, "ori": P}, m2x=X2, m2h=H2, m2bias=P, y=P, ldy=d * (1 + n) if block else d,
                               dout=d, divisor=float(N)))
        keep = dict(in_out=P, hid_out=P) if training else {}
        m = dict(W=P, bias=P, y=P, Wx=X2, Wh=H2, **keep)
        if g["node_form"]:
            mlp2.append(L.Mlp2Group(feat=P, ori=P, **m))                                   # NodeAggSpec
        elif small:
            mlp2.append(L.Mlp2Group(feat=P, H=0 if pair else P, ori=P, E=E, sym=int(pair), **m))   # ScatterSpec
        else:
            mlp2.append(L.Mlp2Group(x=P, **m))                                             # stand-alone scatter's output
            scatter.append(L.ScatterGroup(feat=P, H=0 if pair else P, ori=P, out=P, E=E, sym=int(pair)))
    arr = lambda cls, xs: (cls * len(xs))(*xs) if xs else None
    return dict(twin=twin, edge=arr(L.EdgeGroup, edge), agg=arr(L.AggGroup, agg), agg_closing=arr(L.AggGroup, aggc),
                mlp2=(arr(L.Mlp2Group, mlp2), B * N, 128, 128, d, d * (1 + n) if block else d, N, float(N)),
                n2e=arr(L.N2EGroup, n2e), gather=arr(L.GatherGroup, gather), scatter=arr(L.ScatterGroup, scatter))


def assert_plans_match(forms: Dict, agg, mlp2, n2e, gather, where, scatter=False) -> None:
    """The launchers' plans of one forward (groupnet_amd._lib.LaunchPlan of gn_agg_mlp_plan_*, and of gn_mlp2_plan_* /
    gn_node2edge_plan_* / gn_agg_gather_plan_* / gn_agg_scatter_plan_* or None where that launch does not run; scatter=False:
    the caller did not ask) say what `forms` says."""
    from groupnet_amd import _lib as L
    name = lambda plan: L.load().gn_kernel_name(plan.kernel).decode()
    groups = forms["groups"]
    n = len(groups)
    assert agg.n_groups == n and agg.closing == int(forms["fused_closing"]), where
    for i, g in enumerate(groups):
        assert (agg.wpr[i], agg.spw[i], bool(agg.node_form[i])) == (g["wpr"], g["spw"], g["node_form"]), (where, g)
    scene = [agg.pre_grid[i] for i in range(n) if agg.pre_grid[i]]
    assert scene == ([] if forms["scene_grid"] is None else [forms["scene_grid"]]), where
    assert (name(agg), sum(agg.wgs[i] for i in range(n)), agg.grid[0]) == (
        forms["agg_kernel"], forms["agg_wgs"], forms["agg_grid"]), where
    assert sorted(agg.pos[i] for i in range(n) if not agg.pre_grid[i]) == list(range(n - len(scene))), where
    assert [agg.pos[i] for i in range(n)] == forms["agg_pos"], (where, [agg.pos[i] for i in range(n)], forms["agg_pos"])
    assert (mlp2 is None) == (forms["mlp2"] is None) and (n2e is None) == (forms["n2e"] is None), where
    assert (gather is None) == (forms["gather_spw"] is None), where
    if mlp2 is not None:
        assert name(mlp2) == forms["mlp2"], (where, name(mlp2))
        assert forms.get("mlp2_tiles") is None or mlp2.tiles[2] == forms["mlp2_tiles"], (where, mlp2.tiles[2])
    if n2e is not None:
        assert ("rows" if n2e.variant else "banded") == forms["n2e"] and (n2e.EBh == 0) == bool(n2e.variant), where
    if gather is not None:
        assert gather.G == forms["gather_spw"], (where, gather.G)
    if scatter is not False:
        assert (scatter is None) == (forms["scatter"] is None), where
        if scatter is not None:
            assert_scatter_plan(forms["scatter"], scatter, where)


def describe(forms: Dict) -> str:
    g = ", ".join(f"{x['name']}:{'node' if x['node_form'] else 'wpr%d' % x['wpr']}{'/spw%d' % x['spw'] if x['spw'] else ''}"
                  for x in forms["groups"])
    return (f"[{g}] {'fused' if forms['fused_closing'] else 'unfused'} closing, {forms['agg_kernel']} grid "
            f"{forms['agg_grid']}, scene form grid {forms['scene_grid']}, mlp2 {forms['mlp2']}, n2e {forms['n2e']}, gather G {forms['gather_spw']}")


# ---------------------------------------------------------------------------------------------------------------------
# scene sampler
# ---------------------------------------------------------------------------------------------------------------------
def _spread(cands: Sequence[int], k: int) -> List[int]:
    """k members of the sorted candidate list, evenly spread from its first to its last."""
    c = sorted(set(cands))
    if len(c) <= k:
        return c
    return [c[round(i * (len(c) - 1) / (k - 1))] for i in range(k)] if k > 1 else [c[0]]


def _straddling(B: int, rows_per_scene: int, block: int) -> List[int]:
    """Scenes whose rows [b*r, (b+1)*r) cross a multiple of `block` rows, or start / end one."""
    out = []
    r = rows_per_scene
    for b in range(B):
        lo, hi = b * r, (b + 1) * r - 1
        if lo // block != hi // block or lo % block == 0 or (hi + 1) % block == 0:
            out.append(b)
    return out


def sample_scenes(B: int, N: int, forms: Dict, n: int = 48, seed: int = 0, per_rule: int = 4) -> torch.Tensor:
    """Sorted scene indices (int64): the first and last scene; per rule `per_rule` scenes spread over the batch that
    straddle a 32-row block of every group's rows (edge rows and node rows), a workgroup of the selected form (128/wpr
    edge rows, or `spw` whole scenes), and a seeded random remainder up to n."""
    if B <= n:
        return torch.arange(B)
    pick = {0, B - 1}
    rules = [_straddling(B, N, 32)]                              # node rows: node stage, closing MLP
    for g in forms["groups"]:
        rules.append(_straddling(B, g["E"], 32))                  # the group's 32-row blocks
        if g["spw"]:
            rules.append([b for b in range(B) if b % g["spw"] in (0, g["spw"] - 1)])
        elif not g["node_form"]:
            rules.append(_straddling(B, g["E"], 128 // g["wpr"]))   # one workgroup's row blocks
    for c in rules:
        pick.update(_spread(c, per_rule))
    rest = [b for b in range(B) if b not in pick]
    gen = torch.Generator().manual_seed(seed)
    need = max(0, n - len(pick))
    if need:
        pick.update(rest[i] for i in torch.randperm(len(rest), generator=gen)[:need].tolist())
    return torch.tensor(sorted(pick), dtype=torch.long)


# ---------------------------------------------------------------------------------------------------------------------
# float64 oracle on sampled scenes
# ---------------------------------------------------------------------------------------------------------------------
def state64(state: Dict[str, torch.Tensor], requires_grad: bool = False) -> Dict[str, torch.Tensor]:
    return {k: v.detach().double().requires_grad_(requires_grad) for k, v in state.items()}


def _noise(U, scenes):
    return [u[scenes].double() for u in (U if isinstance(U, (list, tuple)) else [U])]


def _chunks(m: int, chunk: Optional[int]):
    step = m if not chunk else chunk
    return [slice(i, min(m, i + step)) for i in range(0, m, step)]


def pairwise64(state, h, U, scenes, nmp: int = 1, chunk: Optional[int] = None):
    """Pairwise module (MS_HGNN_oridinary.forward) in float64 on h[scenes] -> (node_feat, factors) of those scenes.
    `state` may be a float64 state (e.g. leaves that require grad); chunk: scenes per oracle call (memory at large N)."""
    st = state if all(v.dtype == torch.float64 for v in state.values()) else state64(state)
    hs, Us = h[scenes].double(), _noise(U, scenes)
    nf, fac = [], []
    for c in _chunks(len(scenes), chunk):
        a, b = O.ms_hgnn_pairwise_forward(st, hs[c], [u[c] for u in Us], nmp, decomposed=True)
        nf.append(a)
        fac.append(b)
    return torch.cat(nf), torch.cat(fac)


def hyper_incidence(h, scenes, scale: int) -> torch.Tensor:
    """H of the sampled scenes from the fp32 affinity, lowest index winning ties (the HIP kernel's rule)."""
    return O.topk_incidence_ranked(O.affinity(h[scenes].float()), scale)


def hyper64(state, h, H, U, scenes, nmp: int = 1, chunk: Optional[int] = None):
    """Hyper module (MS_HGNN_hyper.forward) in float64 on h[scenes] with the incidence H of those scenes (as given:
    (len(scenes), E, N)) -> (node_feat, factors)."""
    st = state if all(v.dtype == torch.float64 for v in state.values()) else state64(state)
    hs, Us, Hd = h[scenes].double(), _noise(U, scenes), H.double()
    nf, fac = [], []
    for c in _chunks(len(scenes), chunk):
        a, b = O._message_passing(st, hs[c], Hd[c], [u[c] for u in Us], nmp, True, None)
        nf.append(a)
        fac.append(b)
    return torch.cat(nf), torch.cat(fac)


def clean_scenes(state_pair, states_hyper, scales, h, Hs, U_pair, U_hyper, scenes, with_pair: bool = True,
                 chunk: int = 16) -> torch.Tensor:
    """(len(scenes),) bool: the scenes none of whose oracle ReLU inputs lies within relu_probe.WINDOW of zero.
    The probe counts only ReLU inputs whose batch is its own, so every chunk of scenes gets one probe of its own and one
    unchunked oracle call.  Hs: per scale the incidence of `scenes` (or None)."""
    from relu_probe import relu_probe
    out = []
    for c in _chunks(len(scenes), chunk):
        with torch.no_grad(), relu_probe(c.stop - c.start) as probe:
            block64(state_pair, states_hyper, scales, h, None if Hs is None else [H[c] for H in Hs], U_pair, U_hyper,
                    scenes[c], with_pair=with_pair)
        assert probe.units > 0, "the probe saw no ReLU input"
        out.append(probe.clean())
    return torch.cat(out)


def block64(state_pair, states_hyper, scales, h, Hs, U_pair, U_hyper, scenes, nmp: int = 1,
            chunk: Optional[int] = None, with_pair: bool = True, with_hyper: bool = True):
    """Multiscale block (PastEncoder.forward around the path) in float64 on h[scenes]: cat(f, pairwise, hyper_s...) and
    the factors of every module.  Hs: per scale the incidence of the sampled scenes (None: built here from the fp32
    affinity).  with_pair=False / with_hyper=False leave the pairwise / hyper columns zero and their factors None (a
    loss that does not read them)."""
    hs = h[scenes].double()
    feats, facs = [hs], []
    if with_pair:
        nf, fac = pairwise64(state_pair, h, U_pair, scenes, nmp, chunk)
    else:
        nf, fac = torch.zeros_like(hs), None
    feats.append(nf)
    facs.append(fac)
    for i, (st, s) in enumerate(zip(states_hyper, scales)):
        if not with_hyper:
            feats.append(torch.zeros_like(hs))
            facs.append(None)
            continue
        H = hyper_incidence(h, scenes, s) if Hs is None or Hs[i] is None else Hs[i]
        nf, fac = hyper64(st, h, H, U_hyper[i], scenes, nmp, chunk)
        feats.append(nf)
        facs.append(fac)
    return torch.cat(feats, dim=-1), facs


# ---------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_launch_forms_gpu.py (shared with the CPU test that checks they reach every form)
# ---------------------------------------------------------------------------------------------------------------------
def _case(kind, B, N, scales, precision="f16x3", dtype="fp32"):
    return dict(id=f"{kind}-B{B}-N{N}-s{'.'.join(map(str, scales))}-{precision if dtype == 'fp32' else dtype}",
                kind=kind, B=B, N=N, scales=list(scales), precision=precision, dtype=dtype)


FORWARD_CASES = (
    # N = 11, scales {2,5,11}: E = 11 switches wpr 4 -> 2 at B = 370 and 2 -> 1 (closing unfused) at B = 2232; B = 64 is
    # the anchor (the forms the small-size tests already trust); B = 512 packs 5 scenes per workgroup
    [_case("block", B, 11, [2, 5, 11], p) for p in ("f16x3", "bf16x6", "fp32")
     for B in (64, 369, 370, 512, 2231, 2232, 4096)]
    # one scale = N module (E = 1): wpr 4 -> 2 at B = 4065, 2 -> 1 at B = 24545
    + [_case("hyper", B, 11, [11]) for B in (4064, 4065, 24576)]
    # the N <= 16 limit of the fused gather / scatter / pooling / closing stage; N = 17 at B = 2736 packs 4 scenes per
    # gather workgroup and takes the row form of node -> edge
    + [_case("block", 512, 16, [2, 5, 16]), _case("block", 512, 17, [2, 5, 17]), _case("block", 2736, 17, [2, 5, 17])]
    # bf16 storage: config 4, and the twins' scene form of the pairwise aggregation on both sides of N = 64
    + [_case("block", 1024, 50, [2, 4, 8, 16], dtype="bf16"), _case("block", 256, 64, [2, 16, 64], dtype="bf16"),
       _case("block", 256, 65, [2, 16, 65], dtype="bf16")]
)

# training forward + backward of the block (fp32): node -> edge banded (B = 512) and row form (B = 2232, config 4 at its
# own batch, B = 1024: at N = 50 only ~4 % of the scenes are clean in the hyper modules, so the clean scenes are drawn
# from the whole batch)
BACKWARD_CASES = [_case("train", 512, 11, [2, 5, 11]), _case("train", 2232, 11, [2, 5, 11]),
                  _case("train", 1024, 50, [2, 4, 8, 16])]


def case_forms(case: Dict) -> Dict:
    return expected_forms(case["B"], case["N"], case["scales"], case["precision"], case["dtype"],
                          training=case["kind"] == "train", block=case["kind"] != "hyper",
                          with_pair=case["kind"] != "hyper")
