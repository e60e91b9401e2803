"""Test helper: the cases and batch builders of the scene-isolation tests (tests/test_scene_isolation_cpu.py checks this
table and the oracle, tests/test_scene_isolation_gpu.py runs it).  Pure torch on the CPU; the library is never loaded.

The property.  With batch_norm = 0 a scene's output is a function of that scene alone — its features, its noise, the
weights.  The kernels pack rows of several scenes into one workgroup (32-row blocks of the B*N node rows and of the
B*E edge rows, several whole scenes in the node form's LDS stage and in the fused closing stage, several scenes per
gather / scatter workgroup) and take some decisions per workgroup (the f16x3 range vote, the node form's clamp scale,
the weight-image flag), so the property has to be observed, not assumed: every case here is the smallest shape that
still puts several scenes into one workgroup of its route, with a ragged last block.

A batch is a vector of per-scene magnitudes applied to ONE set of N(0,1) scenes and per-scene uniforms, so the same
scene (same data, same noise) appears in several batches beside different neighbours, and can be permuted and subset
with its noise.
"""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import torch

# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
# what a case's id names, in the terms of groupnet_amd.route: per module kind (source, closing_input, pooled in the edge
# kernel), the kinds of module that share the node2edge / gather / scatter launch, masks, closing asked
_SMALL = dict(pair=("pair-node", "node-agg", True), hyper=("fused-gather", "scatter-spec", True),
              node2edge="", gather="", scatter="", masks=False, ask_closing=True)
_SMALL_FP32 = dict(pair=("pair", "scatter-spec", False), hyper=("fused-gather", "scatter-spec", False),
                   node2edge="ph", gather="", scatter="", masks=False, ask_closing=True)
_LARGE = dict(pair=("pair", "scatter", True), hyper=("eo", "scatter", False),
              node2edge="h", gather="h", scatter="ph", masks=False, ask_closing=False)
_LARGE_MASK = dict(_LARGE, masks=True)
_TWIN_SCENE = dict(pair=("scene", "node-agg", True), hyper=("eo", "scatter", False),
                   node2edge="h", gather="h", scatter="h", masks=False, ask_closing=False)
_TWIN_PAIR = dict(pair=("twin-pair", "scatter", True), hyper=("eo", "scatter", False),
                  node2edge="h", gather="h", scatter="ph", masks=False, ask_closing=False)


def _case(id, B, N, scales, route, precision="f16x3", dtype="fp32", nmp=1, incidence="dense", seed=0):
    return dict(id=id, B=B, N=N, scales=list(scales), precision=precision, dtype=dtype, nmp=nmp, incidence=incidence,
                route=route, seed=seed)


CASES = [
    # 77 node rows: 3 blocks, the last of 13 rows, every block boundary inside a scene; node form, pooled edge kernel,
    # fused closing stage (fp32 cores: the pair form, the node2edge launch, the closing launch)
    _case("n11-f16x3", 7, 11, [2, 5, 11], _SMALL, seed=21),
    _case("n11-bf16x6", 7, 11, [2, 5, 11], _SMALL, precision="bf16x6", seed=21),
    _case("n11-fp32", 7, 11, [2, 5, 11], _SMALL_FP32, precision="fp32", seed=21),
    # the second round reads the first round's output
    _case("n11-nmp2", 7, 11, [2, 5], _SMALL, nmp=2, seed=12),
    # 16 scenes per row block, E = 1
    _case("n2", 9, 2, [2], _SMALL, seed=2),
    # both sides of the fused gather / scatter / pool limit; N = 17 in both incidence forms
    _case("n16", 5, 16, [2, 5, 16], _SMALL, seed=16),
    _case("n17-dense", 5, 17, [2, 5, 17], _LARGE, seed=19),
    _case("n17-mask", 5, 17, [2, 5, 17], _LARGE_MASK, incidence="mask", seed=19),
    # the pair form beyond the node form, and the twins' scene form
    _case("n50-f16x3", 3, 50, [2, 4, 8, 16], _LARGE, seed=53),
    _case("n50-bf16", 3, 50, [2, 4, 8, 16], _TWIN_SCENE, dtype="bf16", seed=50),
    # the twins' per-pair gather, beyond the scene form and the mask range
    _case("n65-bf16", 3, 65, [2, 16, 65], _TWIN_PAIR, dtype="bf16", seed=65),
]
CASE_IDS = [c["id"] for c in CASES]

# training forward + backward in a mixed batch: finite magnitudes only (`seed`: chosen on the CPU for the clean scenes
# the backward gate needs, tests/test_scene_isolation_cpu.py)
TRAIN_CYCLE = (1.0, 3e3, 1.0, 30.0, 1.0)
TRAIN_CASES = [dict(_case("train-n11", 7, 11, [2, 5, 11], None, seed=111), min_clean=3),
               dict(_case("train-n50", 3, 50, [2, 4, 8, 16], None, seed=185), min_clean=1)]

K_PAIR, K_HYPER = 6, 10


def n_edges(N: int, s: int) -> int:
    return 1 if s == N else N


# ---------------------------------------------------------------------------------------------------------------------
# magnitudes
# ---------------------------------------------------------------------------------------------------------------------
MIXED_CYCLE = (1.0, 1e6, 1.0, 0.0, 3e3, 1.0, 1e12)      # 1e6, 1e12: the range vote; 3e3: fits as input, hidden rows do not
OVERFLOW = 1e24                                          # M > 2^72: the max form; inf / NaN inside that scene
NAN, INF = float("nan"), float("inf")                    # an all-NaN scene; a scene with one +inf and one -inf entry
MIXED_CLASSES = ("ordinary", "zero", "3e3", "1e6", "1e12")


def klass(m: float) -> str:
    if math.isnan(m):
        return "nan"
    if math.isinf(m):
        return "inf"
    if m >= OVERFLOW:
        return "overflow"
    return {0.0: "zero", 1.0: "ordinary", 3e3: "3e3", 1e6: "1e6", 1e12: "1e12", 30.0: "30"}[m]


def is_checked(m: float) -> bool:
    """A scene whose own result is asserted: finite and not overflowing."""
    return math.isfinite(m) and m < OVERFLOW


def is_ordinary(m: float) -> bool:
    """N(0,1) data or all zeros: gated at the ordinary tolerances, and never the reason for a workgroup's fallback."""
    return m in (0.0, 1.0)


def checked(mags: Sequence[float]) -> List[int]:
    return [b for b, m in enumerate(mags) if is_checked(m)]


def mixed_offsets(B: int) -> List[int]:
    """Where in MIXED_CYCLE a case's mixed batches start.  A batch of B >= 7 scenes holds the whole cycle; a smaller
    one cannot, so the case runs as many mixed batches as it takes to meet every class, each starting on the previous
    one's last scene (an ordinary or a large scene, so every batch keeps both kinds)."""
    offs, seen, o = [], set(), 0
    while not seen >= set(MIXED_CLASSES):
        offs.append(o)
        seen |= {klass(MIXED_CYCLE[(o + b) % len(MIXED_CYCLE)]) for b in range(B)}
        o += B - 1
    return offs


def poison_positions(B: int) -> Tuple[Tuple[int, ...], Tuple[int, int]]:
    """(the overflowing scenes, (the NaN scene, the inf scene)): at least B - 2 scenes of a poisoned batch are checked, and
    among them one that lies across an inner row-block edge of every group (`straddle_gaps`): at B = 5 that is scene 3
    (N = 17: rows 51..67; N = 16: ends at row 64), at B = 7 the scenes 2 and 5, at B = 9 scene 8."""
    return ((1, 4) if B >= 7 else (1,)), (1, 3 if B > 5 else 2)


def across_an_inner_edge(B: int, r: int, block: int = 32) -> List[int]:
    """The scenes of B x r rows that share a `block`-row block with a neighbour at an inner block edge: their rows cross
    a multiple of `block`; or, where r divides the block (so no scene crosses), a scene b > 0 that starts or ends on a
    multiple of `block` inside the rows.  Scene 0 merely starting row 0 does not count."""
    out = []
    for b in range(B):
        lo, hi = b * r, (b + 1) * r - 1
        if lo // block != hi // block:
            out.append(b)
        elif block % r == 0 and b > 0 and ((lo % block == 0) or ((hi + 1) % block == 0 and hi + 1 < B * r)):
            out.append(b)
    return out


def straddle_gaps(case: Dict, many: Dict[str, List[float]], row_counts: Sequence[Tuple[str, int]]) -> List[tuple]:
    """(batch, rows) of every batch in which no checked scene lies across an inner block edge of one of `row_counts`
    ((name, rows per scene): the node rows and every group's edge rows); rows that fit one block are left out."""
    B, gaps = case["B"], []
    for name, mags in many.items():
        cs = set(checked(mags))
        for what, r in row_counts:
            if B * r > 32 and not cs & set(across_an_inner_edge(B, r)):
                gaps.append((name, what))
    return gaps


def batches(B: int) -> Dict[str, List[float]]:
    """Every batch of a case, as per-scene magnitudes: all ordinary, the mixed batches, the first mixed batch with
    overflowing neighbours, and with non-finite neighbours."""
    out = {"ordinary": [1.0] * B}
    for o in mixed_offsets(B):
        out[f"mixed{o}"] = [MIXED_CYCLE[(o + b) % len(MIXED_CYCLE)] for b in range(B)]
    over, (nan, inf) = poison_positions(B)
    out["overflow"] = [OVERFLOW if b in over else m for b, m in enumerate(out["mixed0"])]
    out["nonfinite"] = [NAN if b == nan else INF if b == inf else m for b, m in enumerate(out["mixed0"])]
    return out


def zero_neighbour_batches(B: int) -> Dict[str, List[float]]:
    """Every second scene ordinary, the others all-zero, and the complement: beside zeros nothing votes."""
    return {"zeros-odd": [1.0 if b % 2 == 0 else 0.0 for b in range(B)],
            "zeros-even": [1.0 if b % 2 == 1 else 0.0 for b in range(B)]}


def train_mags(B: int) -> List[float]:
    return [TRAIN_CYCLE[b % len(TRAIN_CYCLE)] for b in range(B)]


# ---------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------
def base_inputs(case: Dict):
    """(h0 (B, N, 64) N(0,1) scenes — bf16-representable for bf16 storage —, U: per module, pairwise first, the list of
    its `nmp` uniform tensors (B, E, K)), all per scene: row b belongs to scene b alone."""
    B, N = case["B"], case["N"]
    gen = torch.Generator().manual_seed(1000 + case["seed"])
    h0 = torch.randn(B, N, 64, generator=gen)
    if case["dtype"] == "bf16":
        h0 = h0.bfloat16().float()
    shapes = [(B, N * N, K_PAIR)] + [(B, n_edges(N, s), K_HYPER) for s in case["scales"]]
    U = [[torch.rand(shp, generator=gen) for _ in range(case["nmp"])] for shp in shapes]
    return h0, U


def cpu_block(case: Dict):
    """(the case's MultiScaleHGNN on the CPU, the pairwise module's state, the hyper modules' states) — the weights of
    test_bf16_gpu.block_and_states(scales, seed), for any number of rounds and without a device."""
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(case["seed"])
    blk = MultiScaleHGNN(case["scales"], nmp_layers=case["nmp"])
    sp = {k: v.detach().clone() for k, v in blk.interaction.state_dict().items()}
    shs = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in blk.interaction_hyper]
    return blk, sp, shs


def scaled(case: Dict, h0: torch.Tensor, mags: Sequence[float]) -> torch.Tensor:
    """The batch of `mags`: scene b is h0[b] times its magnitude; all zeros; all NaN; or h0[b] with one +inf and one
    -inf entry."""
    N = h0.shape[1]
    h = h0.clone()
    for b, m in enumerate(mags):
        if math.isnan(m):
            h[b] = NAN
        elif math.isinf(m):
            h[b, N // 2, 3] = INF
            h[b, N - 1, 40] = -INF
        elif m == 0.0:
            h[b] = 0.0
        elif m != 1.0:
            h[b] = h0[b] * m
    if case["dtype"] == "bf16":
        h = h.bfloat16().float()
    return h


def oracle32(sp, shs, h: torch.Tensor, Hs, U, b: int, nmp: int = 1):
    """The fp32 oracle of scene b alone on the incidences Hs (per scale, (1, E, N)) -> (node features, factors), each per
    module, pairwise first: what fp32 rounding alone does to the float64 oracle of that scene."""
    from oracle import ms_hgnn_oracle as O
    one = torch.tensor([b])
    hb = h[one].float()
    res = [O.ms_hgnn_pairwise_forward(sp, hb, [u[one] for u in U[0]], nmp, decomposed=True)]
    res += [O._message_passing(st, hb, H.float(), [u[one] for u in us], nmp, True, None) for st, H, us in zip(shs, Hs, U[1:])]
    return [r[0] for r in res], [r[1] for r in res]


# A large scene is gated at 2e-5 of its own max|ref| against the FLOAT64 oracle.  Its Gumbel softmax is saturated (logits
# of 1e3 .. 1e12 over tau = 0.5), so an edge whose two best types are closer than the fp32 rounding of such a logit picks
# another type in ANY fp32 evaluation, the fp32 oracle included (measured: 7e-4 of max|ref| on such a scene, 3e-7 .. 1e-5
# otherwise).  The seeds are chosen so that no large scene is that ill-conditioned: the fp32 oracle alone stays within
# half the gate, which leaves the other half to the implementation's own fp32 rounding.
LARGE_CONDITION = 0.5
TOL_LARGE = 2e-5      # of the scene's own max|ref| (test_f16x3_range_vote_falls_back_to_bf16x6)


def case_route(case: Dict):
    """`route.message_passing_route` of the case's eval block with the engine's knobs as the engine reads them."""
    from groupnet_amd import MS_HGNN_batch as M, ops, route as R
    mods = [(True, K_PAIR)] + [(False, K_HYPER)] * len(case["scales"])
    knobs = R.Knobs(M._FUSE_POOL, ops.POOL_MAX_N, ops.node_form_enabled(), case["incidence"] == "mask")
    return R.message_passing_route(case["N"], tuple(mods), twin=case["dtype"] == "bf16", training=False,
                                   matrix16=case["precision"] != "fp32", knobs=knobs, closing_asked=True)


# Large scenes on bf16 storage.  bf16 keeps 8 significant bits (u = 2^-9): a pre-softmax logit carries a few u of the
# largest magnitude in its chain, and through exp(. / tau), tau = 0.5, a scene whose logits are of magnitude 1e3 .. 1e12
# has edges whose sampled type the format does not determine (measured 7e-2 .. 6e-1 of max|ref| from the oracle).  Such a
# scene is therefore gated in the two parts the format does determine:
#   * the edge head on the DETERMINED edges — the float64 winner of y = logits + gumbel leads the runner-up by more than
#     4 e_emu + 8, e_emu = max|y_emu - y| over the module's edges of that scene for a CPU restatement of the chain with
#     weights and every layer's operands rounded to bf16 (`head_y16`; 4 e_emu is the slack the twins' other gates take;
#     a remaining lead of 8 = 2 tau ln(K / TOL_ORACLE), rounded up, puts 1 - TOL_ORACLE on the winner), and by no less
#     than TWIN_GAP x max|y|: there the twin puts at least 1 - TOL_ORACLE on the same type;
#   * everything behind the edge head, GIVEN the twin's own edge features fac x dist: typed aggregation, scatter and
#     closing MLP of the float64 oracle on them, at the twins' gate TOL_ORACLE of max|ref| (a wrong fallback, scale or
#     type weight shows here whatever the edge head sampled).
TWIN_GAP = 2.0 ** -5


def ordered_edge_feat(ef: torch.Tensor, N: int) -> torch.Tensor:
    """The pairwise module's edge features per unordered pair as the edge kernel writes them — (1, N(N+1)/2, K), rows
    (i, j >= i) row-major, fac (dist_ij + dist_ji) and, with the self-loop's incidence weight 2 folded in, 2 fac dist_ii —
    as ordered-edge features (1, N*N, K) with the same aggregate under the oracle's incidence: the pair's row on edge
    (i, j), zero on (j, i) (both ordered edges meet the same typed MLP output and the same two nodes), half the row on
    a self-loop (whose incidence weight the oracle applies itself)."""
    ii, jj = torch.triu_indices(N, N)
    out = torch.zeros(ef.shape[0], N * N, ef.shape[-1], dtype=ef.dtype)
    out[:, ii * N + jj] = ef * torch.where(ii == jj, 0.5, 1.0).to(ef.dtype)[None, :, None]
    return out


def head_y16(st, h, H, U, b: int):
    """y = logits + gumbel of scene b's edge head as `head_and_tail64` forms it, restated in fp32 with the weights and
    every layer's operands rounded to bf16 (node MLP, pooling, edge MLP): what the storage format alone does to y."""
    from oracle import ms_hgnn_oracle as O
    r16 = lambda t: t.bfloat16().float()
    s16 = {k: (r16(v.float()) if k.endswith("weight") else v.float()) for k, v in st.items()}
    one = torch.tensor([b])
    hb = r16(h[one].float())
    Hf = O.pairwise_incidence(h.shape[1], 1, torch.float32) if H is None else H.float()
    real = O.mlp

    def mlp16(state, prefix, x):
        n = 0
        while f"{prefix}.layers.{n}.weight" in state:
            n += 1
        for i in range(n):
            x = torch.nn.functional.linear(r16(x), state[f"{prefix}.layers.{i}.weight"], state[f"{prefix}.layers.{i}.bias"])
            if i != n - 1:
                x = torch.relu(x)
        return x
    O.mlp = mlp16
    try:
        edges, _ = O.node2edge(s16, hb, Hf, 0, True)
        y = mlp16(s16, "nmp_mlp_start.MLP_distribution", mlp16(s16, "nmp_mlp_start.init_MLP", edges))
    finally:
        O.mlp = real
    u = U[0][one].float()
    return (y - torch.log(O.GUMBEL_EPS - torch.log(u + O.GUMBEL_EPS))).double()


def determined_edges(y: torch.Tensor, y16: torch.Tensor):
    """((1, E) bool: the edges whose float64 winner the bf16 format cannot change, (1, E) the winner, e_emu)."""
    e_emu = float((y16 - y).abs().max())
    top = y.topk(2, dim=-1)
    lead = top.values[..., 0] - top.values[..., 1]
    return lead > max(4.0 * e_emu + 8.0, TWIN_GAP * float(y.abs().max())), top.indices[..., :1], e_emu


def head_and_tail64(st, h, H, U, ef, b: int):
    """Scene b of one module in float64 (one round): y = logits + gumbel of its edge head (1, E, K), and the node
    features the rest of the module gives on the edge features `ef` (1, E, K).  H: (1, E, N), or None for the pairwise
    graph (`ef` ordered)."""
    from launch_forms import state64
    from oracle import ms_hgnn_oracle as O
    s64, one = state64(st), torch.tensor([b])
    hb = h[one].double()
    Hd = O.pairwise_incidence(h.shape[1], 1, torch.float64) if H is None else H.double()
    edges, _ = O.node2edge(s64, hb, Hd, 0, True)
    z = O.mlp(s64, "nmp_mlp_start.init_MLP", edges)
    u = U[0][one].double()
    y = O.mlp(s64, "nmp_mlp_start.MLP_distribution", z) - torch.log(O.GUMBEL_EPS - torch.log(u + O.GUMBEL_EPS))
    nf = O.mlp(s64, "nmp_mlp_end", O.edge2node(s64, ef.double(), hb, Hd, 0))
    return y, nf


def train_clean_scenes(case: Dict) -> torch.Tensor:
    """The ordinary scenes of a training case's batch none of whose oracle ReLU inputs lies within relu_probe.WINDOW of
    zero — over the whole block up to N = 16, over the hyper modules beyond (a pairwise module of N = 50 has ~7 M ReLU
    units per scene and is never clean: tests/test_launch_forms_gpu.py)."""
    from launch_forms import clean_scenes, hyper_incidence
    _, sp, shs = cpu_block(case)
    h0, U = base_inputs(case)
    mags = train_mags(case["B"])
    f = scaled(case, h0, mags)
    ordinary = torch.tensor([b for b, m in enumerate(mags) if m == 1.0])
    Hs = [hyper_incidence(f, ordinary, s) for s in case["scales"]]
    keep = clean_scenes(sp, shs, case["scales"], f, Hs, U[0], U[1:], ordinary, with_pair=case["N"] <= 16)
    return ordinary[keep]


def derangement(B: int, seed: int) -> torch.Tensor:
    """A seeded permutation of the scenes without a fixed point."""
    gen = torch.Generator().manual_seed(seed)
    while True:
        p = torch.randperm(B, generator=gen)
        if not bool((p == torch.arange(B)).any()):
            return p


def take(U, idx: torch.Tensor):
    """The noise of the scenes `idx`, in that order."""
    return [[u[idx].contiguous() for u in us] for us in U]


# ---------------------------------------------------------------------------------------------------------------------
# gates shared with tests/test_parity_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
def prob_gate(got, ref32, ref64, slack):
    """Probabilities against the FLOAT64 oracle: within slack x max(1e-4, 3 x the fp32 oracle's own distance from it)
    (test_modules_under_extreme_magnitudes states why: a logit of magnitude 10^3 carries 1e-4 of fp32 rounding, which the
    exponential turns into that much probability)."""
    own = float((ref32.double() - ref64).abs().max())               # what fp32 rounding alone does to the oracle
    err = float((got.detach().cpu().double() - ref64).abs().max())
    print(f"probabilities: HIP vs float64 oracle {err:.2e}, fp32 oracle vs float64 {own:.2e}")
    return err <= slack * max(1e-4, 3.0 * own)
