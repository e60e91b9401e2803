"""Test helper: the number of edge types K as a dimension of the hot path (no GPU needed to import).

The reference fixes K = 6 (pairwise) and K = 10 (hyper); the kernels take 1..15 (edge head) and 1..16 (typed
aggregation) and branch on K in many places (waves per row block, the fused closing stage, the node form's K <= 12, the
weight-ring prefetch, features 8..15 of the edge head, the Philox routes, the factor head's row K of a 16-row tile, the
backward's padding to a multiple of 4).  This module holds what the tests of K share:

  * `with_edge_types(cls, K)`: the product's modules at another K (constructor signatures stay the reference's);
  * the K tables;
  * inputs drawn on the CPU from seeds of their own, and float64 references built on oracle.ms_hgnn_oracle — every
    reference takes `dtype`, so tests/test_edge_types_cpu.py can hold the fp32 oracle on the SAME inputs against the
    float64 one (it must stay within a third of every gate);
  * the launcher's rules for one aggregation launch of one group, restated through launch_forms.agg_wpr.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from launch_forms import agg_wpr, cdiv, pair_count
from oracle import ms_hgnn_oracle as O

K_ALL = tuple(range(1, 16))                      # the edge head: the factor head takes row K of the 16-row tile
K_AGG = tuple(range(1, 17))                      # the typed aggregation: GN_MAX_TYPES
K_EDGES = (1, 2, 3, 4, 5, 8, 9, 12, 13, 15)      # the branch points, for the larger matrices
K_AGG_EDGES = K_EDGES + (16,)                    # ... of the aggregation stage alone


@functools.lru_cache(maxsize=None)
def with_edge_types(cls, K: int):
    """`cls` (MS_HGNN_oridinary or MS_HGNN_hyper) with K edge types: `_build` sees edge_types = K."""
    class Typed(cls):
        def _build(self, *args, **kwargs):
            self.edge_types = K
            super()._build(*args, **kwargs)
    Typed.__name__ = Typed.__qualname__ = f"{cls.__name__}_K{K}"
    return Typed


def pair_module(K: int, seed: int, nmp: int = 1):
    import groupnet_amd as G
    torch.manual_seed(seed)
    return with_edge_types(G.MS_HGNN_oridinary, K)(embedding_dim=16, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0,
                                                   nmp_layers=nmp)


def hyper_module(K: int, scale: int, seed: int, nmp: int = 1):
    import groupnet_amd as G
    torch.manual_seed(seed)
    return with_edge_types(G.MS_HGNN_hyper, K)(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0,
                                               nmp_layers=nmp, scale=scale)


def state_of(module, prefix: str = "") -> Dict[str, torch.Tensor]:
    """CPU copy of a module's state dict, keys behind `prefix.` where given."""
    p = prefix + "." if prefix else ""
    return {p + k: v.detach().cpu().clone() for k, v in module.state_dict().items()}


def cast(state: Dict[str, torch.Tensor], dtype) -> Dict[str, torch.Tensor]:
    return {k: v.to(dtype) for k, v in state.items()}


def _gen(*key: int) -> torch.Generator:
    seed = 0
    for k in key:
        seed = seed * 1009 + int(k)
    return torch.Generator().manual_seed(seed)


def pair_index(N: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(i, j) of the unordered pair rows in gn_pair_decode order ((i, j >= i), row-major), and per ordered edge
    e = i * N + j the pair row that holds it."""
    ii, jj = torch.triu_indices(N, N)
    row = torch.empty(N, N, dtype=torch.long)
    row[ii, jj] = torch.arange(ii.numel())
    row[jj, ii] = torch.arange(ii.numel())
    return ii, jj, row.reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the edge head (MLP_dict_softmax: gn_edge_mlp_gumbel_*)
# ---------------------------------------------------------------------------------------------------------------------
# (id, B, rows per scene, sym_N): 69 rows = two full 32-row blocks and a ragged one; the pairwise unordered form at
# N = 5, 15 pair rows and 25 ordered dist rows per scene
EDGE_SHAPES = (("rows", 3, 23, 0), ("sym5", 3, 15, 5))


def edge_head(K: int):
    """The module tests/test_device_noise_gpu.py runs at K (seed 100 + K), on the CPU."""
    from groupnet_amd.MS_HGNN_batch import MLP_dict_softmax
    torch.manual_seed(100 + K)
    return MLP_dict_softmax(64, 64, (128,), edge_types=K)


def edge_inputs(K: int, shape: Tuple[str, int, int, int], bf16: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(edges (B,E,64) fp32 — bf16-representable for the twins —, U (B, ordered edges, K)) of an EDGE_SHAPES entry."""
    _, B, E, sym_N = shape
    g = _gen(1, K, E)
    edges = torch.randn(B, E, 64, generator=g)
    U = torch.rand(B, sym_N * sym_N if sym_N else E, K, generator=g)
    return (edges.bfloat16().float() if bf16 else edges), U


def edge_ref(state: Dict[str, torch.Tensor], edges: torch.Tensor, U: torch.Tensor, sym_N: int = 0, dtype=torch.float64
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(factor * dist, dist) of O.edge_mlp_gumbel on `state` (keys behind "head.") in `dtype`.  sym_N: `edges` holds the
    unordered pair rows; dist is that of the N * N ordered edges, the first output fac * (dist_ij + dist_ji) per pair row
    (twice the self-loop's: its incidence weight 2)."""
    st, e, u = cast(state, dtype), edges.to(dtype), U.to(dtype)
    if not sym_N:
        return O.edge_mlp_gumbel(st, "head", e, u)
    ii, jj, row = pair_index(sym_N)
    fd, dist = O.edge_mlp_gumbel(st, "head", e[:, row], u)
    return fd[:, ii * sym_N + jj] + fd[:, jj * sym_N + ii], dist


# ---------------------------------------------------------------------------------------------------------------------
# 2. the typed aggregation stage (edge_aggregation: gn_agg_mlp_*)
# ---------------------------------------------------------------------------------------------------------------------
# One launch of one group each.  form: "eo" (a tensor), "gather" (GatherSpec with a top-k H), "pair" (PairSpec(A)),
# "pair-node" (PairSpec(A, node=True)), "twin-pair" (GatherSpec(ori, None, True)), "scene" (... node=True).
# B = 3: fewer than 128 row blocks (1 or 4 waves per row block); eo (37, 111, 64) = 4107 rows = 129 row blocks, the
# last one ragged, and the pair form at B = 63, N = 11 (4158 rows = 130 row blocks): 1 or 2 waves per row block.
AggCase = Tuple[str, int, int, int]      # (form, B, N or 0, E or scale)
AGG_CASES_FP32: Tuple[AggCase, ...] = (
    ("eo", 3, 0, 23), ("eo", 37, 0, 111), ("gather", 3, 11, 3), ("gather", 3, 20, 5), ("pair", 3, 5, 0), ("pair", 3, 11, 0),
    ("pair", 63, 11, 0), ("pair-node", 3, 5, 0), ("pair-node", 3, 11, 0))
AGG_CASES_BF16: Tuple[AggCase, ...] = (
    ("eo", 3, 0, 23), ("eo", 37, 0, 111), ("gather", 3, 11, 3), ("twin-pair", 3, 5, 0), ("twin-pair", 3, 33, 0),
    ("scene", 3, 5, 0), ("scene", 3, 33, 0))
NODE_FORM_MAX_K = 12


def agg_cases(precision: str, dtype: str = "fp32") -> List[AggCase]:
    """The cases a matrix path has: the fp32 cores have no node form."""
    if dtype == "bf16":
        return list(AGG_CASES_BF16)
    return [c for c in AGG_CASES_FP32 if not (precision == "fp32" and c[0] == "pair-node")]


def agg_module(K: int):
    from groupnet_amd.MS_HGNN_batch import edge_aggregation
    torch.manual_seed(100 + K)
    return edge_aggregation(64, 64, (128,), edge_types=K)


def agg_inputs(K: int, case: AggCase, bf16: bool = False) -> Dict[str, torch.Tensor]:
    """{"ef" (B,E,K) in [0,1), and "eo" (B,E,64) or "ori" (B,N,64) [+ "H" (B,E,N) from the oracle's fp32 ranking]}."""
    form, B, N, x = case
    g = _gen(2, K, B, N, x)
    rnd = lambda *s: torch.randn(*s, generator=g).bfloat16().float() if bf16 else torch.randn(*s, generator=g)
    if form == "eo":
        out = dict(eo=rnd(B, x, 64))
        E = x
    else:
        out = dict(ori=rnd(B, N, 64))
        E = pair_count(N)
        if form == "gather":
            out["H"] = O.topk_incidence_ranked(O.affinity(out["ori"]), x)
            E = out["H"].shape[1]
    out["ef"] = torch.rand(B, E, K, generator=g)
    return out


def agg_ref(state: Dict[str, torch.Tensor], case: AggCase, inp: Dict[str, torch.Tensor], dtype=torch.float64) -> torch.Tensor:
    """O.aggregate_typed_mlp on `state` (keys behind "agg.") in `dtype`: per edge row, or — node and scene form — its
    H^T feat over the ordered pairwise incidence (each ordered edge carrying half its pair row's type weights: the pair
    row holds fac * (dist_ij + dist_ji))."""
    form, B, N, _ = case
    st, ef = cast(state, dtype), inp["ef"].to(dtype)
    if form == "eo":
        return O.aggregate_typed_mlp(st, "agg", ef, inp["eo"].to(dtype))
    ori = inp["ori"].to(dtype)
    if form == "gather":
        return O.aggregate_typed_mlp(st, "agg", ef, O.aggregate_gather(inp["H"].to(dtype), ori))
    ii, jj, row = pair_index(N)
    if form in ("pair", "twin-pair"):
        return O.aggregate_typed_mlp(st, "agg", ef, ori[:, ii] + ori[:, jj])
    H = O.pairwise_incidence(N, B, dtype)
    feat = O.aggregate_typed_mlp(st, "agg", ef[:, row] / 2, O.aggregate_gather(H, ori))
    return torch.matmul(H.permute(0, 2, 1), feat)


def agg_rows(case: AggCase) -> int:
    form, B, N, x = case
    return B * (x if form == "eo" else (N if form == "gather" else pair_count(N)))


def agg_launch_forms(case: AggCase, K: int, precision: str, dtype: str = "fp32", rb2: Optional[str] = None) -> Dict:
    """What gn_agg_mlp_plan_* must say about the launch of this one group (the rules of launch_forms.expected_forms for a
    group of its kind): {"wpr", "node_form", "kernel", "scene_grid"}; "kernel" None where only the scene kernel runs."""
    form, B, N, _ = case
    twin = dtype == "bf16"
    node = form in ("pair-node", "scene")
    if form == "scene":
        return dict(wpr=1, node_form=True, kernel=None, scene_grid=B * cdiv(N, 32))
    kernel = "agg_mlp_kernel" if (precision == "fp32" and not twin) else "agg_x_kernel"
    if twin and rb2 == "1":
        kernel = "agg_rb2_kernel"
    return dict(wpr=1 if node else agg_wpr(agg_rows(case), K), node_form=node, kernel=kernel, scene_grid=None)


# ---------------------------------------------------------------------------------------------------------------------
# 3. whole modules through the engine
# ---------------------------------------------------------------------------------------------------------------------
def engine_modules(N: int, scales: Sequence[Optional[int]], types: Sequence[int], seed: int, nmp: int = 1):
    """Modules in launch order — scale None: the pairwise module — at `types[i]` edge types, and their CPU states."""
    mods = [pair_module(K, seed + 31 * i, nmp) if s is None else hyper_module(K, s, seed + 31 * i, nmp)
            for i, (s, K) in enumerate(zip(scales, types))]
    return mods, [state_of(m) for m in mods]


def engine_inputs(B: int, N: int, scales: Sequence[Optional[int]], types: Sequence[int], seed: int, nmp: int = 1,
                  bf16: bool = False):
    """h (B,N,64), per module the incidence from the oracle's fp32 ranking (None: pairwise) and `nmp` uniform tensors."""
    g = _gen(3, seed, B, N)
    h = torch.randn(B, N, 64, generator=g)
    if bf16:
        h = h.bfloat16().float()
    corr = O.affinity(h)
    Hs = [None if s is None else O.topk_incidence_ranked(corr, s) for s in scales]
    U = [[torch.rand(B, N * N if H is None else H.shape[1], K, generator=g) for _ in range(nmp)] for H, K in zip(Hs, types)]
    return h, Hs, U


def engine_ref(states, h, Hs, U, scenes: torch.Tensor, nmp: int = 1, dtype=torch.float64):
    """[(node_feat, factors)] per module on h[scenes], in `dtype` (launch_forms.pairwise64 / hyper64 for float64)."""
    from launch_forms import hyper64, pairwise64
    out = []
    for st, H, u in zip(states, Hs, U):
        if dtype == torch.float64:
            out.append(pairwise64(st, h, u, scenes, nmp) if H is None else hyper64(st, h, H[scenes], u, scenes, nmp))
            continue
        hs, us = h[scenes].to(dtype), [x[scenes].to(dtype) for x in u]
        if H is None:
            out.append(O.ms_hgnn_pairwise_forward(cast(st, dtype), hs, us, nmp, decomposed=True))
        else:
            out.append(O._message_passing(cast(st, dtype), hs, H[scenes].to(dtype), us, nmp, True, None))
    return out


# the cases of tests/test_edge_types_gpu.py part 3 (tests/test_edge_types_cpu.py runs the fp32 oracle on the same inputs).
# scales: None is the pairwise module; types: K per module in that order
def _ecase(tag: str, B: int, N: int, scales: Sequence[Optional[int]], types: Sequence[int], nmp: int = 1, dtype: str = "fp32"):
    ks = ".".join(map(str, types))
    return dict(id=f"{tag}-B{B}-N{N}-K{ks}" + ("-bf16" if dtype == "bf16" else ""), B=B, N=N, scales=list(scales),
                types=tuple(types), nmp=nmp, dtype=dtype, seed=300 + 17 * sum(types) + len(types))


# the latency form at N = 11 (fuse_closing=True): (pair K, hyper K).  B = 7 with scales {2, 5, 11}: every hyper group has
# fewer than 128 row blocks, so the closing stage is taken from K = 4 on; B = 400 with scales {2, 5}: 4400 rows = 138 row
# blocks, taken from K = 2 on (two waves per row block, K = 3 and 5 leave them unequal shares).  The scale = N group of
# 400 rows would decline K < 4 for every group of the launch: it runs at B = 7.
LATENCY_TYPES = ((1, 1), (12, 2), (1, 3), (12, 4), (1, 5), (12, 15))
LATENCY_CASES = ([_ecase("latency", 7, 11, [None, 2, 5, 11], (kp, kh, kh, kh)) for kp, kh in LATENCY_TYPES]
                 + [_ecase("latency", 400, 11, [None, 2, 5], (kp, kh, kh)) for kp, kh in LATENCY_TYPES])
# beyond the node form's K <= 12 the pairwise module takes the pair form and the closing MLP's fused scatter
PAIR_FORM_CASES = [_ecase("pairform", 7, 11, [None, 2], (K, 10)) for K in (13, 15)]
# one grouped launch whose order follows the cost in K
ORDER_CASE = _ecase("order", 7, 11, [None, 2, 5, 11], (6, 1, 15, 4))
ORDER_POS = [3, 1, 0, 2]        # cost: node form 1; K = 1 at one wave: 8; K = 15 at four: 30; K = 4 at four: 8 (after K = 1: stable)
N17_CASES = [_ecase("n17", 3, 17, [None, 2, 17], (K, K, K)) for K in (1, 5, 13)]              # stand-alone gather and scatter
SCENE_CASES = [_ecase("scene", 3, 33, [None, 2], (K, K), dtype="bf16") for K in (1, 9, 15)]   # bf16 storage, scene form
NMP2_CASES = [_ecase("nmp2", 7, 11, [None, 3, 11], (K, K, K), nmp=2) for K in (3, 13)]
ENGINE_CASES = LATENCY_CASES + PAIR_FORM_CASES + [ORDER_CASE] + N17_CASES + SCENE_CASES + NMP2_CASES


def engine_forms(case: Dict) -> Dict:
    """launch_forms.expected_forms of the case's forward (the block's latency form: the closing stage asked for)."""
    from launch_forms import expected_forms
    return expected_forms(case["B"], case["N"], [s for s in case["scales"] if s is not None], "f16x3", case["dtype"],
                          types=case["types"])


def engine_scenes(case: Dict) -> torch.Tensor:
    """The scenes compared with the oracle: all of a small batch, launch_forms.sample_scenes of a large one."""
    from launch_forms import sample_scenes
    B, N = case["B"], case["N"]
    return torch.arange(B) if B <= 48 else sample_scenes(B, N, engine_forms(case), n=48, seed=B + N)


def engine_case(case: Dict):
    """-> (modules, their CPU states, h, Hs, U, scenes) of an ENGINE_CASES entry."""
    mods, states = engine_modules(case["N"], case["scales"], case["types"], case["seed"], case["nmp"])
    h, Hs, U = engine_inputs(case["B"], case["N"], case["scales"], case["types"], case["seed"], case["nmp"],
                             bf16=case["dtype"] == "bf16")
    return mods, states, h, Hs, U, engine_scenes(case)


# ---------------------------------------------------------------------------------------------------------------------
# 4. backward
# ---------------------------------------------------------------------------------------------------------------------
BACKWARD_KINDS = ("pair", "hyper3", "hyperN")      # the pairwise module, a hyper module at scale 3 and at scale = N
BACKWARD_K = (1, 3, 5, 13, 15)                     # (5 and 13 are padded to 8 and 16 rows in the backward)
BACKWARD_SIZES = ((5, 11), (2, 20))
# A ReLU input this close to zero in the float64 oracle is below what fp32 resolves at the pre-activations' magnitude
# (O(1): one ulp is 1.2e-7): an fp32 implementation has that unit on or off by chance, and with it the unit's whole
# gradient contribution — a finite error that a batch of two to five scenes does not average away (tests/relu_probe.py).
RELU_MARGIN = 1e-7


def backward_oracle(kind: str, state, h: torch.Tensor, U: torch.Tensor, H: Optional[torch.Tensor]):
    """(node_feat, factors) of the module in the dtype of its arguments (one round)."""
    if kind == "pair":
        return O.ms_hgnn_pairwise_forward(state, h, [U], 1, decomposed=True)
    return O._message_passing(state, h, H, [U], 1, True, None)


def backward_case(kind: str, K: int, B: int, N: int):
    """-> {"mod" (on the CPU), "state", "scale", "h", "U", "R1", "R2", "shift", "dead" (`dead_parameters`)}: a module at K types (heads and attention
    scaled away from their flat start, as tests/test_backward_gpu.py) and the inputs of L = <node_feat, R1> + <factors, R2>.
    The inputs are the first of up to 16 seeded draws on which the float64 ORACLE has no ReLU input within RELU_MARGIN of
    zero and at least one clean scene (relu_probe: none within WINDOW), so that the clean-scene gate always applies;
    nothing of the code under test enters the choice (tests/test_edge_types_cpu.py runs the search without a GPU)."""
    from relu_probe import relu_probe
    scale = None if kind == "pair" else (3 if kind == "hyper3" else N)
    mod = pair_module(K, 500 + K) if kind == "pair" else hyper_module(K, scale, 600 + K + N)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if "attention_mlp" in name or "MLP_distribution" in name or "MLP_factor" in name:
                p.mul_(4.0)
    state = state_of(mod)
    E = N * N if kind == "pair" else (1 if scale == N else N)
    for shift in range(16):
        g = _gen(4, BACKWARD_KINDS.index(kind), K, B, N, shift)
        h, U = torch.randn(B, N, 64, generator=g), torch.rand(B, E, K, generator=g)
        R1, R2 = torch.randn(B, N, 64, generator=g), torch.randn(B, E, K, generator=g)
        H = None if kind == "pair" else O.topk_incidence_ranked(O.affinity(h), scale)
        with torch.no_grad(), relu_probe(B) as probe:
            backward_oracle(kind, cast(state, torch.float64), h.double(), U.double(), None if H is None else H.double())
        if float(probe.near.min()) > RELU_MARGIN and bool(probe.clean().any()):
            c = dict(mod=mod, state=state, scale=scale, h=h, U=U, R1=R1, R2=R2, shift=shift)
            c["dead"] = dead_parameters(kind, c)
            return c
    raise AssertionError(f"no draw of {kind} K={K} B={B} N={N} keeps the oracle's ReLU inputs away from zero")


def dead_parameters(kind: str, c: Dict) -> List[str]:
    """The parameters of a `backward_case` whose gradient is zero AS A FUNCTION, in every arithmetic: the oracle's outputs
    do not depend on them at all.  Candidates are those whose float64 gradient on the whole batch is None or exactly
    zero; a candidate is dead iff the oracle's outputs stay bit-identical, in float64 and in fp32, when it is moved by
    O(1) and by O(1000).  That holds for a parameter the forward never reaches and for the distribution head at K = 1
    (a softmax over one type is exp(0) / exp(0)).  It does not hold for a gradient that merely cancels: the attention
    bias of an all-member hyperedge (scale = N) is a softmax shift, whose gradient is a sum of terms that cancel to
    rounding — exactly 0.0 on some hosts and scenes, a residue on others —, and a shift by 1000 moves the logits' low
    bits and with them the outputs.  Such a parameter is compared at the gate like every live one."""
    B = c["h"].shape[0]
    r = backward_reference(kind, dict(c, dead=[]), torch.arange(B))
    g = _gen(5, len(c["state"]))
    dead = []
    with torch.no_grad():
        base = {}
        for dt in (torch.float64, torch.float32):
            H = None if r["H"] is None else r["H"].to(dt)
            base[dt] = (cast(c["state"], dt), c["h"].to(dt), c["U"].to(dt), H)
            base[dt] += (backward_oracle(kind, *base[dt]),)
        for k, grad in r["grads"].items():
            if grad is not None and bool(grad.any()):
                continue
            same = True
            for dt, size in ((torch.float64, 1.0), (torch.float64, 1000.0), (torch.float32, 1.0), (torch.float32, 1000.0)):
                st, h, U, H, (nf0, fac0) = base[dt]
                moved = dict(st)
                moved[k] = st[k] + size * (0.5 + torch.rand(st[k].shape, generator=g)).to(dt)
                nf, fac = backward_oracle(kind, moved, h, U, H)
                same = same and torch.equal(nf, nf0) and torch.equal(fac, fac0)
            if same:
                dead.append(k)
    return sorted(dead)


def backward_reference(kind: str, c: Dict, rows: torch.Tensor):
    """Float64 autograd of the oracle on the scenes `rows` of a `backward_case` -> {"nf", "fac", "dh" (dL/dh), "grads"
    ({parameter: gradient or None}), "probe" (the relu_probe of the forward), "H", "dead" (the case's)}."""
    from relu_probe import relu_probe
    st = {k: v.detach().double().requires_grad_(True) for k, v in c["state"].items()}
    hh = c["h"][rows].detach().double().requires_grad_(True)
    H = None if kind == "pair" else O.topk_incidence_ranked(O.affinity(c["h"][rows]), c["scale"])
    with relu_probe(len(rows)) as probe:
        nf, fac = backward_oracle(kind, st, hh, c["U"][rows].double(), None if H is None else H.double())
    ((nf * c["R1"][rows].double()).sum() + (fac * c["R2"][rows].double()).sum()).backward()
    return dict(nf=nf.detach(), fac=fac.detach(), dh=hh.grad, grads={k: v.grad for k, v in st.items()}, probe=probe, H=H,
                dead=c["dead"])


def live_parameters(kind: str, K: int) -> int:
    """Parameter tensors a one-round forward reaches: six two-layer MLPs (node -> edge start, attention, the edge head's
    three, the closing MLP) and the K typed ones, four tensors each — less the distribution head at K = 1, whose softmax
    over one type is constant."""
    return 24 + 4 * K - (4 if K == 1 else 0)


def rel_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max |got - ref| / max |ref|, in float64."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)


def abs_err(got: torch.Tensor, ref: torch.Tensor) -> float:
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max())
