"""The route of a message-passing forward: which launches it consists of and what each is asked to fuse, decided in one
pure function that `MS_HGNN_batch.run_message_passing` follows; and the graph stage before it — how f becomes the
incidences of every scale — decided in another, `graph_stage_route`, that `multiscale.build_graphs` follows; and the
forms of a backward round, `backward_round_route`, that `backward.round_backward` follows.

A leaf module: no torch, no library, no environment.  The launchers' own decisions (work shapes, kernels, whether an
aggregation launch takes the closing stage it was asked for) stay in their plan functions ("Launch plan").
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import NamedTuple, Tuple

# Kernel limits (`ops` validates its items against them and re-exports them under these names)
POOL_KERNEL_MAX_N = 16      # hyper pooling inside the edge kernel: a row's incidence stays in registers
NODE_FORM_MAX_N = 16        # node form of the pair form (fp32 storage)
NODE_FORM_MAX_K = 12
SCENE_FORM_MAX_N = 64       # the twins' scene form
MASK_MAX_N = 64             # one 64-bit word per hyperedge / node
# The per-scene node->edge backward (gn_node2edge_bwd_f32 / _grouped_f32) holds (4*N*64 + 64 + 16*N) floats of a scene in
# LDS within its 150 KiB budget: 152 576 B at N = 140, 153 664 B at N = 141
N2E_BWD_SCENE_MAX_N = 140

# The engine's own limits.  Beyond these N the stand-alone gather / scatter kernels (LDS-tiled, high occupancy) beat a
# per-lane scan of H rows / a per-lane gather of N feature rows in the prologue of an MFMA kernel (latency-bound at 1-2
# waves per SIMD; measured again in round 2 at N = 50, B = 1024, bf16: typed MLP 390 -> 439 us against a 38-us gather
# launch, closing MLP 54 -> 303 us against 71 + 56 us of scatter launches).
_FUSED_GATHER_MAX_N = 16      # eo = H @ ori inside the typed MLP kernel
_FUSED_SCATTER_MAX_N = 16     # cat(H^T feat, ori)/N inside the closing MLP

# The aggregation's source (`ModuleRoute.source`)
PAIR = "pair"                   # ops.PairSpec: the pairwise graph's pair form on the per-node first layer A
PAIR_NODE = "pair-node"         # ... in its node form
SCENE = "scene"                 # ops.GatherSpec(node=True): the twins' scene form of the pairwise graph
TWIN_PAIR = "twin-pair"         # ops.GatherSpec: the twins' per-pair gather of the pairwise graph
FUSED_GATHER = "fused-gather"   # ops.GatherSpec: eo = H @ ori of a hyper module formed inside the kernel
EO = "eo"                       # the eo tensor of the stand-alone gather launch
# What feeds the closing MLP (`ModuleRoute.closing_input`)
NODE_AGG = "node-agg"           # ops.NodeAggSpec: the aggregation wrote H^T feat per node
SCATTER_SPEC = "scatter-spec"   # ops.ScatterSpec: cat(H^T feat, ori) / N formed inside the closing MLP's kernel
SCATTER = "scatter"             # the output of the stand-alone scatter launch


class Knobs(NamedTuple):
    """Everything that can change per call."""
    fuse_pool: bool         # node->edge pooling inside the edge kernel (MS_HGNN_batch._FUSE_POOL)
    pool_max_n: int         # ... of a hyper module up to this N (ops.POOL_MAX_N)
    node_form: bool         # ops.node_form_enabled()
    masked: bool            # the mask form is on (ops.incidence_form()) and every hyper module came with its masks


@dataclass(frozen=True)
class ModuleRoute:
    pool_in_edge_kernel: bool   # node->edge pooling: ops.PoolSpec in the edge kernel, else the node2edge launch
    first_layer: bool           # the node stage forms the typed MLP's per-node first layer A for this module
    source: str
    node_form: bool             # ... is PAIR_NODE or SCENE: the aggregation writes H^T feat per node
    closing_input: str


@dataclass(frozen=True)
class Route:
    modules: Tuple[ModuleRoute, ...]
    node2edge: Tuple[int, ...]      # the modules that share the node2edge launch (empty: no such launch) ...
    gather: Tuple[int, ...]         # ... the stand-alone gather launch ...
    scatter: Tuple[int, ...]        # ... and the stand-alone scatter launch
    masks: bool                     # those three launches read the hyper modules' masks (and a training step keeps them)
    ask_closing: bool               # ask the aggregation launch's plan to take the closing MLP (ops.agg_mlp_closing)


def masks_in_range(N: int) -> bool:
    """N lies where the stand-alone gather / scatter and the node->edge launch run and a 64-bit word holds a row."""
    return min(_FUSED_GATHER_MAX_N, _FUSED_SCATTER_MAX_N) < N <= MASK_MAX_N


# The graph stage of a block (`GraphStage.kind`): what turns f into the incidences of every scale
NONE = "none"                   # nothing to build (no scales)
BANDED = "banded"               # ops.affinity + ops.topk_incidence: the scene tile is beyond the fused launch's LDS budget
FUSED = "fused"                 # ops.AffinityTail: one job for affinity, every scale's incidence, f -> final, cat(H_s), counter

# Inside a graph capture the fused job and the first node stage (which needs only f) are forked, so the graph runs them
# side by side — worth it only when the launches are long: at B*N = 5.6 k rows the extra graph edges cost more (+9 us
# per replay) than the 7-us overlap saves; at 51 k rows the replay is 33 us shorter.  Eager launches stay on one stream.
FORK_MIN_ROWS = 32768


class StageFacts(NamedTuple):
    """What the caller of a graph stage knows per call."""
    grouped: bool           # the 1+S modules run as grouped launches (one `run_message_passing` for all of them)
    latency_form: bool      # the block's `affinity_tail`: one launch and one boundary fewer where they can be saved
    capturing: bool         # the current stream of a GPU tensor is being captured into a graph
    embed: bool             # the encoder front-end: f itself comes out of the graph stage
    may_defer: bool         # the caller can hand the job to its first node stage (the encoders launch it at once)


@dataclass(frozen=True)
class GraphStage:
    kind: str
    masks: bool             # the launch emits the member words and the incidences carry them
    fork: bool              # the job is launched on the side stream; the message passing joins after its first node stage
    deferred: bool          # the job is handed to the first node stage (its tail workgroups, or issued right before it)
    own_copy: bool          # the builder copies f into final and bumps the counter itself: no fused launch does it
    ask_closing: bool       # what the caller passes on as `run_message_passing(fuse_closing=)`
    H_cat: bool             # cat(H_s) is built (the encoders: from two scales on, as the reference)


def graph_stage_masks(S: int, masked: bool, ragged: bool) -> bool:
    """Whether the fused launch of S scales is asked for the member words: not for a ragged batch, whose route reads no
    masks and whose launch emits none."""
    return S > 0 and masked and not ragged


@functools.lru_cache(maxsize=None)
def graph_stage_route(S: int, form: str, rows: int, *, masked: bool, ragged: bool, training: bool,
                      facts: StageFacts, ragged_training: bool = False) -> GraphStage:
    """The graph stage of one forward over S scales.  form: the library's answer for the launch in question
    (`ops.graph_form`: "tail" | "fused" | "banded" — the tile rule is stated in C only); rows = B*N; masked: the mask form
    is on and `masks_in_range(N)` holds; training: the forward runs under autograd — it writes into no final and leaves
    the counter to its caller, and nothing is forked, deferred or asked of the closing stage.
    ragged: no masks, and the job — which is never the tail, `AffinityTail.fits_tail` — is still handed
    on where the caller defers: the first node stage issues it on its own.  ragged and training go together only under
    the caller's opt-in, ragged_training (`MS_HGNN_batch.set_ragged_training`): the stage is then the training one —
    launched at once, no final, the counter is the caller's — over the counts.
    Whether a deferred job rides as tail workgroups ("tail") or is issued beside the node stage ("fused") is the node
    stage's decision; here only "banded" or not matters."""
    if ragged and training and not ragged_training:
        raise NotImplementedError("ragged batches are inference-only")
    if form != BANDED and (S or facts.embed):
        kind = FUSED            # the front-end's launch needs >= 1 scale: the builder gives it N, the all-ones edge
    else:
        kind = BANDED if S else NONE
    live = kind == FUSED and not training
    masks = kind == FUSED and graph_stage_masks(S, masked, ragged)
    fork = live and facts.grouped and not facts.embed and facts.capturing and rows >= FORK_MIN_ROWS
    # forked, ungrouped or emitting masks (which only the stand-alone launch does) the job is a launch of its own
    deferred = live and facts.may_defer and facts.grouped and not fork and facts.latency_form and not masks
    return GraphStage(kind=kind, masks=masks, fork=fork, deferred=deferred, own_copy=kind != FUSED and not training,
                      ask_closing=facts.grouped and facts.latency_form and not facts.embed and not training,
                      H_cat=kind != NONE and S >= (2 if facts.embed else 1))


@functools.lru_cache(maxsize=None)
def message_passing_route(N: int, modules: Tuple[Tuple[bool, int], ...], *, twin: bool, training: bool, matrix16: bool,
                          knobs: Knobs, closing_asked: bool, ragged: bool = False, ragged_training: bool = False) -> Route:
    """The route of one forward over N agents.  modules: (pairwise, K edge types) per module in launch order; twin: bf16
    storage; training: the forward keeps what a backward reads; matrix16: the 16-bit-core weight images are in use;
    closing_asked: the caller would like the aggregation launch to apply the closing MLP.
    ragged: the scenes hold different numbers of agents (N is the padded size; a training forward only under the
    caller's opt-in, ragged_training — `MS_HGNN_batch.set_ragged_training`).  The agent count enters
    the arithmetic in the node->edge pooling and in the scatter, so both run as their own (count-aware) launches and
    every form that fuses one of them into an MFMA kernel is left out: no pooling in the edge kernel, no node / scene
    form of the pairwise aggregation (their sums run over all N partners), no closing stage in the aggregation launch,
    no fused scatter, no masks.  What stays is row-wise or reads the padding only through zero entries of H.  That route
    already keeps what a backward reads — the node->edge launch's `edges` of every module, the pair form on the per-node
    first layer (no node form), the scatter launch's tensor as the closing MLP's input — so the ragged training forward
    takes it as it is."""
    if twin and training:
        raise NotImplementedError("the bf16 twins are forward-only")
    if ragged:
        if training and not ragged_training:
            raise NotImplementedError("ragged batches are inference-only")
        mods = [ModuleRoute(False, pairwise and not twin,
                            (TWIN_PAIR if twin else PAIR) if pairwise else (FUSED_GATHER if N <= _FUSED_GATHER_MAX_N else EO),
                            False, SCATTER) for pairwise, _ in modules]
        every = tuple(range(len(mods)))
        return Route(modules=tuple(mods), node2edge=every,
                     gather=tuple(i for i, m in enumerate(mods) if m.source == EO), scatter=every, masks=False,
                     ask_closing=False)
    mods = []
    for pairwise, K in modules:
        # Inference: the pooled edge rows feed only the edge MLP, so its kernel forms them itself and `edges` never
        # exists in HBM — always for the pairwise graph, for hyper modules up to pool_max_n nodes; larger hyper modules
        # (and training, whose backward reads `edges`) keep the node2edge launch.
        pool = knobs.fuse_pool and not training and (twin or matrix16) and (pairwise or N <= knobs.pool_max_n)
        # Pairwise, fp32 storage: eo = ori_i + ori_j makes the typed MLP's first layer linear in the two nodes, so it
        # runs once per NODE, in the round's node stage, and the pair form does the rest.  The twins run both layers on
        # the matrix cores: per node, one scene per workgroup (scene form), or per unordered pair.
        first_layer = pairwise and not twin
        if first_layer:
            node = (knobs.node_form and matrix16 and N <= NODE_FORM_MAX_N and K <= NODE_FORM_MAX_K
                    and N <= _FUSED_SCATTER_MAX_N)
            source = PAIR_NODE if node else PAIR
        elif pairwise:
            node = knobs.node_form and N <= SCENE_FORM_MAX_N
            source = SCENE if node else TWIN_PAIR
        else:
            node = False
            source = FUSED_GATHER if N <= _FUSED_GATHER_MAX_N else EO
        closing_input = NODE_AGG if node else (SCATTER_SPEC if N <= _FUSED_SCATTER_MAX_N else SCATTER)
        mods.append(ModuleRoute(pool, first_layer, source, node, closing_input))
    which = lambda pred: tuple(i for i, m in enumerate(mods) if pred(m))
    return Route(modules=tuple(mods),
                 node2edge=which(lambda m: not m.pool_in_edge_kernel),
                 gather=which(lambda m: m.source == EO),
                 scatter=which(lambda m: m.closing_input == SCATTER),
                 masks=knobs.masked and masks_in_range(N),
                 ask_closing=closing_asked and not training and not twin and N <= _FUSED_SCATTER_MAX_N)


@dataclass(frozen=True)
class BackwardRound:
    pair_rows: bool         # a pairwise module walks its N(N+1)/2 unordered-pair rows (`sym`), as its forward did; else
                            # ordered rows and the explicit (B, N*N, N) incidence
    kept: bool              # every module reads the activations the forward kept; else every module re-computes them
    n2e_grouped: bool       # one gn_node2edge_bwd_grouped_f32 for all modules, else one gn_node2edge_bwd_f32 per module


@functools.lru_cache(maxsize=None)
def backward_round_route(N: int, pairwise: Tuple[bool, ...], ragged: bool = False, *,
                         deterministic: bool = False) -> BackwardRound:
    """The route of one backward round over N agents (`backward.round_backward`).  pairwise: per module of the round.
    All of it hangs on whether a scene fits the per-scene node->edge backward.  Where it does not, a pairwise module
    needs ordered edge rows — the general kernel reads an incidence, and the pairwise one exists only per ordered edge —
    while its forward kept activations per unordered pair: they are re-computed, and since the re-computation is one
    grouped launch per stage, for every module of the round.
    ragged: the forward recorded per-scene counts.  The count-aware node->edge backward exists in the per-scene form
    only (gn_node2edge_bwd_ragged_grouped_f32), so the round is the fitting one or none.
    deterministic: the caller asks for the ordered pooling backward (gn_node2edge_bwd_det_grouped_f32), which also has
    the per-scene form only: the fitting round, unchanged, or none."""
    fits = N <= N2E_BWD_SCENE_MAX_N
    if deterministic and not fits:
        raise NotImplementedError(f"the deterministic backward needs N <= {N2E_BWD_SCENE_MAX_N} (got {N}): the ordered "
                                  "node->edge backward has the per-scene form only")
    if ragged and not fits:
        raise NotImplementedError(f"the backward of a ragged batch needs N <= {N2E_BWD_SCENE_MAX_N} (got {N}): the "
                                  "count-aware node->edge backward has the per-scene form only")
    return BackwardRound(pair_rows=fits, kept=fits or not any(pairwise), n2e_grouped=fits)
