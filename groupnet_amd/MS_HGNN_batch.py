"""Drop-in replacement of the reference's ``model/MS_HGNN_batch.py`` for MI355X.

    from groupnet_amd.MS_HGNN_batch import MS_HGNN_oridinary, MS_HGNN_hyper, MLP

keeps the constructor arguments, ``forward()`` signatures, return tuples and
``state_dict`` keys of the reference classes (model/MS_HGNN_batch.py:55-198,
201-229, 270-443), so ``model/GroupNet_nba.py:9,209-248,290-299`` works unchanged
and ``load_state_dict(strict=True)`` of a reference checkpoint succeeds.  The
modules are parameter containers plus orchestration: every tensor operation of the
forward is a hand-written gfx950 kernel of libgroupnet_hip.so (``groupnet_amd.ops``).
There is no CPU path and no torch-math fallback; CPU tensors raise ``ValueError``.

Differences from the reference that a caller can observe
  * tensors must be on the GPU (the reference fork only runs on the CPU);
  * under autograd the two MS_HGNN modules return outputs with a HIP backward attached
    (``groupnet_amd.backward``); their sub-modules (``MLP``,
    ``MLP_dict_softmax``, ``edge_aggregation``) called on their own are forward-only;
  * optional ``noise_u=`` lets the caller inject the uniforms of the Gumbel noise.
    By default they are drawn exactly as the reference does — ``torch.rand`` on the
    global CPU generator, one ``(B,E,K)`` draw per MLP_dict_softmax call
    (model/MS_HGNN_batch.py:45,454) — and uploaded; ``set_noise_mode('device', seed)``
    switches to the on-device Philox stream.
"""
from __future__ import annotations

import contextlib
import os
import warnings
from typing import Iterator, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn as nn

from . import ops, route, weights
from .weights import _param_key, _volatile, training_call  # noqa: F401  (cache policy, re-exported)

Tensor = torch.Tensor
_HDIM_EXTEND = 64      # model/MS_HGNN_batch.py:72,292
_GUMBEL_TAU = 0.5      # model/MS_HGNN_batch.py:45


def masks_apply(N: int) -> bool:
    """Whether a forward (inference or training) over N agents has launches that read the bit-mask form of an incidence:
    the form is switched on (`ops.set_incidence_form` / GN_INC_MASKS=1) and N lies where the stand-alone gather /
    scatter and the node->edge launch run and a 64-bit word holds a row (16 < N <= 64).  Elsewhere nobody asks for masks
    and no launch changes."""
    return ops.incidence_form() == "mask" and route.masks_in_range(N)


# node->edge pooling inside the edge kernel (inference); the parity tests clear it to compare against the node2edge launch
_FUSE_POOL = True


# ---------------------------------------------------------------------------------------------
# noise source
# ---------------------------------------------------------------------------------------------
class _NoiseState:
    mode = "host"   # "host": torch.rand on the CPU generator (reference contract); "device": Philox
    seed = 0
    offset = 0      # running element offset of the device stream (host-side bookkeeping)
    counter = None  # optional 1-element int64 GPU tensor added to `offset` on the device (graph replays)


def set_noise_mode(mode: str, seed: Optional[int] = None, offset: int = 0, counter: Optional[Tensor] = None) -> None:
    """'host' (default, reference-identical stream) or 'device' (Philox4x32-10, no host work).
    ``counter``: a 1-element int64 GPU tensor holding the stream position on the DEVICE; a captured
    hipGraph that ends with ``ops.counter_add(counter, n)`` then draws fresh noise on every replay."""
    if mode not in ("host", "device"):
        raise ValueError("mode must be 'host' or 'device'")
    _NoiseState.mode = mode
    _NoiseState.counter = counter if mode == "device" else None
    if seed is not None:
        _NoiseState.seed = int(seed)
        _NoiseState.offset = int(offset)


def _draw_uniform(shape: Tuple[int, int, int], device: torch.device):
    """The uniforms of one MLP_dict_softmax call: a tensor drawn as the reference does (host mode), or
    a handle on the next shape-sized span of the device Philox stream, expanded inside the edge kernel."""
    if _NoiseState.mode == "host":
        return torch.rand(shape).float().to(device, non_blocking=True)
    u = ops.PhiloxNoise(_NoiseState.seed, _NoiseState.offset, _NoiseState.counter)
    _NoiseState.offset += shape[0] * shape[1] * shape[2]
    return u


def _noise_iter(noise_u: Union[None, Tensor, Sequence[Tensor]]) -> Optional[Iterator[Tensor]]:
    if noise_u is None:
        return None
    if isinstance(noise_u, (torch.Tensor, ops.PhiloxNoise)):
        return iter([noise_u])
    return iter(list(noise_u))


def _plist(m: nn.Module) -> tuple:
    """Parameters of `m` as a cached tuple (walking the module tree costs ~10 us per call and the engine asks
    hundreds of times per step); dropped by `invalidate_weight_caches`."""
    pl = m.__dict__.get("_gn_plist")
    if pl is None:
        pl = m.__dict__["_gn_plist"] = tuple(m.parameters())
    return pl


def _needs_grad(mod: nn.Module, *inputs: Optional[Tensor]) -> bool:
    """True when autograd is recording and the call involves anything that wants a gradient."""
    if not torch.is_grad_enabled():
        return False
    return any(t is not None and t.requires_grad for t in inputs) or any(p.requires_grad for p in _plist(mod))


# Training on ragged batches (``n_agents`` under autograd) is opt-in: None — not set by `set_ragged_training`, the
# environment decides per call (GN_RAGGED_TRAINING=1: on).
_RAGGED_TRAINING: Optional[bool] = None


def ragged_training() -> bool:
    """Whether a forward with ``n_agents`` may run under autograd: what `set_ragged_training` chose, else
    GN_RAGGED_TRAINING=1 switches it on (read per call).  Off by default: such a call is refused before any launch.
    Inside `ragged_train_graph_scope` it is on whatever the two say."""
    if _TRAIN_GRAPH_SCOPE[0]:
        return True
    if _RAGGED_TRAINING is not None:
        return _RAGGED_TRAINING
    return os.environ.get("GN_RAGGED_TRAINING", "0") == "1"


def set_ragged_training(on: Optional[bool]) -> None:
    """True / False for calls issued from now on; None hands the choice back to the environment."""
    global _RAGGED_TRAINING
    _RAGGED_TRAINING = None if on is None else bool(on)


# The step of a ragged `graphs.GraphedTrainStep` is its own opt-in: how many `ragged_train_graph_scope`s are open.
_TRAIN_GRAPH_SCOPE = [0]


@contextlib.contextmanager
def ragged_train_graph_scope():
    """Entered by `graphs.GraphedTrainStep._step` alone, around the step of a ragged capture: inside it a forward with
    ``n_agents`` runs under autograd whatever `set_ragged_training` / GN_RAGGED_TRAINING say (`ragged_training`), and so
    do holders that admit empty slots (`trains_empty_slots`: `ops.StaticAgentCounts`, a subset whose values live on the
    device).  Every other refusal of a ragged call holds inside it as well.  Closed on the way out, an exception
    included; scopes nest."""
    _TRAIN_GRAPH_SCOPE[0] += 1
    try:
        yield
    finally:
        _TRAIN_GRAPH_SCOPE[0] -= 1


def trains_empty_slots() -> bool:
    """Whether counts that admit empty slots may run under autograd: inside `ragged_train_graph_scope` only."""
    return _TRAIN_GRAPH_SCOPE[0] > 0


# The deterministic backward is opt-in the same way: None — not set by `set_deterministic`, the environment decides per
# call (GN_DETERMINISTIC=1: on).
_DETERMINISTIC: Optional[bool] = None


def deterministic() -> bool:
    """Whether a backward sums in a fixed order (`backward.GemmBatch.run` takes gn_gemm_grouped_det_f32, the pooling
    backward gn_node2edge_bwd_det_grouped_f32): what `set_deterministic` chose, else GN_DETERMINISTIC=1 switches it on
    (read per call).  Off by default: every call launches what it always did.  torch's own
    `use_deterministic_algorithms` flag is not read."""
    if _DETERMINISTIC is not None:
        return _DETERMINISTIC
    return os.environ.get("GN_DETERMINISTIC", "0") == "1"


def set_deterministic(on: Optional[bool]) -> None:
    """True / False for calls issued from now on; None hands the choice back to the environment.  A captured graph keeps
    the form it was captured with."""
    global _DETERMINISTIC
    _DETERMINISTIC = None if on is None else bool(on)


# What a ragged call (``n_agents``) is refused for, by the caller's keyword: the exception and its text
_RAGGED_REFUSALS = {
    "large": (NotImplementedError, f"n_agents: training on ragged batches needs N <= {route.N2E_BWD_SCENE_MAX_N} (the "
                                   "count-aware node->edge backward has the per-scene form only)"),
    "handed_in": (ValueError, "n_agents: the ragged incidence is built here; H= / masks= cannot be handed in with it"),
    "listall": (NotImplementedError, "n_agents: the exhaustive (listall) search has no ragged form"),
    "grad": (NotImplementedError, "n_agents: ragged batches are inference-only (call under torch.no_grad())"),
    "training": (NotImplementedError, "n_agents: ragged batches are inference-only (call block.eval() first)"),
}


def refuse_ragged(**holds: bool) -> None:
    """Raise the first refusal of `_RAGGED_REFUSALS` whose condition holds, in the order the caller names them."""
    for why, held in holds.items():
        if held:
            exc, text = _RAGGED_REFUSALS[why]
            raise exc(text)


def ragged_grad_refusals(grad: bool, N: int) -> dict:
    """What a ragged call under autograd (``grad``) is refused for: everything without the opt-in (`ragged_training`),
    with it a padded size beyond the per-scene node->edge backward."""
    on = ragged_training()
    return dict(grad=grad and not on, large=grad and on and N > route.N2E_BWD_SCENE_MAX_N)


def ragged_counts(n_agents, x: Tensor, **refusals: bool) -> Optional[ops.AgentCounts]:
    """A forward's ``n_agents`` for its (B,N,...) input ``x`` as the validated `ops.AgentCounts`, or None where the call
    is not ragged (`ops.agent_counts`; an empty batch never is).  A ragged call is refused by `refuse_ragged`."""
    B, N = x.shape[0], x.shape[1]
    counts = ops.agent_counts(n_agents, B, N, x.device) if B and N else None
    if counts is not None:
        refuse_ragged(**refusals)
    return counts


# ---------------------------------------------------------------------------------------------
# agents missing anywhere (``n_agents`` = an `ops.AgentSubset`): compaction, the ragged route, expansion
# ---------------------------------------------------------------------------------------------
def subset_of(n_agents, x: Tensor, grad: bool, **refusals: bool) -> Optional["ops.AgentSubset"]:
    """``n_agents`` as the `ops.AgentSubset` of a forward over the (B,N,...) input ``x``, or None where it is anything
    else.  A subset call is refused here, before anything is uploaded or launched: a subset of other sizes
    (ValueError), what a ragged call is refused for (`refuse_ragged`, `ragged_grad_refusals`), and under autograd a
    subset built from a GPU mask, which admits empty scenes."""
    if not isinstance(n_agents, ops.AgentSubset):
        return None
    ops.agent_counts(n_agents, x.shape[0], x.shape[1], x.device)      # the sizes
    refuse_ragged(**refusals, **ragged_grad_refusals(grad, x.shape[1]))
    if grad and n_agents.admits_empty and not trains_empty_slots():
        raise NotImplementedError("n_agents: counts that admit empty slots (a subset built from a GPU mask) are "
                                  "inference-only")
    return n_agents


def subset_noise(noise_u, shape: Tuple[int, int, int], rounds: int, device) -> Optional[list]:
    """One module's noise on the subset route, in the ORIGINAL layout: the caller's tensor(s) or `ops.PhiloxNoise`
    handle(s), checked, as a list per round; without them the host-mode draws of every round, made here as the engine
    would make them; None in device mode (the draws are those of the compacted batch)."""
    if noise_u is None:
        if _NoiseState.mode != "host":
            return None
        return [_draw_uniform(shape, device) for _ in range(rounds)]
    us = [noise_u] if isinstance(noise_u, (torch.Tensor, ops.PhiloxNoise)) else list(noise_u)
    for u in us:
        if not isinstance(u, ops.PhiloxNoise):
            ops._req(u, "noise_u", shape)
    return us


def remap_noise(us: Optional[list], kind: int, items: list) -> Optional[list]:
    """The compacted twin of a module's noise list: every tensor gets a scratch twin and an item in ``items`` (the
    caller's compaction launch); handles and the single row of a scale-N module (``kind`` None) pass through."""
    if us is None or kind is None:
        return us
    out = []
    for u in us:
        if isinstance(u, torch.Tensor):
            c = torch.empty_like(u)
            items.append((u, c, kind))
            u = c
        out.append(u)
    return out


class _Remap(torch.autograd.Function):
    """`ops.remap_rows` of several tensors under autograd: ``to_slots`` False — the compaction (map = order), True —
    the expansion (map = slot).  Each is the other's adjoint on the positions that carry values: the backward is the
    same launch with the other map over the incoming gradients, into fresh tensors (the caller's are not written)."""

    @staticmethod
    def forward(ctx, sub, to_slots: bool, kinds: tuple, *tensors: Tensor):
        ctx.sub, ctx.to_slots, ctx.kinds = sub, to_slots, kinds
        srcs = [t.contiguous() for t in tensors]
        outs = [torch.empty_like(s) for s in srcs]
        ops.remap_rows(list(zip(srcs, outs, kinds)), sub.slot if to_slots else sub.order)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        res, items = [None] * len(grads), []
        for i, (g, kind, need) in enumerate(zip(grads, ctx.kinds, ctx.needs_input_grad[3:])):
            if g is not None and need:
                g = g.contiguous()
                res[i] = torch.empty_like(g)
                items.append((g, res[i], kind))
        if items:
            ops.remap_rows(items, ctx.sub.order if ctx.to_slots else ctx.sub.slot)
        return (None, None, None, *res)


def _check_subset_out(out: Optional[Tensor], h: Tensor, width: int) -> None:
    """A caller's ``out=`` on the subset route: where the expansion writes node_feat, (B,N,width) of h's type."""
    if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == h.dtype
                                and tuple(out.shape) == (h.shape[0], h.shape[1], width)):
        raise ValueError(f"out: a GPU tensor of shape {(h.shape[0], h.shape[1], width)} and dtype {h.dtype}")


def incidence_item(Hc: Tensor, H: Tensor) -> Tuple[Tensor, Tensor, int]:
    """The expansion item of one module's incidence: a (B,N,N) top-k H as a matrix of ordered pairs, the single (B,1,N) row
    of a scale-N module as node rows of its (B,N,1) view."""
    if Hc.shape[1] == 1 and Hc.shape[2] != 1:
        return Hc.transpose(1, 2), H.transpose(1, 2), ops.REMAP_NODE_ROWS
    return Hc, H, ops.REMAP_PAIR_ROWS


_warned_grad = False


def _check_forward_only(*inputs: Tensor) -> None:
    global _warned_grad
    if not torch.is_grad_enabled():
        return
    if any(t is not None and t.requires_grad for t in inputs):
        raise RuntimeError("this sub-module is forward-only when called on its own: an input requires grad. "
                           "Differentiate through MS_HGNN_oridinary / MS_HGNN_hyper (groupnet_amd.backward) or call "
                           "it under torch.no_grad().")
    if not _warned_grad:
        warnings.warn("groupnet_amd sub-modules called on their own are forward-only; outputs carry no autograd graph.")
        _warned_grad = True


# ---------------------------------------------------------------------------------------------
# parameter containers (same names / shapes as the reference so state_dicts interchange)
# ---------------------------------------------------------------------------------------------
class MLP(nn.Module):
    """Stack of nn.Linear with an activation between layers (model/MS_HGNN_batch.py:201-229).

    Inside the MS-HGNN modules an MLP is only a parameter container — the fused HIP chains read
    its weights.  Called on its own (the reference's L3 model imports it for unrelated heads,
    model/GroupNet_nba.py:9,31-32) every Linear runs on the HIP GEMM (`groupnet_amd.linear.hip_linear`,
    differentiable); activations / dropout between the layers are elementwise torch ops.  GPU tensors only,
    like everything else in this package.
    """

    def __init__(self, input_dim, output_dim, hidden_size=(1024, 512), activation='relu', discrim=False,
                 dropout=-1):
        super().__init__()
        widths = [input_dim, *hidden_size, output_dim]
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(widths[:-1], widths[1:]))
        if activation == 'relu':
            self.activation = nn.ReLU()
        elif activation == 'sigmoid':
            self.activation = nn.Sigmoid()
        self.sigmoid = nn.Sigmoid() if discrim else None
        self.dropout = dropout

    def forward(self, x):
        from .linear import hip_linear
        ops._req(x, "x")
        last = len(self.layers) - 1
        for i, layer in enumerate(self.layers):
            x = hip_linear(x, layer)
            if i != last:
                x = self.activation(x)
                if self.dropout != -1:
                    p = min(0.1, self.dropout / 3) if i == 1 else self.dropout
                    x = nn.functional.dropout(x, p=p, training=True)
            elif self.sigmoid is not None:
                x = self.sigmoid(x)
        return x


def _two_layer(mlp: MLP) -> Tuple[nn.Linear, nn.Linear]:
    if len(mlp.layers) != 2:
        raise NotImplementedError("the HIP chains are built for MLPs with one hidden layer")
    return mlp.layers[0], mlp.layers[1]


class MLP_dict_softmax(nn.Module):
    """Edge-type head (model/MS_HGNN_batch.py:31-53): (factor * distribution, distribution)."""

    def __init__(self, input_dim, output_dim, hidden_size=(1024, 512), activation='relu', discrim=False,
                 dropout=-1, edge_types=5):
        super().__init__()
        if input_dim != _HDIM_EXTEND or tuple(hidden_size) != (128,):
            raise NotImplementedError("HIP edge-MLP chain is specialised to 64 -> 128 -> {64, K, 1}")
        if not 1 <= edge_types <= 15:
            raise NotImplementedError("edge_types must be in 1..15")
        self.bottleneck_dim = edge_types
        self.MLP_distribution = MLP(input_dim=input_dim, output_dim=edge_types, hidden_size=hidden_size)
        self.MLP_factor = MLP(input_dim=input_dim, output_dim=1, hidden_size=hidden_size)
        self.init_MLP = MLP(input_dim=input_dim, output_dim=input_dim, hidden_size=hidden_size)

    def _packed(self) -> dict:
        """Weight stream of the edge-MLP kernel (layout: `weights.edge_mlp`) and its biases."""
        return weights.cache(self, "edge").get(_plist(self), lambda plan: weights.edge_mlp(
            plan, _two_layer(self.init_MLP), _two_layer(self.MLP_distribution), _two_layer(self.MLP_factor)))

    def forward(self, x, noise_u: Optional[Tensor] = None):
        _check_forward_only(x)
        if x.dim() != 3:
            raise ValueError("MLP_dict_softmax expects (B, E, 64); the reference's softmax is only "
                             "well-defined for 3-D input (model/MS_HGNN_batch.py:517-520)")
        K = self.bottleneck_dim
        U = noise_u if noise_u is not None else _draw_uniform((x.shape[0], x.shape[1], K), x.device)
        return ops.edge_mlp_gumbel(x, U, self._packed(), K, _GUMBEL_TAU)


class edge_aggregation(nn.Module):
    """Typed edge -> node aggregation (model/MS_HGNN_batch.py:247-268): cat(H^T feat, ori)."""

    def __init__(self, input_dim, output_dim, hidden_size=(1024, 512), activation='relu', discrim=False,
                 dropout=-1, edge_types=5):
        super().__init__()
        if input_dim != 64:
            raise NotImplementedError("HIP aggregation kernels are specialised to 64-wide features")
        if not 1 <= edge_types <= 16:
            raise NotImplementedError("edge_types must be in 1..16")      # GN_MAX_TYPES (include/groupnet_hip.h)
        self.edge_types = edge_types
        self.dict_dim = input_dim
        self.agg_mlp = nn.ModuleList(MLP(input_dim=input_dim, output_dim=input_dim, hidden_size=(128,))
                                     for _ in range(edge_types))
        self.mlp = MLP(input_dim=input_dim, output_dim=input_dim, hidden_size=(128,))  # unused, kept for state_dict

    def _packed(self) -> dict:
        """Packed images of the K typed MLPs (layout: `weights.typed_agg`)."""
        return weights.cache(self, "agg").get(_plist(self.agg_mlp), lambda plan: weights.typed_agg(
            plan, [m.layers[0] for m in self.agg_mlp], [m.layers[1] for m in self.agg_mlp]))

    def forward(self, edge_distribution, H, ori):
        """Returns cat(H^T feat, ori) WITHOUT the division by N (that is edge2node's,
        model/MS_HGNN_batch.py:120,355).  ``H=None`` selects the implicit pairwise graph."""
        _check_forward_only(edge_distribution, ori)
        return self._aggregate(edge_distribution, H, ori, divisor=1.0)

    def _aggregate(self, edge_feat, H, ori, divisor=None):
        """gather -> typed MLP -> scatter; divisor=None applies the / N of edge2node."""
        eo = ops.agg_gather(ori, H)
        feat = ops.agg_mlp(eo, edge_feat, self._packed(), self.edge_types)
        return ops.agg_scatter(feat, H, ori, divisor)


def invalidate_weight_caches(module: nn.Module) -> None:
    """Mark every packed / concatenated weight image below `module` stale.  They are keyed on the parameters'
    (address, in-place version); anything that rewrites parameters behind autograd's back — a replayed
    hipGraph containing the optimizer step — must call this before the next eager use.  (The pack plans
    themselves — arenas and segment tables — stay; the next use re-runs their one refresh launch.  A captured inference
    graph — `graphs.GraphedMultiScale`, `graphs.GraphedPastEncoder` — sees the invalidation too and re-derives its
    images before its next replay.)"""
    weights.note_invalidation()
    for m in module.modules():
        d = m.__dict__
        d.pop("_gn_plist", None)
        for c in weights.caches(m):
            c.invalidate()
        for entry in (d.get("_affine") or {}).values():
            entry[0] = None         # the composed embedding: its buffers stay, the next use writes them again


class _MessagePassing(nn.Module):
    """What both reference modules share: one or more node->edge->node rounds
    (model/MS_HGNN_batch.py:174-195, 425-441)."""

    edge_types: int

    def _build(self, h_dim: int, bottleneck_dim: int, nmp_layers: int) -> None:
        if h_dim != 64:
            raise NotImplementedError("the gfx950 kernels are specialised to h_dim == 64 "
                                      "(every caller in the reference uses 64, model/GroupNet_nba.py:209-248)")
        if nmp_layers < 1:
            raise ValueError("nmp_layers must be >= 1")
        K = self.edge_types
        self.nmp_mlp_start = MLP_dict_softmax(input_dim=_HDIM_EXTEND, output_dim=h_dim, hidden_size=(128,),
                                              edge_types=K)
        rounds = []
        for _ in range(nmp_layers - 1):
            rounds.append(MLP(input_dim=h_dim * 2, output_dim=h_dim, hidden_size=(128,)))
            rounds.append(MLP_dict_softmax(input_dim=_HDIM_EXTEND, output_dim=h_dim, hidden_size=(128,),
                                           edge_types=K))
        self.nmp_mlps = nn.ModuleList(rounds)
        self.nmp_mlp_end = MLP(input_dim=h_dim * 2, output_dim=bottleneck_dim, hidden_size=(128,))
        self.attention_mlp = nn.ModuleList(MLP(input_dim=_HDIM_EXTEND * 2, output_dim=1, hidden_size=(32,))
                                           for _ in range(nmp_layers))
        self.node2edge_start_mlp = nn.ModuleList(MLP(input_dim=h_dim, output_dim=_HDIM_EXTEND, hidden_size=(256,))
                                                 for _ in range(nmp_layers))
        self.edge_aggregation_list = nn.ModuleList(
            edge_aggregation(input_dim=h_dim, output_dim=bottleneck_dim, hidden_size=(128,), edge_types=K)
            for _ in range(nmp_layers))

    # -- packed weights ------------------------------------------------------------------------
    def _packed_n2e(self, idx: int) -> dict:
        start, att = self.node2edge_start_mlp[idx], self.attention_mlp[idx]
        return weights.cache(self, ("n2e", idx)).get(_plist(start) + _plist(att), lambda plan: weights.node_chain(
            plan, _two_layer(start), _two_layer(att)))

    def _packed_mlp2(self, mlp: MLP) -> dict:
        return weights.cache(mlp, "mlp2").get(_plist(mlp), lambda plan: weights.closing_mlp(plan, *_two_layer(mlp)))

    # -- stages (single-module faces of the grouped engine below) -----------------------------------
    def _node2edge(self, x: Tensor, H: Optional[Tensor], idx: int) -> Tensor:
        pk = self._packed_n2e(idx)
        xp, pq = ops.node_mlp(x, pk)
        return ops.node2edge(xp, pq, H, pk["w2"], pk["b2"])

    def _edge2node(self, edge_feat: Tensor, ori: Tensor, H: Optional[Tensor], idx: int) -> Tensor:
        return self.edge_aggregation_list[idx]._aggregate(edge_feat, H, ori)

    def _run(self, h: Tensor, H, E: int, noise_u, out: Optional[Tensor] = None, n_agents=None) -> Tuple[Tensor, Tensor]:
        return run_message_passing([self], [h], [H], [noise_u], [out], n_agents=n_agents)[0]

    def _forward_autograd(self, h: Tensor, H: Optional["ops.Incidence"], noise_u, out: Optional[Tensor],
                          counts: Optional["ops.AgentCounts"] = None) -> Tuple[Tensor, Tensor]:
        """Training path: fused forward + HIP backward through torch.autograd.  ``H``: None or the
        module's `ops.Incidence`, whose masks the forward and the backward read where `masks_apply` holds.  ``counts``:
        the ragged batch's counts (`set_ragged_training`); ``H`` is then the ragged incidence."""
        from .backward import MSHGNNFunction
        if out is not None:
            raise ValueError("out= is an inference-time extra; under autograd the module returns a new tensor")
        if h.dtype == torch.bfloat16:
            # bf16 activations under autograd (config 4's storage type in training): the twins' kernels are
            # forward-only, so the training step runs the fp32 training path on the up-cast inputs — forward values
            # then carry fp32 intermediates (within the twins' own tolerance of them), gradients are those of the fp32
            # function at the bf16-rounded inputs, and outputs / the input gradient come back in bf16 (the casts are
            # ordinary differentiable torch ops).
            H = None if H is None else ops.Incidence(H.H.float(), H.masks)
            nf, fac = MSHGNNFunction.apply((self,), (H,), (noise_u,), counts, h.float(), *_plist(self))
            return nf.to(torch.bfloat16), fac.to(torch.bfloat16)
        if h.dtype != torch.float32:
            raise NotImplementedError("activations must be fp32 or bf16")
        return MSHGNNFunction.apply((self,), (H,), (noise_u,), counts, h, *_plist(self))


BF16_MAX_BOTTLENECK = 64      # gn_mlp2_bf16: the bf16-core kernels hold at most two 32-wide output tiles


def _check_storage_width(bottleneck_dim: int, dtype: torch.dtype) -> None:
    """bf16 storage runs the closing MLP on the bf16-core kernels alone, whose output ends at 64 columns (the launcher
    refuses a wider one): said here, before a forward has launched anything, instead of at its last launch."""
    if dtype == torch.bfloat16 and bottleneck_dim > BF16_MAX_BOTTLENECK:
        raise ValueError(f"bf16 activations need bottleneck_dim <= {BF16_MAX_BOTTLENECK} (got {bottleneck_dim}): the bf16 "
                         f"closing MLP kernels write at most {BF16_MAX_BOTTLENECK} columns; run a wider module on fp32 tensors")


def run_message_passing(mods: Sequence["_MessagePassing"], hs: Sequence[Tensor], Hs: Sequence, noises: Sequence,
                        outs: Sequence[Optional[Tensor]], traces=None, join=None, affinity=None,
                        fuse_closing: bool = False, n_agents=None) -> List[Tuple[Tensor, Tensor]]:
    """The message-passing rounds of SEVERAL modules over the same scenes, stage by stage, each stage
    ONE grouped launch (model/MS_HGNN_batch.py:174-195 and :425-441 for every module at once).

    mods[i] runs on hs[i] (B,N,64) with incidence Hs[i] (None = the implicit pairwise graph, a dense tensor, or an
    `ops.Incidence`: the dense tensor with its bit-mask form);
    noises[i] is None (draw), a tensor / PhiloxNoise, or a list of nmp_layers of them; outs[i]
    optionally receives node_feat.  Returns [(node_feat, factors)] per module.  All modules must
    share nmp_layers and bottleneck_dim (they do in every caller of the reference).
    Which launches the forward consists of and what each is asked to fuse is `route.message_passing_route`'s decision,
    taken once per call from the sizes, the storage type and the per-call switches; the stages below follow it.
    `traces` (training): one `backward.ModuleTrace` per module, which receives the node features entering
    every round and the dist every round sampled — all the backward needs besides the inputs.
    `join`: called once after the first node stage has been launched and before anything reads Hs (a caller that
    builds the incidences on a forked stream joins it here).
    `affinity`: an `ops.AffinityTail` — the deferred affinity + top-k launch that produces Hs; it rides in the first
    node-stage launch (its tail workgroups), or is issued beside it when that launch cannot take it.
    `fuse_closing`: let the typed-aggregation launch apply the closing MLP of every stage itself where its launch shape
    allows (`ops.agg_mlp_closing`: the launcher's plan decides): one launch fewer per stage, bit-identical rows.  At B = 512, N = 11 the chain costs
    inside that launch what the closing launch cost on its own (single-stream forward 0.104 -> 0.103 ms, 4-stream
    throughput -2 %): the block asks for it in its latency form only.
    The mask form: with it switched on (`masks_apply(N)`) and masks on EVERY hyper module's incidence, the stand-alone
    gather and scatter launches read the masks instead of H, and so does the node->edge launch where it takes its row
    form (bit-identical results) — in inference and in a training forward (`traces`, which receive the masks the step
    runs on: the backward reads them there, so both directions of a step run in one form); otherwise masks are
    ignored.
    `n_agents` (a ragged batch: `ops.agent_counts`; with `traces` only under `set_ragged_training`, the traces then
    receive the counts for the backward): scene b holds n_b <= N agents, its first rows, and
    Hs are the ragged incidences (zero rows and columns >= n_b).  The forward takes the ragged route: the node->edge
    launch and the scatter launch receive the counts, everything else is row-wise or meets the padding only through
    zeros of H, and ONE more launch zeroes the padded positions of every node_feat and factors at the end.  Counts that
    all equal N are no counts.  An `ops.StaticAgentCounts` (a captured graph's counts) keeps the ragged route whatever it
    holds and admits empty slots, n_b = 0: a second small launch then zeroes their single factor row of scale-N modules."""
    n = len(mods)
    if not (n == len(hs) == len(Hs) == len(noises) == len(outs)) or n == 0:
        raise ValueError("run_message_passing: one h, H, noise and out per module")
    nmp = mods[0].nmp_layers
    if any(m.nmp_layers != nmp or m.bottleneck_dim != mods[0].bottleneck_dim for m in mods):
        raise ValueError("grouped modules must share nmp_layers and bottleneck_dim")
    _check_storage_width(mods[0].bottleneck_dim, hs[0].dtype)
    B, N = hs[0].shape[0], hs[0].shape[1]
    counts = ops.agent_counts(n_agents, B, N, hs[0].device)
    ragged_train = counts is not None and traces is not None
    if ragged_train and not ragged_training():
        raise NotImplementedError("n_agents: ragged batches are inference-only")
    if ragged_train and counts.admits_empty and not trains_empty_slots():
        raise NotImplementedError("n_agents: counts that admit empty slots (ops.StaticAgentCounts) are inference-only")
    ragged = {} if counts is None else {"n_agents": counts}      # what the two count-aware launches are handed
    incs = [H if H is None or isinstance(H, ops.Incidence) else ops.Incidence(H) for H in Hs]
    rt = route.message_passing_route(
        N, tuple([(g is None, m.edge_types) for g, m in zip(incs, mods)]), twin=hs[0].dtype == torch.bfloat16,
        training=traces is not None, matrix16=ops.BF16X6,
        knobs=route.Knobs(_FUSE_POOL, ops.POOL_MAX_N, ops.node_form_enabled(),
                          ops.incidence_form() == "mask" and all(g is None or g.masks is not None for g in incs)),
        closing_asked=fuse_closing, ragged=counts is not None, ragged_training=ragged_train)
    # every module's graph as the ops item tuples take it: the dense H (None: pairwise), sym, the masks where the step
    # reads them.  The pairwise graph is symmetric: edges (i,j) and (j,i) pool the same feature, meet the same typed
    # MLP output and are summed into the same two nodes.  Its per-edge MLPs therefore run once per
    # unordered pair (N(N+1)/2 rows instead of N*N); only the Gumbel softmax runs per ordered edge.
    dense = [None if g is None else g.H for g in incs]
    syms = [g is None for g in incs]
    masks = [g.masks if g is not None and rt.masks else None for g in incs]
    Es = [N * N if H is None else H.shape[1] for H in dense]   # ordered edges: the shape of noise and factors
    if traces is not None:
        for t, mk in zip(traces, masks):
            t.masks = mk
            t.counts = counts
    given = [_noise_iter(u) for u in noises]

    def next_u(i: int):
        if given[i] is not None:
            try:
                return next(given[i])
            except StopIteration:
                raise ValueError(f"noise_u: {nmp} uniform tensors of shape ({B},{Es[i]},{mods[i].edge_types}) needed")
        return _draw_uniform((B, Es[i], mods[i].edge_types), hs[i].device)

    def node2edge(xs: Sequence[Tensor], idx: int) -> Tuple[List, List[Optional[Tensor]]]:
        """-> per module the edge MLP's rows (an `edges` tensor or a PoolSpec) and the typed MLP's per-node first layer
        A (None where the route does not form it)."""
        pks = [m._packed_n2e(idx) for m in mods]
        keep = [] if traces is not None else None
        # the node rows entering this round also feed the typed aggregation MLP that closes it: its first layer runs
        # in this same launch where the route says so
        aggs = [m.edge_aggregation_list[idx] for m in mods]
        specs = [(a._packed(), a.edge_types) if r.first_layer else None for a, r in zip(aggs, rt.modules)]
        xpq, As = ops.node_stage_grouped([(x, pk) for x, pk in zip(xs, pks)], keep, specs,
                                         affinity if idx == 0 else None)
        if join is not None and idx == 0:
            join()       # the incidences were built on a forked stream beside the node stage (graph capture)
        edges: List = [None] * n
        if rt.node2edge:
            for i, e in zip(rt.node2edge, ops.node2edge_grouped([(xpq[i][0], xpq[i][1], dense[i], pks[i]["w2"], pks[i]["b2"],
                                                                  syms[i], masks[i]) for i in rt.node2edge], **ragged)):
                edges[i] = e
        for i, r in enumerate(rt.modules):
            if r.pool_in_edge_kernel:
                edges[i] = ops.PoolSpec(xpq[i][0], xpq[i][1], dense[i], pks[i]["w2"], pks[i]["b2"], syms[i])
        if traces is not None:      # kept for the backward: nothing of this round is re-computed there
            for t, kd, (xp, pq), e in zip(traces, keep, xpq, edges):
                t.n2e.append(dict(x1=kd["hid"], xp=xp, pq=pq, edges=e))
        return edges, As

    def edge_mlp(stages, edges: Sequence[Tensor], want_dist: bool):
        # draws happen module by module, in the order given — the reference's RNG order per call site
        us = [next_u(i) for i in range(n)]
        keep = [] if traces is not None else None
        res = ops.edge_mlp_gumbel_grouped([(e, u, st._packed(), st.bottleneck_dim, N if sy else 0, want_dist)
                                           for e, u, st, sy in zip(edges, us, stages, syms)], _GUMBEL_TAU, keep)
        if traces is not None:
            for t, kd in zip(traces, keep):
                t.estage.append(kd)
        return res

    def edge2node(edge_feats: Sequence[Tensor], oris: Sequence[Tensor], As: Sequence[Optional[Tensor]], idx: int,
                  closing: Sequence[Tuple[dict, Optional[Tensor]]]) -> Tuple[Optional[List[Tensor]], Optional[List]]:
        """-> (None, the inputs of the stage's closing MLPs: tensors / ScatterSpec / NodeAggSpec), or (the closing MLPs'
        OUTPUTS, None) where the route asks the aggregation launch to apply them itself — ``closing`` = (packed MLP, out
        or None) per module — and its launch shape allows it."""
        aggs = [m.edge_aggregation_list[idx] for m in mods]
        # larger graphs: eo = H @ ori of every hyper module from ONE stand-alone gather launch
        eos = dict(zip(rt.gather, ops.agg_gather_grouped([(oris[i], dense[i], syms[i], masks[i]) for i in rt.gather]))) if rt.gather else {}
        items = []
        for i, r in enumerate(rt.modules):
            if r.first_layer:
                src = ops.PairSpec(As[i], node=r.node_form)
            elif r.source == route.EO:
                src = eos[i]
            else:       # eo formed inside the kernel: H @ ori, or the twins' ori_i + ori_j per node or per unordered pair
                src = ops.GatherSpec(oris[i], dense[i], syms[i], node=r.node_form)
            items.append((src, edge_feats[i], aggs[i]._packed(), aggs[i].edge_types))
        if rt.ask_closing and len({(-1 if o is None else o.stride(-2)) for _, o in closing}) == 1:
            closed = ops.agg_mlp_closing(items, [(pk2, o, ori) for (pk2, o), ori in zip(closing, oris)])
            if closed is not None:
                return closed, None
        feats = ops.agg_mlp_grouped(items)
        # larger graphs: one stand-alone scatter launch for the modules whose aggregation wrote per-edge features
        scat = dict(zip(rt.scatter, ops.agg_scatter_grouped([(feats[i], dense[i], oris[i], syms[i], masks[i]) for i in rt.scatter], **ragged))) if rt.scatter else {}
        # cat(H^T feat, ori) / N is formed inside the MLP kernel that consumes it (node form: H^T feat is what the
        # aggregation kernel wrote), or is the scatter launch's output
        return None, [ops.NodeAggSpec(feats[i], oris[i]) if r.closing_input == route.NODE_AGG else
                      ops.ScatterSpec(feats[i], dense[i], oris[i], syms[i]) if r.closing_input == route.SCATTER_SPEC else
                      scat[i] for i, r in enumerate(rt.modules)]

    edges, As = node2edge(hs, 0)
    res = edge_mlp([m.nmp_mlp_start for m in mods], edges, True)
    edge_feats, factors = [r[0] for r in res], [r[1] for r in res]
    if traces is not None:
        for t, r in zip(traces, res):
            t.dists.append(r[1])
    node_feats, idx = list(hs), 0
    for l in range(2 * (nmp - 1)):
        stages = [m.nmp_mlps[l] for m in mods]
        if l % 2 == 0:
            closed, agg = edge2node(edge_feats, node_feats, As, idx,
                                    [(m._packed_mlp2(st), None) for m, st in zip(mods, stages)])
            keep = [] if traces is not None else None
            node_feats = (closed if closed is not None else
                          ops.mlp2_grouped([(a, m._packed_mlp2(st), None) for a, m, st in zip(agg, mods, stages)], keep))
            idx += 1
            if traces is not None:
                for t, x, kd in zip(traces, node_feats, keep):
                    t.xs.append(x)
                    t.tails.append(kd)
        else:
            edges, As = node2edge(node_feats, idx)
            res = edge_mlp(stages, edges, traces is not None)
            edge_feats = [r[0] for r in res]
            if traces is not None:
                for t, r in zip(traces, res):
                    t.dists.append(r[1])
    closed, agg = edge2node(edge_feats, node_feats, As, idx,
                            [(m._packed_mlp2(m.nmp_mlp_end), o) for m, o in zip(mods, outs)])
    if closed is not None:
        return list(zip(closed, factors))
    ends = [(a, m._packed_mlp2(m.nmp_mlp_end), o) for a, m, o in zip(agg, mods, outs)]
    # the last MLP writes in place when `out` is given; grouped when every group has the same stride
    strides = {(-1 if o is None else o.stride(-2)) for o in outs}
    keep = [] if traces is not None else None
    if len(strides) == 1:
        node_feats = ops.mlp2_grouped(ends, keep)
    else:
        node_feats = [ops.mlp2_grouped([e], keep)[0] for e in ends]
    if traces is not None:
        for t, kd in zip(traces, keep):
            t.tails.append(kd)
    if counts is not None:      # the padded rows of the outputs went through the row-wise stages: zero them, one launch
        ops.zero_padding([(x, ops.ZERO_NODE_ROWS) for x in node_feats] +
                         [(fc, ops.ZERO_PAIR_ROWS if H is None else ops.ZERO_EDGE_ROWS) for fc, H in zip(factors, dense)],
                         counts)
        if counts.admits_empty:      # an empty slot: the single row of a scale-N module is not padding, yet must be zeros
            ops.zero_empty_scenes([fc for fc, H in zip(factors, dense) if H is not None and fc.shape[1] == 1], counts)
    return list(zip(node_feats, factors))


class MS_HGNN_oridinary(_MessagePassing):
    """Pairwise (fully connected, self-loops included) message passing — drop-in for the reference
    class of the same (misspelt) name, model/MS_HGNN_batch.py:55-198.  ``forward(h_states)`` ->
    ``(node_feat (B,N,bottleneck), factors (B,N*N,6))``.  The N^2 x N incidence the reference
    rebuilds with numpy on every call (:143-160) is never materialised."""

    def __init__(self, embedding_dim=64, h_dim=64, mlp_dim=1024, bottleneck_dim=1024, activation='relu',
                 batch_norm=True, dropout=0.0, nmp_layers=4, vis=False):
        super().__init__()
        self.mlp_dim = mlp_dim
        self.h_dim = h_dim
        self.bottleneck_dim = bottleneck_dim
        self.embedding_dim = embedding_dim
        self.nmp_layers = nmp_layers
        self.batch_norm = batch_norm
        self.activation = activation
        self.vis = vis
        self.hdim_extend = _HDIM_EXTEND
        self.edge_types = 6   # model/MS_HGNN_batch.py:74
        self._build(h_dim, bottleneck_dim, nmp_layers)

    # reference-named stage methods (rel_rec / rel_send are accepted and ignored: the graph is implicit)
    def node2edge(self, x, rel_rec=None, rel_send=None, idx=0):
        return self._node2edge(x, None, idx)

    def edge2node(self, x, rel_rec, rel_send, ori, idx):
        return self._edge2node(x, ori, None, idx)

    def forward(self, h_states, noise_u=None, out=None, n_agents=None):
        """``out`` (optional): where node_feat is written, e.g. a column block of the caller's
        concatenated feature tensor.  Under autograd (an input or a parameter requires grad) the call
        goes through `groupnet_amd.backward.MSHGNNFunction`: same fused forward, HIP backward.
        ``n_agents`` (optional; INTEGRATION.md, "Ragged batches"): one count per scene, 1 <= n_b <= N — the first n_b
        agent rows of scene b are real, the rest is (finite) padding.  Valid node rows and edges (i, j < n_b; the noise
        is read at the padded index i*N + j) are what the module computes for the scene alone; padded positions of both
        outputs are zeros.  Under autograd only with `set_ragged_training(True)` ("Ragged batches",
        Training): the input gradient then comes back with rows n >= n_b exactly zero."""
        ops._req(h_states, "h_states", (None, None, self.h_dim), ops._ACT_DTYPES)
        N = h_states.shape[1]
        grad = _needs_grad(self, h_states)
        sub = subset_of(n_agents, h_states, grad)
        if sub is not None:
            return self._forward_subset(h_states, noise_u, out, sub, grad)
        n_agents = ragged_counts(n_agents, h_states, **ragged_grad_refusals(grad, N))
        if h_states.shape[0] and N and grad:
            return self._forward_autograd(h_states, None, noise_u, out, n_agents)
        _check_storage_width(self.bottleneck_dim, h_states.dtype)
        if h_states.shape[0] == 0 or N == 0:      # empty batch: nothing to launch
            nf = out if out is not None else h_states.new_empty((h_states.shape[0], N, self.bottleneck_dim))
            return nf, h_states.new_empty((h_states.shape[0], N * N, self.edge_types))
        return self._run(h_states, None, N * N, noise_u, out, n_agents)

    def _forward_subset(self, h: Tensor, noise_u, out: Optional[Tensor], sub: "ops.AgentSubset", grad: bool):
        """``n_agents`` = an `ops.AgentSubset` ("Agents missing anywhere"): ONE launch compacts the
        features and the noise tensors of every round into scratch, the ragged forward runs on them as with
        ``n_agents=<counts>``, ONE launch expands node_feat and factors to the original slots and zeroes the rest.
        Invalid input rows are never read.  Under autograd the two launches are `_Remap` nodes."""
        B, N = h.shape[0], h.shape[1]
        if grad and out is not None:
            raise ValueError("out= is an inference-time extra; under autograd the module returns a new tensor")
        _check_subset_out(out, h, self.bottleneck_dim)
        us = subset_noise(noise_u, (B, N * N, self.edge_types), self.nmp_layers, h.device)
        items: list = []
        uc = remap_noise(us, ops.REMAP_PAIR_ROWS, items)
        if grad:
            if items:
                ops.remap_rows(items, sub.order)
            (hc,) = _Remap.apply(sub, False, (ops.REMAP_NODE_ROWS,), h)
            nf, fac = self.forward(hc, noise_u=uc, n_agents=sub.compacted)
            return _Remap.apply(sub, True, (ops.REMAP_NODE_ROWS, ops.REMAP_PAIR_ROWS), nf, fac)
        hc = torch.empty_like(h)
        ops.remap_rows([(h, hc, ops.REMAP_NODE_ROWS)] + items, sub.order)
        nfc, facc = self.forward(hc, noise_u=uc, n_agents=sub.compacted)
        nf = out if out is not None else torch.empty_like(nfc)
        fac = torch.empty_like(facc)
        ops.remap_rows([(nfc, nf, ops.REMAP_NODE_ROWS), (facc, fac, ops.REMAP_PAIR_ROWS)], sub.slot)
        return nf, fac


class MS_HGNN_hyper(_MessagePassing):
    """Top-k hypergraph message passing at one group size — drop-in for
    model/MS_HGNN_batch.py:270-443 (listall=False, the only mode the reference runs, :312).
    ``forward(h_states, corr)`` -> ``(node_feat (B,N,bottleneck), factor (B,E,10), H (B,E,N))``
    with E = 1 when scale == N, else N."""

    def __init__(self, embedding_dim=64, h_dim=64, mlp_dim=1024, bottleneck_dim=1024, activation='relu',
                 batch_norm=True, dropout=0.0, nmp_layers=4, scale=2, vis=False, actor_number=11):
        super().__init__()
        self.mlp_dim = mlp_dim
        self.h_dim = h_dim
        self.bottleneck_dim = bottleneck_dim
        self.embedding_dim = embedding_dim
        self.nmp_layers = nmp_layers
        self.batch_norm = batch_norm
        self.activation = activation
        self.scale = scale
        self.vis = vis
        # never used by forward, present in reference checkpoints (model/MS_HGNN_batch.py:290-291)
        self.spatial_embedding = nn.Linear(2, embedding_dim)
        self.spatial_transform = nn.Linear(h_dim, h_dim)
        self.hdim_extend = _HDIM_EXTEND
        self.edge_types = 10  # model/MS_HGNN_batch.py:294
        self._build(h_dim, bottleneck_dim, nmp_layers)
        self.listall = False

    def init_adj_attention(self, feat, feat_corr, scale_factor=2, n_agents=None):
        """H (B,E,N) from the affinity matrix (model/MS_HGNN_batch.py:372-388).  ``n_agents``: the incidence of a
        ragged batch (`ops.topk_incidence`)."""
        if feat_corr.dtype == torch.bfloat16:     # ranked in fp32 either way; fp32 corr keeps near-ties apart
            feat_corr = feat_corr.float()
        ops._req(feat_corr, "corr", (feat.shape[0], feat.shape[1], feat.shape[1]))
        return ops.topk_incidence(feat_corr, [int(scale_factor)], n_agents)[0]

    def init_adj_attention_listall(self, feat, feat_corr, scale_factor=2):
        """H (B,E,N) by exhaustive search of the best group per agent (model/MS_HGNN_batch.py:390-414);
        used by forward when ``self.listall`` is set (hard-coded False in the reference, :312)."""
        ops._req(feat_corr, "corr", (feat.shape[0], feat.shape[1], feat.shape[1]))
        return ops.listall_incidence(feat_corr, int(scale_factor))

    def _build_H(self, h_states, corr):
        build = self.init_adj_attention_listall if self.listall else self.init_adj_attention
        return build(h_states, corr, scale_factor=self.scale)

    def node2edge(self, x, H, idx=0):
        return self._node2edge(x, H, idx)

    def edge2node(self, x, ori, H, idx):
        return self._edge2node(x, ori, H, idx)

    def forward(self, h_states, corr, noise_u=None, H=None, out=None, masks=None, n_agents=None):
        """``H`` (optional) lets a caller that already built the incidence for every scale in one
        fused launch (``ops.affinity_topk``) hand it in; by default it is built here from ``corr``.
        ``masks`` (optional): the `ops.IncidenceMasks` of a caller-supplied ``H``, used when the mask form is
        switched on (`masks_apply`); an ``H`` handed in without them stays dense (it may carry other weights than 0/1),
        an ``H`` built here gets its masks from the builder.
        ``n_agents`` (optional; INTEGRATION.md, "Ragged batches"): one count per scene, 1 <= n_b <= N.  Row i < n_b of
        H holds the top-min(scale, n_b) of corr[b, i, :n_b], a module with scale == N (the padded size) has its one
        hyperedge hold the n_b valid agents; a scene with n_b <= scale < N gets n_b identical all-member hyperedges (the
        E = 1 shortcut is keyed on N).  Valid rows of node_feat and factor are what the module computes for the scene
        alone; padded positions of the three outputs are zeros; padded rows of h_states and corr must be finite.
        Top-k incidence built here only (no ``H=`` / ``masks=``, no ``listall``); under autograd only with
        `set_ragged_training(True)` ("Ragged batches", Training)."""
        ops._req(h_states, "h_states", (None, None, self.h_dim), ops._ACT_DTYPES)
        grad = _needs_grad(self, h_states)
        sub = subset_of(n_agents, h_states, grad, handed_in=H is not None or masks is not None, listall=self.listall)
        if sub is not None:
            return self._forward_subset(h_states, corr, noise_u, out, sub, grad)
        n_agents = ragged_counts(n_agents, h_states, handed_in=H is not None or masks is not None, listall=self.listall,
                                 **ragged_grad_refusals(grad, h_states.shape[1]))
        if n_agents is not None:
            if self.scale > h_states.shape[1]:
                raise RuntimeError("selected index k out of range")
            if grad:
                # the ragged incidence is a constant of the backward, as H is on the full-batch training path
                H = self.init_adj_attention(h_states.detach(), corr.detach(), scale_factor=self.scale, n_agents=n_agents)
                node_feat, factor = self._forward_autograd(h_states, ops.Incidence(H), noise_u, out, n_agents)
                return node_feat, factor, (H if H.dtype == h_states.dtype else H.to(h_states.dtype))
            _check_storage_width(self.bottleneck_dim, h_states.dtype)
            H = self.init_adj_attention(h_states, corr, scale_factor=self.scale, n_agents=n_agents)
            node_feat, factor = self._run(h_states, ops.Incidence(H), H.shape[1], noise_u, out, n_agents)
            return node_feat, factor, (H if H.dtype == h_states.dtype else H.to(h_states.dtype))
        if h_states.shape[0] and _needs_grad(self, h_states):
            # H is a constant of the backward (top-k selection has no gradient; corr is only used to build it)
            if H is None:
                H = self._build_H(h_states.detach(), corr.detach())
                masks = ops.incidence_masks(H, assume_binary=True) if masks_apply(h_states.shape[1]) else None
            node_feat, factor = self._forward_autograd(h_states, ops.Incidence(H, masks), noise_u, out)
            return node_feat, factor, H
        _check_storage_width(self.bottleneck_dim, h_states.dtype)      # (before the incidence is built)
        if h_states.shape[0] == 0:                  # empty batch: nothing to launch
            B, N = h_states.shape[0], h_states.shape[1]
            if self.scale > N:
                raise RuntimeError("selected index k out of range")
            E = 1 if self.scale == N else N
            nf = out if out is not None else h_states.new_empty((B, N, self.bottleneck_dim))
            return nf, h_states.new_empty((B, E, self.edge_types)), h_states.new_empty((B, E, N))
        if H is None:
            H = self._build_H(h_states, corr)
            masks = ops.incidence_masks(H, assume_binary=True) if masks_apply(h_states.shape[1]) else None
        else:
            ops._req(H, "H", (h_states.shape[0], None, h_states.shape[1]))
        node_feat, factor = self._run(h_states, ops.Incidence(H, masks), H.shape[1], noise_u, out)
        return node_feat, factor, (H if H.dtype == h_states.dtype else H.to(h_states.dtype))    # type_as(feat), :376,384

    def _forward_subset(self, h: Tensor, corr: Tensor, noise_u, out: Optional[Tensor], sub: "ops.AgentSubset", grad: bool):
        """``n_agents`` = an `ops.AgentSubset`: as `MS_HGNN_oridinary._forward_subset`, with the caller's ``corr``
        compacted as a matrix of ordered pairs and H expanded with the other two results.  Hyperedge rows of a top-k
        module (factor, rows of H, the noise) move like node rows; the single row of a scale-N module stays."""
        B, N = h.shape[0], h.shape[1]
        if self.scale > N:
            raise RuntimeError("selected index k out of range")
        if grad and out is not None:
            raise ValueError("out= is an inference-time extra; under autograd the module returns a new tensor")
        _check_subset_out(out, h, self.bottleneck_dim)
        ops._req(corr, "corr", (B, N, N), ops._ACT_DTYPES)
        rows = ops.REMAP_NODE_ROWS if self.scale != N else None      # E = N hyperedge rows, or the one row that stays
        us = subset_noise(noise_u, (B, 1 if self.scale == N else N, self.edge_types), self.nmp_layers, h.device)
        cc = torch.empty_like(corr)
        items: list = [(corr.detach(), cc, ops.REMAP_PAIR_ROWS)]
        uc = remap_noise(us, rows, items)
        if grad:
            ops.remap_rows(items, sub.order)
            (hc,) = _Remap.apply(sub, False, (ops.REMAP_NODE_ROWS,), h)
            nfc, facc, Hc = self.forward(hc, cc, noise_u=uc, n_agents=sub.compacted)
            fac_kind = ops.REMAP_NODE_ROWS if rows is not None else None
            if fac_kind is None:
                (nf,), fac = _Remap.apply(sub, True, (ops.REMAP_NODE_ROWS,), nfc), facc
            else:
                nf, fac = _Remap.apply(sub, True, (ops.REMAP_NODE_ROWS, fac_kind), nfc, facc)
            H = torch.empty_like(Hc)
            ops.remap_rows([incidence_item(Hc, H)], sub.slot)
            return nf, fac, H
        hc = torch.empty_like(h)
        ops.remap_rows([(h, hc, ops.REMAP_NODE_ROWS)] + items, sub.order)
        nfc, facc, Hc = self.forward(hc, cc, noise_u=uc, n_agents=sub.compacted)
        nf = out if out is not None else torch.empty_like(nfc)
        H = torch.empty_like(Hc)
        back = [(nfc, nf, ops.REMAP_NODE_ROWS), incidence_item(Hc, H)]
        fac = facc
        if rows is not None:
            fac = torch.empty_like(facc)
            back.append((facc, fac, ops.REMAP_NODE_ROWS))
        ops.remap_rows(back, sub.slot)
        return nf, fac, H
