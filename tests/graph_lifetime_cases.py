"""Test helper: what can change under a captured graph, as tables (no GPU needed).

A captured inference forward (`graphs.GraphedMultiScale`, `graphs.GraphedPastEncoder`) holds no packing launch: it reads
the packed weight images where they lay at capture, and `refresh_weights()` re-derives them in place.  The tables below
name the CONFIGURATIONS that are captured (one capture each), the parameter FAMILIES that are changed one at a time (a
refresh that misses one image family leaves exactly one of them stale), and the training CASES whose every replay is
held against an eager twin.  tests/test_graph_lifetime_cpu.py checks on the float64 oracle that the family table names
every parameter of a block and of an encoder exactly once and that every single-family change is far above the
tolerance; tests/test_graph_lifetime_gpu.py runs the tables.
"""
import contextlib
import re
import types
from collections import namedtuple

import torch

from oracle import ms_hgnn_oracle as O
from oracle import past_encoder_oracle as PO

TOL = 1e-5                    # test_parity_gpu.TOL (north_star: fp32 features within 1e-5)
VISIBLE = 100 * TOL           # what one family's change must move the float64 oracle's output by, at least
SEED = 2468                   # Philox seed of every capture of part A
# see make_block: every weight matrix x this.  The {2,5,11} block is the one held against the float64 oracle within TOL, a
# bound meant for features of O(1): x1.5 keeps them there even after item 2's x1.5 on every parameter (max 0.5 -> 3.9)
WEIGHT_GAIN = {(2, 5, 11): 1.5}
WEIGHT_GAIN_ELSE = 2.0

# ---- part A: the captured configurations ---------------------------------------------------------------------------------
# precision: through ops.set_precision (None: the default, f16x3); tail: `affinity_tail` of the capture (True = the
# latency form, which reads the fused-closing images); form: ops.set_incidence_form; counts: ragged=True with these
# counts; kind: "block" (GraphedMultiScale) or "encoder" (GraphedPastEncoder, T = 5).
Config = namedtuple("Config", "id kind B N scales nmp precision bf16 tail form counts")
CONFIGS = [
    Config("f16x3-latency", "block", 5, 11, (2, 5, 11), 1, None, False, True, None, None),
    Config("f16x3-throughput", "block", 5, 11, (2, 5, 11), 1, None, False, False, None, None),
    Config("bf16x6", "block", 5, 11, (2, 5, 11), 1, "bf16x6", False, True, None, None),
    Config("fp32", "block", 5, 11, (2, 5, 11), 1, "fp32", False, True, None, None),
    Config("bf16-storage", "block", 5, 11, (2, 5, 11), 1, None, True, True, None, None),
    Config("mask-standalone", "block", 3, 17, (4, 17), 1, None, False, True, "mask", None),
    Config("nmp2", "block", 3, 7, (3, 7), 2, None, False, True, None, None),
    Config("ragged", "block", 5, 11, (2, 5, 11), 1, None, False, True, None, (11, 7, 3, 11, 1)),
    Config("encoder", "encoder", 3, 11, (5, 11), 1, None, False, None, None, None),
]
CONFIG_BY_ID = {c.id: c for c in CONFIGS}
ENCODER_T = 5

# ---- the parameter families -------------------------------------------------------------------------------------------
# pattern: on a parameter's name RELATIVE to its module (pairwise or hyper) — or, `top`, on the encoder's front-end name;
# one_type: the pattern's group 1 is the edge type and the change touches this type only; factor: p <- p * factor;
# dead: parameters the forward never reads (kept for state_dict parity with the reference) — a change moves nothing;
# nmp2: exists only with nmp_layers > 1.
Family = namedtuple("Family", "id pattern top one_type factor dead nmp2")
AGG_TYPE = 2
_F = lambda id, pattern, top=False, one_type=None, factor=1.5, dead=False, nmp2=False: Family(
    id, re.compile(pattern), top, one_type, factor, dead, nmp2)
FAMILIES = [
    # (x1.5 of these four moves a hyper module of the {2,5,11} block by 6e-4 .. 1e-3 only: enlarged)
    _F("node-l0", r"node2edge_start_mlp\.\d+\.layers\.0\.", factor=4.0),
    _F("node-l1", r"node2edge_start_mlp\.\d+\.layers\.1\.", factor=4.0),
    _F("att-l0", r"attention_mlp\.\d+\.layers\.0\.", factor=8.0),
    _F("att-l1", r"attention_mlp\.\d+\.layers\.1\.", factor=8.0),
    _F("init", r"nmp_mlp_start\.init_MLP\."),
    _F("dist", r"nmp_mlp_start\.MLP_distribution\."),
    _F("factor", r"nmp_mlp_start\.MLP_factor\."),
    _F("agg-l0", r"edge_aggregation_list\.\d+\.agg_mlp\.(\d+)\.layers\.0\.", one_type=AGG_TYPE),
    _F("agg-l1", r"edge_aggregation_list\.\d+\.agg_mlp\.(\d+)\.layers\.1\.", one_type=AGG_TYPE),
    _F("end-l0", r"nmp_mlp_end\.layers\.0\."),
    _F("end-l1", r"nmp_mlp_end\.layers\.1\."),
    _F("rounds", r"nmp_mlps\.", nmp2=True),
    _F("unread", r"edge_aggregation_list\.\d+\.mlp\.|spatial_embedding\.|spatial_transform\.", dead=True),
    _F("input_fc", r"input_fc\.", top=True),
    _F("input_fc2", r"input_fc2\.", top=True),
    _F("input_fc3", r"input_fc3\.", top=True),
    _F("pos-fc", r"pos_encoder\.fc\.", top=True),
]
FAMILY_BY_ID = {f.id: f for f in FAMILIES}
_MODULE = re.compile(r"(interaction(?:_hyper\d*(?:\.\d+)?)?)\.(.*)$")


def split_name(name):
    """'interaction_hyper.0.x.y' -> ('interaction_hyper.0', 'x.y'); a front-end parameter -> (None, name)."""
    m = _MODULE.match(name)
    return (m.group(1), m.group(2)) if m else (None, name)


def families_of(name):
    """The families whose pattern names the parameter `name` (the table is complete iff this is always one)."""
    mod, rel = split_name(name)
    return [f for f in FAMILIES if f.top == (mod is None) and f.pattern.match(rel)]


def family_members(names, module, family):
    """The parameters of `module` (None: the encoder's front-end) that a change of `family` touches."""
    out = []
    for n in names:
        mod, rel = split_name(n)
        m = family.pattern.match(rel)
        if mod == module and m and family.top == (mod is None):
            if family.one_type is None or int(m.group(1)) == family.one_type:
                out.append(n)
    return out


def modules_under_test(cfg):
    """The pairwise module and ONE hyper module (the first), by their prefix in the parameter names."""
    return ["interaction", "interaction_hyper" if cfg.kind == "encoder" else "interaction_hyper.0"]


def family_changes(cfg, names, dead=False):
    """[(tag, family, parameter names)] of item 5 for a configuration: every live family of the pairwise module and of one
    hyper module, and the front-end families of the encoder."""
    out = []
    for f in FAMILIES:
        if f.dead != dead or (f.nmp2 and cfg.nmp == 1) or (f.top and cfg.kind != "encoder"):
            continue
        for mod in ([None] if f.top else modules_under_test(cfg)):
            members = family_members(names, mod, f)
            assert members, (cfg.id, f.id, mod)
            out.append((f"{mod or 'front'}:{f.id}", f, members))
    return out


def scale_(params, names, factor):
    """p <- p * factor IN PLACE through .data (no version bump: what a hand-written optimizer does)."""
    with torch.no_grad():
        for n in names:
            params[n].data.mul_(factor)


@contextlib.contextmanager
def scaled(params, names, factor):
    """`scale_` for the body, the exact old values (written in place) afterwards."""
    saved = {n: params[n].detach().clone() for n in names}
    scale_(params, names, factor)
    try:
        yield
    finally:
        with torch.no_grad():
            for n, v in saved.items():
                params[n].data.copy_(v)


# ---- the models ---------------------------------------------------------------------------------------------------------
def make_block(cfg, seed=0):
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(100 + seed)
    blk = MultiScaleHGNN(list(cfg.scales), nmp_layers=cfg.nmp).eval()
    with torch.no_grad():      # default init: features of 0.1 on which the attention layers are all but invisible (a x1.5
        for n, p in blk.named_parameters():     # change of them moves 1e-7 .. 1e-5); a gain per matrix: features of O(1)
            if n.endswith(".weight") and p.dim() == 2:
                p.mul_(WEIGHT_GAIN.get(tuple(cfg.scales), WEIGHT_GAIN_ELSE))
    return blk


def make_encoder(cfg, seed=0):
    from groupnet_amd.past_encoder import PastEncoder
    torch.manual_seed(200 + seed)
    enc = PastEncoder(types.SimpleNamespace(hidden_dim=64, hyper_scales=list(cfg.scales), past_length=ENCODER_T)).eval()
    with torch.no_grad():      # default init gives an almost constant embedding; spread it out (as test_past_encoder)
        for p in (enc.input_fc.weight, enc.input_fc2.weight, enc.input_fc3.weight, enc.pos_encoder.fc.weight):
            p.mul_(3.0)
    return enc


def make_model(cfg, seed=0):
    return make_encoder(cfg, seed) if cfg.kind == "encoder" else make_block(cfg, seed)


def make_inputs(cfg, seed=0):
    g = torch.Generator().manual_seed(300 + seed)
    if cfg.kind == "encoder":
        B, N, T = cfg.B, cfg.N, ENCODER_T
        traj = torch.cumsum(torch.randn(B * N, T, 2, generator=g), dim=1) + torch.rand(B * N, 1, 2, generator=g) * 20
        vel = traj[:, 1:] - traj[:, :-1]
        return torch.cat((traj, torch.cat([vel[:, [0]], vel], dim=1)), dim=-1)
    return torch.randn(cfg.B, cfg.N, 64, generator=g)


# ---- the float64 oracle at a Philox position ------------------------------------------------------------------------------
def edge_types(model, kind):
    hyper = model.interaction_hyper if kind == "encoder" else model.interaction_hyper[0]
    return model.interaction.edge_types, hyper.edge_types


def philox_noise(shapes, rounds, seed, position):
    """The uniforms of one forward at stream position `position`, laid out module-major as `multiscale.draw_noise` draws
    them: every round of the pairwise module, then scale by scale.  -> per module a list of `rounds` (B,E,K) tensors."""
    out, pos = [], position
    for (b, e, k) in shapes:
        us = []
        for _ in range(rounds):
            us.append(torch.from_numpy(O.philox_uniform(b * e * k, seed, pos)).view(b, e, k))
            pos += b * e * k
        out.append(us)
    return out, pos - position


def noise_shapes(cfg, kp, kh):
    B, N = cfg.B, cfg.N
    return [(B, N * N, kp)] + [(B, 1 if s == N else N, kh) for s in cfg.scales]


def _cast64(st):
    return {k: v.detach().double() for k, v in st.items()}


def oracle64(cfg, state, x, noise):
    """The model's output in float64 from a state_dict, CPU inputs and the uniforms of `philox_noise`.  The incidences are
    ranked on the fp32 affinity, as the kernels rank them; everything after them is float64."""
    B, N, nmp = cfg.B, cfg.N, cfg.nmp
    sub = lambda pre: _cast64({k[len(pre):]: v for k, v in state.items() if k.startswith(pre)})
    if cfg.kind == "encoder":
        f = PO.embed(_cast64({k: v for k, v in state.items() if not k.startswith("interaction")}), x.double(), B, N)
        hyper = ["interaction_hyper.", "interaction_hyper2.", "interaction_hyper3."]
    else:
        f = x.double()
        hyper = [f"interaction_hyper.{i}." for i in range(len(cfg.scales))]
    corr = O.affinity(f.float())
    u64 = lambda us: [u.double() for u in us]
    feats = [f, O._message_passing(sub("interaction."), f, O.pairwise_incidence(N, B, torch.float64), u64(noise[0]), nmp,
                                   True, None)[0]]
    for pre, s, us in zip(hyper, cfg.scales, noise[1:]):
        H = O.topk_incidence(corr, s, like=f.float()).double()
        feats.append(O._message_passing(sub(pre), f, H, u64(us), nmp, True, None)[0])
    return torch.cat(feats, dim=-1)


# ---- part B: every replay of a training graph ---------------------------------------------------------------------------
# lr: chosen so that a step from the one-step-stale weights is far outside the gate in every family (asserted on the GPU,
# eager against eager); `form`: ops.set_incidence_form during capture, replays and the eager twin.
TrainCase = namedtuple("TrainCase", "id opt B N scales nmp lr form")
TRAIN_CASES = [
    TrainCase("sgd-momentum", "sgd", 6, 11, (2, 5, 11), 1, 0.05, None),
    TrainCase("adam-capturable", "adam", 4, 7, (3, 7), 2, 0.01, None),
    TrainCase("sgd-mask-form", "sgd0", 3, 17, (4, 17), 1, 0.05, "mask"),
]
TRAIN_BY_ID = {c.id: c for c in TRAIN_CASES}
TRAIN_K = 4
TRAIN_SEED = 1357
SPREAD_MARGIN = 8             # gate = margin x the spread of two eager runs of one step (atomics reorder the sums)
STALE_POWER = 10              # a step from the one-step-stale state must differ by this many gates
ORACLE_MARGIN = 4
# measured on MI355X (tests/test_graph_lifetime_gpu.py prints every run's figures):
# the spread of two eager runs of one step, max over tensors and replays of max |u_A - u_B| / max |u_A| ...
# (a parameter's difference less one fp32 spacing of the weight, see the test's `_rel`; with plain or momentum SGD a
# parameter moves by lr x the buffer, so its spread is the buffer's: measured 0 once the spacing is taken off)
UPDATE_SPREAD = {"sgd-momentum": {"param": 1.0e-6, "momentum_buffer": 1.0e-6},
                 "adam-capturable": {"param": 1.9e-6, "exp_avg": 1.6e-6, "exp_avg_sq": 2.4e-6},
                 "sgd-mask-form": {"param": 7.3e-8}}      # (1.2e-8 at lr = 0.05, 7.3e-8 at lr = 0.5)
# ... and max over steps of |eager loss - float64 oracle trajectory's loss| / loss, first case
ORACLE_LOSS_DISTANCE = 9.3e-8


def make_optimizer(case, params):
    if case.opt == "adam":
        # eps: with the default 1e-8 an element whose gradient is rounding noise (1e-10) still moves by a full lr, its
        # sign decided by the order of the atomics; 1e-5 keeps the update a well-conditioned function of the gradient
        return torch.optim.Adam(params, lr=case.lr, eps=1e-5, capturable=True)
    return torch.optim.SGD(params, lr=case.lr, momentum=0.9 if case.opt == "sgd" else 0.0)


def train_batches(case, width):
    """K + 1 different (f, target) pairs: one per replay and one for the eager step taken between two replays."""
    g = torch.Generator().manual_seed(77)
    return [(torch.randn(case.B, case.N, 64, generator=g), torch.randn(case.B, case.N, width, generator=g))
            for _ in range(TRAIN_K + 1)]


def train_family(name):
    """Family of a trained parameter (the unread ones receive no gradient and never move)."""
    fs = families_of(name)
    return fs[0].id if fs else None


# ---- part C: side-by-side replays -----------------------------------------------------------------------------------------
SideCase = namedtuple("SideCase", "id B N scales bf16")
SIDE_CASES = [SideCase("fp32", 512, 11, (2, 5, 11), False), SideCase("bf16", 64, 50, (2, 4, 8, 16), True)]
SIDE_GRAPHS, SIDE_ROUNDS = 4, 3


def side_counts(case, i):
    """Mixed counts of the i-th ragged capture, different per capture."""
    return [1 + (7 * b + 3 * i) % case.N for b in range(case.B)]
