"""Captured graphs over their lifetime (tables: tests/graph_lifetime_cases.py).

A. A captured inference forward holds no packing launch; it reads the packed weight images in place.  Every way the
   parameters change under it — load_state_dict, .data writes, eager optimizer steps, replays of a training graph on
   the same block, one parameter family at a time, storage that moved — followed by `refresh_weights()` (or by nothing,
   where `invalidate_weight_caches` announces the change): the replay equals an eager forward at the new weights and the
   same Philox position bit for bit, and differs from the replay before the change.
B. Every replay of a `GraphedTrainStep`, not the first alone, against an eager twin started from the same weights and
   optimizer state: loss bit for bit, every parameter's and every optimizer state tensor's update within a gate.
C. Graphs of ONE block replayed side by side on four streams, as the benchmark runs them, against the same replays alone.
"""
import contextlib
import copy

import pytest
import torch

import graph_lifetime_cases as L
from test_parity_gpu import TOL

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def switches(monkeypatch):
    """The process-wide switches a configuration sets, put back afterwards."""
    import groupnet_amd as G
    from groupnet_amd import ops
    monkeypatch.setattr(ops, "BF16X6", ops.BF16X6)
    monkeypatch.setattr(ops, "F16X3", ops.F16X3)
    yield ops
    ops.set_incidence_form(None)
    G.set_noise_mode("host", seed=0, offset=0)


def _invalidate(model):
    from groupnet_amd.MS_HGNN_batch import invalidate_weight_caches
    invalidate_weight_caches(model)


# ---------------------------------------------------------------------------------------------------------------------
# A. forward graphs across weight changes
# ---------------------------------------------------------------------------------------------------------------------
class Rig:
    """One configuration: the model, its inputs, captures of it, and the eager forward they are held against."""

    def __init__(self, cfg):
        self.cfg = cfg
        self.encoder = cfg.kind == "encoder"
        self.model = L.make_model(cfg).to(dev())
        x = L.make_inputs(cfg).to(dev())
        self.x = x.bfloat16() if cfg.bf16 else x
        self.counts = list(cfg.counts) if cfg.counts else None
        self.params = dict(self.model.named_parameters())
        self.names = list(self.params)
        self.k = 0
        self.g = self.capture()

    def capture(self):
        from groupnet_amd.graphs import GraphedMultiScale, GraphedPastEncoder
        c = self.cfg
        if self.encoder:
            return GraphedPastEncoder(self.model, c.B, c.N, seed=L.SEED)
        return GraphedMultiScale(self.model, c.B, c.N, seed=L.SEED, dtype=torch.bfloat16 if c.bf16 else torch.float32,
                                 affinity_tail=c.tail, ragged=self.counts is not None)

    def position(self):
        """A new Philox position for every check: replay k of a graph that was never rewound."""
        self.k += 1
        return self.k * self.g.draws_per_step

    def replay(self, g, pos):
        g.counter.fill_(pos - g.draws_per_step)
        out, H = g(self.x, n_agents=self.counts) if self.counts else g(self.x)
        return out.clone(), (None if H is None else H.clone())

    def eager(self, pos):
        import groupnet_amd as G
        m, c = self.model, self.cfg
        prev = getattr(m, "affinity_tail", None)
        G.set_noise_mode("device", seed=L.SEED, offset=pos)
        try:
            with torch.no_grad():
                if self.encoder:
                    return m(self.x, c.B, c.N)
                m.affinity_tail = c.tail
                return m(self.x, n_agents=self.counts)
        finally:
            G.set_noise_mode("host", seed=0, offset=0)
            if not self.encoder:
                m.affinity_tail = prev

    def oracle(self, pos):
        kp, kh = L.edge_types(self.model, self.cfg.kind)
        noise, draws = L.philox_noise(L.noise_shapes(self.cfg, kp, kh), self.cfg.nmp, L.SEED, pos)
        assert draws == self.g.draws_per_step
        state = {k: v.detach().cpu() for k, v in self.model.state_dict().items()}
        return L.oracle64(self.cfg, state, self.x.float().cpu(), noise)

    def holds(self, graphs, pos, pres, tag, invalidate=True, oracle=False):
        """Replays of `graphs` at `pos` == the eager forward there, bit for bit, and != their replays `pres` from before
        the change.  ``invalidate``: the eager side re-derives its images itself (after the replays: the graphs must not
        profit from it), so that it cannot be stale in the same way as a graph."""
        outs = [self.replay(g, pos) for g in graphs]
        if invalidate:
            _invalidate(self.model)
        e_out, e_H = self.eager(pos)
        assert bool(torch.isfinite(e_out.float()).all()), f"{self.cfg.id} {tag}: the eager forward is not finite"
        for (out, H), pre in zip(outs, pres):
            assert torch.equal(out, e_out), f"{self.cfg.id} {tag}: the replay is not the eager forward at these weights"
            assert (H is None and e_H is None) or torch.equal(H, e_H), f"{self.cfg.id} {tag}: H"
            if pre is not None:
                assert not torch.equal(out, pre[0]), f"{self.cfg.id} {tag}: the change did not move the output"
        if oracle:
            err = float((outs[0][0].double().cpu() - self.oracle(pos)).abs().max())
            print(f"{self.cfg.id} {tag}: max |replay - float64 oracle| = {err:.2e} (TOL {TOL:.0e})")
            assert err <= TOL, (tag, err)

    def change(self, mutate, tag, invalidate=True, oracle=False):
        """mutate(); refresh_weights(); the replay follows."""
        pos = self.position()
        pre = self.replay(self.g, pos)
        mutate()
        self.g.refresh_weights()
        self.holds([self.g], pos, [pre], tag, invalidate, oracle)


def _sgd_steps(rig, steps=2):
    """Eager optimizer steps in train() mode (the encoder: dropout active, host noise), then eval().  The encoder's
    un-normalised features (max 7, their squares' gradient through four front-end layers) take a smaller rate."""
    m, c = rig.model, rig.cfg
    m.train()
    opt = torch.optim.SGD(m.parameters(), lr=1e-4 if rig.encoder else 0.05)
    try:
        for _ in range(steps):
            opt.zero_grad(set_to_none=True)
            out = m(rig.x, c.B, c.N)[0] if rig.encoder else m(rig.x)[0]
            (out.float() ** 2).mean().backward()
            opt.step()
    finally:
        m.eval()


@contextlib.contextmanager
def _launches_recorded(monkeypatch, graphs):
    """Every launch of the library (each asks for the stream) and every replay, as test_refusals_come_before_any_launch."""
    from groupnet_amd import ops, weights
    seen, real = [], ops.stream_handle
    with monkeypatch.context() as mp:
        mp.setattr(ops, "stream_handle", lambda: seen.append(1) or real())
        mp.setattr(weights, "stream_handle", lambda: seen.append(1) or real())
        mp.setattr(type(graphs[0].graph), "replay", lambda self: seen.append("replay"))
        yield seen


@pytest.mark.parametrize("cfg", L.CONFIGS, ids=[c.id for c in L.CONFIGS])
def test_forward_graph_follows_weight_changes(cfg, switches, monkeypatch):
    """Items 1-6 of part A on one capture per configuration.  The first configuration is also held against the float64
    oracle (uniforms from `philox_uniform`, module-major) within test_parity_gpu.TOL, which keeps the eager side from being
    stale itself."""
    from groupnet_amd.graphs import GraphedTrainStep
    ops = switches
    if cfg.precision:
        ops.set_precision(cfg.precision)
    if cfg.form:
        ops.set_incidence_form(cfg.form)
    rig = Rig(cfg)
    g, model = rig.g, rig.model
    oracle = cfg.id == L.CONFIGS[0].id
    seed0 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    rig.holds([g], rig.position(), [None], "as captured", invalidate=False, oracle=oracle)

    # 1. load_state_dict of another seed's weights (bumps the versions; the eager side is NOT told anything else)
    other = {k: v.to(dev()) for k, v in L.make_model(cfg, seed=1).state_dict().items()}
    rig.change(lambda: model.load_state_dict(other), "load_state_dict", invalidate=False, oracle=oracle)
    rig.change(lambda: model.load_state_dict(seed0), "load_state_dict back", oracle=oracle)
    # 2. a .data write on every parameter (no version bump)
    rig.change(lambda: [p.data.mul_(1.5) for p in model.parameters()], ".data x 1.5", oracle=oracle)
    rig.change(lambda: model.load_state_dict(seed0), "load_state_dict after the .data write", oracle=oracle)
    # 3. two eager SGD steps in train() mode, then eval()
    rig.change(lambda: _sgd_steps(rig), "two eager SGD steps", oracle=oracle)
    rig.change(lambda: model.load_state_dict(seed0), "load_state_dict after SGD", invalidate=False)

    # 5. one parameter family at a time, the others untouched
    for tag, fam, members in L.family_changes(cfg, rig.names):
        pos = rig.position()
        pre = rig.replay(g, pos)
        with L.scaled(rig.params, members, fam.factor):
            g.refresh_weights()
            rig.holds([g], pos, [pre], f"family {tag}")
        g.refresh_weights()
        back = rig.replay(g, pos)
        assert torch.equal(back[0], pre[0]), f"{cfg.id} family {tag}: restored"

    # 6. moved storage: refused before anything is launched; the old storage back: followed again
    moved = ["interaction.nmp_mlp_end.layers.0.weight"] + (["input_fc2.bias"] if rig.encoder else [])
    held = [t.clone() for t in g._affine] if rig.encoder else []
    for name in moved:
        p = rig.params[name]
        old = p.data
        p.data = old.clone().mul_(1.25)
        try:
            with _launches_recorded(monkeypatch, [g]) as seen:
                with pytest.raises(RuntimeError, match="capture the graph again"):
                    g.refresh_weights()
                assert not seen, (name, seen)
            assert all(torch.equal(a, b) for a, b in zip(g._affine, held)) if rig.encoder else True
        finally:
            p.data = old
    g.refresh_weights()
    rig.holds([g], rig.position(), [None], "the old storage back")

    # 4. a training graph on the same block (the encoder, which has none: a .data write announced by
    #    invalidate_weight_caches): one forward graph from before it and one from after it, replayed after 1 and after 3
    #    training replays WITHOUT refresh_weights()
    if rig.encoder:
        for n in (1, 3):
            pos = rig.position()
            pre = rig.replay(g, pos)
            L.scale_(rig.params, rig.names, 1.0 + 0.05 * n)
            _invalidate(model)
            rig.holds([g], pos, [pre], f"invalidate_weight_caches after a .data write ({n})")
        return
    torch.manual_seed(5)
    tgt = torch.randn(cfg.B, cfg.N, model.out_features, device=dev())
    step = GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.05), lambda o, H, t: ((o - t) ** 2).mean(),
                            cfg.B, cfg.N, target_shapes=[tuple(tgt.shape)], seed=L.SEED + 1, warmup=2)
    g2 = rig.capture()
    for n in (1, 2):        # 1 training replay, then 2 more
        pos = rig.position()
        pres = [rig.replay(h, pos) for h in (g, g2)]
        for _ in range(n):
            step(rig.x.float(), tgt)
        rig.holds([g, g2], pos, pres, f"after {1 if n == 1 else 3} training replays, no refresh")


# ---------------------------------------------------------------------------------------------------------------------
# B. GraphedTrainStep, every replay
# ---------------------------------------------------------------------------------------------------------------------
def _loss_fn(out, H, t):
    return ((out - t) ** 2).mean()


def _snapshot(blk, opt):
    """(model state_dict, optimizer state_dict), deep copies."""
    return ({k: v.detach().clone() for k, v in blk.state_dict().items()}, copy.deepcopy(opt.state_dict()))


def _twin(case, blk, snap):
    """An eager twin at the snapshot: a deepcopy of the block (without the original's weight caches) and an optimizer
    of the same class loaded from the state_dict."""
    twin = copy.deepcopy(blk)
    for m in twin.modules():
        m.__dict__.pop("_gn_weights", None)
        m.__dict__.pop("_gn_plist", None)
    twin.load_state_dict(snap[0])
    opt = L.make_optimizer(case, twin.parameters())
    opt.load_state_dict(copy.deepcopy(snap[1]))
    return twin, opt


def _eager_step(blk, opt, f, tgt, position):
    import groupnet_amd as G
    counter = torch.full((1,), position, dtype=torch.int64, device=dev())
    G.set_noise_mode("device", seed=L.TRAIN_SEED, offset=0, counter=counter)
    try:
        opt.zero_grad(set_to_none=True)
        out, H = blk(f)
        loss = _loss_fn(out, H, tgt)
        loss.backward()
        opt.step()
    finally:
        G.set_noise_mode("host", seed=0, offset=0)
    return loss.detach().clone()


def _tensors(blk, opt):
    """{name: tensor} of the parameters and of every optimizer state tensor (momentum_buffer, exp_avg, exp_avg_sq, step)."""
    out = {}
    for n, p in blk.named_parameters():
        out[n] = p.detach()
        for key, v in opt.state.get(p, {}).items():
            if torch.is_tensor(v):
                out[f"{n}/{key}"] = v.detach()
    return out


def _updates(before, blk, opt):
    """{name: after - before} in float64; the parameters whose update is identically zero (nothing reads them) included."""
    now = _tensors(blk, opt)
    out = {n: t.double() - before[n].double() for n, t in now.items() if n in before}
    out.update({"=" + n: t.double().clone() for n, t in now.items() if n in before})     # (the new values)
    return out


def _kind(name):
    """'param' for a parameter's update, else the optimizer's name of the state tensor."""
    return name.split("/")[1] if "/" in name else "param"


def _scale(b, name):
    scale = float(b[name].abs().max())
    if "/" in name:
        scale = max(scale, float(b["=" + name].abs().max()))
    return scale


def _ulp32(w):
    """The fp32 spacing at every element of `w` (fp32 values held in float64)."""
    w32 = w.float().abs()
    return (torch.nextafter(w32, torch.full_like(w32, float("inf"))) - w32).double()


def _rel(a, b, name):
    """max |a - b| of one tensor's update relative to max |b| — for an optimizer state tensor relative to the larger of that
    and max |new value| (the update of a moment, (1 - beta)(g - m), is a difference of near-equal numbers), and for a
    one-element bias (attention layer 1) relative to the larger of that and its weight's scale: its gradient is one sum
    that cancels to rounding noise, so the tensor has no scale of its own.
    A PARAMETER's update is observed as the difference of two stored fp32 weights, so it is quantised by the weight's
    spacing, not the update's: two steps whose exact results differ by less than that spacing may still store neighbouring
    weights (weights of 0.1 moving by 4e-5: one spacing, 7.5e-9, is 1.8e-4 of the update — either nothing or that much).
    One spacing of the new weight is therefore taken off every element's difference before it is measured."""
    diff = (a[name] - b[name]).abs()
    if "/" not in name:
        diff = (diff - _ulp32(b["=" + name])).clamp_min(0.0)
    scale = _scale(b, name)
    if b[name].numel() == 1 and ".bias" in name:
        scale = max(scale, _scale(b, name.replace(".bias", ".weight")))
    return float(diff.max()) / scale if scale > 0 else float(diff.max())


def _oracle_trajectory(case, snap, batches, order, positions):
    """The float64 oracle's own SGD trajectory on the CPU from the snapshot: torch autograd on
    `O.ms_hgnn_multiscale_forward`, uniforms from `philox_uniform`.  -> the loss of every step."""
    O = L.O
    ps = {n: v.detach().cpu().double().requires_grad_(True) for n, v in snap[0].items()}
    opt = L.make_optimizer(case, list(ps.values()))
    sd = copy.deepcopy(snap[1])
    for st in sd["state"].values():
        for k, v in st.items():
            st[k] = v.detach().cpu().double() if torch.is_tensor(v) else v
    opt.load_state_dict(sd)
    sub = lambda pre: {k[len(pre):]: v for k, v in ps.items() if k.startswith(pre)}
    shapes = [(case.B, case.N * case.N, 6)] + [(case.B, 1 if s == case.N else case.N, 10) for s in case.scales]
    losses = []
    for b, pos in zip(order, positions):
        f, tgt = batches[b]
        noise, _ = L.philox_noise(shapes, case.nmp, L.TRAIN_SEED, pos)
        opt.zero_grad(set_to_none=True)
        out, _, _ = O.ms_hgnn_multiscale_forward(sub("interaction."),
                                                 [sub(f"interaction_hyper.{i}.") for i in range(len(case.scales))],
                                                 list(case.scales), f.double(), [u.double() for u in noise[0]],
                                                 [[u.double() for u in us] for us in noise[1:]], decomposed=True,
                                                 nmp_layers=case.nmp)
        loss = _loss_fn(out, None, tgt.double())
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


@pytest.mark.parametrize("case", L.TRAIN_CASES, ids=[c.id for c in L.TRAIN_CASES])
def test_every_replay_of_a_training_graph_matches_its_eager_twin(case, switches):
    """K = 4 replays with a new f and target each, an eager training step on the graphed block between replays 2 and 3.
    Before replay k an eager twin (deepcopy of the block, optimizer loaded from state_dict()) takes the same step at
    Philox position (k-1) * draws_per_step.  The loss is equal bit for bit; the update of every parameter and of every
    optimizer state tensor is within the gate of max |update| of that tensor; Adam's step counts are equal.

    The gate: the weight gradients are summed by atomics, so two EAGER runs of one step from one state differ; their
    spread (max over tensors and replays of max |u_A - u_B| / max |u_A|), measured on MI355X per case and per kind of
    tensor — parameter, momentum_buffer, exp_avg, exp_avg_sq: the kinds are conditioned differently, exp_avg_sq moves by
    (1 - beta2)(g^2 - v), a difference of near-equal numbers in one-element tensors — is recorded in
    graph_lifetime_cases.UPDATE_SPREAD, and the gate is SPREAD_MARGIN = 8 x that (the graph may order the atomics unlike
    either eager run).  The spread of every run is printed.  Measured (largest over the runs seen; a parameter's
    difference less one fp32 spacing of its weight, see `_rel`): SGD with momentum — momentum_buffer 1.0e-6, parameter the
    same by lr x buffer (gates 8e-6; the graph's worst 1.0e-6 and 1.2e-8); Adam (eps 1e-5) — parameter 1.9e-6, exp_avg
    1.6e-6, exp_avg_sq 2.4e-6 (gates 1.5e-5, 1.3e-5, 1.9e-5; the graph's worst 3.8e-6, 1.6e-6, 2.8e-6); plain SGD in mask form
    at N = 17 — parameter 7.3e-8 (gate 5.8e-7; the graph's worst 7.7e-8; both 1.2e-8 at the lr of the case).  Without the spacing taken off, the parameter
    spreads read 1.8e-4 .. 7.8e-4 in some runs and 0 in others: the quantisation of the stored weight, not the atomics.
    The power of the check, asserted eager against eager: a step from the one-step-stale state (W_{k-2} and its
    optimizer state) differs from the fresh one by >= STALE_POWER = 10 gates in at least one tensor of every family
    (measured with momentum: >= 1.7e4 gates; the final figures of every case are printed).
    First case: the float64 oracle's own trajectory (CPU autograd) — loss per step within ORACLE_MARGIN = 4 x the recorded
    distance of the EAGER path's losses from the oracle's (graph_lifetime_cases.ORACLE_LOSS_DISTANCE: 9.3e-8 of the loss,
    gate 3.7e-7; the graph's losses ARE the eager ones, bit for bit); ReLU units inside
    the rounding window make this the loose check, the eager twin the sharp one."""
    from groupnet_amd.graphs import GraphedTrainStep
    ops = switches
    if case.form:
        ops.set_incidence_form(case.form)
    blk = L.make_block(case).to(dev()).train()
    opt = L.make_optimizer(case, blk.parameters())
    batches = [(f.to(dev()), t.to(dev())) for f, t in L.train_batches(case, blk.out_features)]
    step = GraphedTrainStep(blk, opt, _loss_fn, case.B, case.N, target_shapes=[tuple(batches[0][1].shape)],
                            seed=L.TRAIN_SEED, warmup=2)
    draws = step.draws_per_step
    gates = {kind: L.SPREAD_MARGIN * s for kind, s in L.UPDATE_SPREAD[case.id].items()}
    snaps = [_snapshot(blk, opt)]
    start = snaps[0]
    spreads, worst, losses, order, positions = [], {}, [], [], []
    EAGER_POS = 1000 * draws      # the eager step between replays 2 and 3 draws elsewhere
    for k in range(1, L.TRAIN_K + 1):
        f, tgt = batches[k - 1]
        pos = (k - 1) * draws
        before = {n: t.clone() for n, t in _tensors(blk, opt).items()}
        runs = []
        for _ in range(2):                          # two eager runs of the same step from the same state
            twin, topt = _twin(case, blk, snaps[-1])
            tb = {n: t.clone() for n, t in _tensors(twin, topt).items()}
            loss = _eager_step(twin, topt, f, tgt, pos)
            runs.append((loss, _updates(tb, twin, topt), topt))
        (loss_a, u_a, opt_a), (loss_b, u_b, _) = runs
        assert torch.equal(loss_a, loss_b)
        names = [n for n in u_a if not n.startswith("=")]
        spreads.append({kind: max(_rel(u_b, u_a, n) for n in names if _kind(n) == kind and not n.endswith("/step"))
                        for kind in gates})
        print(f"{case.id} replay {k}: spread of two eager runs " + ", ".join(f"{kd} {v:.2e}" for kd, v in spreads[-1].items()))
        loss_g = step(f, tgt).clone()
        u_g = _updates(before, blk, opt)
        assert torch.equal(loss_g, loss_a), f"replay {k}: loss {float(loss_g)!r} != eager {float(loss_a)!r}"
        assert set(u_g) == set(u_a) and (case.opt == "sgd0" or len(u_g) > len(list(blk.parameters())))
        for n in names:
            if n.endswith("/step"):
                assert torch.equal(u_g[n], u_a[n]) and float(u_a[n]) == 1.0, (k, n)
                continue
            d, gate = _rel(u_g, u_a, n), gates[_kind(n)]
            worst[_kind(n)] = max(worst.get(_kind(n), 0.0), d)
            assert d <= gate, f"replay {k}: update of {n} off by {d:.2e} of its max (gate {gate:.2e})"
        if len(snaps) >= 2:                         # power: the same step from the one-step-stale state
            twin, topt = _twin(case, blk, snaps[-2])
            tb = {n: t.clone() for n, t in _tensors(twin, topt).items()}
            _eager_step(twin, topt, f, tgt, pos)
            u_s = _updates(tb, twin, topt)
            seen = {}
            for n in names:
                fam = L.train_family(n.split("/")[0])
                if not n.endswith("/step") and float(u_a[n].abs().max()) > 0:
                    seen[fam] = max(seen.get(fam, 0.0), _rel(u_s, u_a, n) / gates[_kind(n)])
            weak = {f_: v for f_, v in seen.items() if v < L.STALE_POWER}
            print(f"{case.id} replay {k}: a step from the one-step-stale state differs, in gates, per family by "
                  + ", ".join(f"{f_} {v:.1e}" for f_, v in sorted(seen.items())))
            assert not weak and len(seen) >= 11, f"replay {k}: a one-step-stale state hides in {weak}"
        losses.append(float(loss_g))
        order.append(k - 1)
        positions.append(pos)
        snaps.append(_snapshot(blk, opt))
        if k == 2:                                  # an eager TRAINING step on the graphed block itself
            f5, t5 = batches[L.TRAIN_K]
            losses.append(float(_eager_step(blk, opt, f5, t5, EAGER_POS)))
            order.append(L.TRAIN_K)
            positions.append(EAGER_POS)
            snaps.append(_snapshot(blk, opt))
    top = {kind: max(s[kind] for s in spreads) for kind in gates}
    print(f"{case.id}: largest spread of two eager runs {top} (recorded {L.UPDATE_SPREAD[case.id]}, gates {gates}); "
          f"the graph's worst update {worst}; losses {losses}")
    assert all(top[kind] <= gates[kind] for kind in gates)      # (the recorded spreads still describe this machine)
    if case.id == L.TRAIN_CASES[0].id:
        cpu_batches = [(f.cpu(), t.cpu()) for f, t in batches]
        want = _oracle_trajectory(case, start, cpu_batches, order, positions)
        dist = [abs(a - b) / abs(b) for a, b in zip(losses, want)]
        print(f"{case.id}: |loss - float64 oracle trajectory| / loss per step {[f'{d:.2e}' for d in dist]} (recorded "
              f"{L.ORACLE_LOSS_DISTANCE:.1e}, gate {L.ORACLE_MARGIN * L.ORACLE_LOSS_DISTANCE:.1e})")
        assert max(dist) <= L.ORACLE_MARGIN * L.ORACLE_LOSS_DISTANCE


# ---------------------------------------------------------------------------------------------------------------------
# C. side-by-side replays, as the benchmark runs them
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["throughput", "with-latency-form", "ragged"])
@pytest.mark.parametrize("case", L.SIDE_CASES, ids=[c.id for c in L.SIDE_CASES])
def test_side_by_side_replays_equal_solo_replays(case, variant):
    """Four `GraphedMultiScale(block, B, N, seed=99+i, affinity_tail=False)` of ONE block, replayed round-robin on four
    streams for three rounds with no host synchronisation in between, each replay's `out` and `H` cloned on its stream:
    every clone equals, bit for bit, the clone of the same replay run alone.  Variants: a fifth, latency-form graph
    (affinity_tail=True) interleaved; four ragged captures carrying different counts.
    fp32 at B = 512, N = 11, scales {2,5,11} — 0.1 ms of GPU work — is the smallest shape at which the launches are long
    enough to actually coexist on the chip; bf16 at B = 64, N = 50, scales {2,4,8,16}.  One process, four streams plus the
    default one, the queue settings as they are."""
    from groupnet_amd.graphs import GraphedMultiScale
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(31)
    blk = MultiScaleHGNN(list(case.scales)).to(dev()).eval()
    dtype = torch.bfloat16 if case.bf16 else torch.float32
    ragged = variant == "ragged"
    graphs = [GraphedMultiScale(blk, case.B, case.N, seed=99 + i, dtype=dtype, affinity_tail=False, ragged=ragged)
              for i in range(L.SIDE_GRAPHS)]
    if variant == "with-latency-form":
        graphs.append(GraphedMultiScale(blk, case.B, case.N, seed=99 + L.SIDE_GRAPHS, dtype=dtype, affinity_tail=True))
    gen = torch.Generator().manual_seed(32)
    for i, g in enumerate(graphs):                  # inputs (and counts) once: the replays below copy nothing
        g.f_in.copy_(torch.randn(case.B, case.N, 64, generator=gen).to(dev()))
        if ragged:
            g.counts.set(switch_counts(g, L.side_counts(case, i)))

    def rewind():
        for g in graphs:
            g.counter.fill_(-g.draws_per_step)
        torch.cuda.synchronize()

    rewind()
    solo = [[] for _ in graphs]
    for i, g in enumerate(graphs):                  # 1. each graph alone
        for _ in range(L.SIDE_ROUNDS):
            out, H = g()
            solo[i].append((out.clone(), H.clone()))
    rewind()                                        # 2.
    streams = [torch.cuda.Stream(device=dev()) for _ in range(4)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    side = [[] for _ in graphs]
    for _ in range(L.SIDE_ROUNDS):                  # 3. round-robin, nothing waits for anything
        for i, g in enumerate(graphs):
            with torch.cuda.stream(streams[i % 4]):
                out, H = g()
                side[i].append((out.clone(), H.clone()))
    torch.cuda.synchronize()                        # 4.
    for i in range(len(graphs)):
        assert not torch.equal(solo[i][0][0], solo[i][1][0])          # (fresh noise per replay)
        assert not torch.equal(solo[i][0][0], solo[(i + 1) % len(graphs)][0][0])
        for r in range(L.SIDE_ROUNDS):
            assert torch.equal(side[i][r][0], solo[i][r][0]), f"{case.id} {variant}: out of graph {i}, round {r}"
            assert torch.equal(side[i][r][1], solo[i][r][1]), f"{case.id} {variant}: H of graph {i}, round {r}"


def switch_counts(g, counts):
    from groupnet_amd import ops
    return ops.count_values(counts, g.B, g.N, lowest=0)
