"""Ragged training from a captured graph ("Ragged batches", Training from a captured graph):
`GraphedTrainStep(ragged=True / "subset")` — every replay against its eager twin, the mask entry, masks with holes, empty
slots through the backward, the refusals, the scope, and an eval graph beside the train graph.

Gates.  Replay against the eager twin, with the deterministic mode on at capture and in the twin: `torch.equal` on the
loss and on every parameter (the same kernels add the same numbers in the same order).  The twin of a replay whose counts
all equal N is handed them as an `ops.AgentCounts`, which keeps the ragged route as the capture does — a plain list of N's
is no counts and takes the full-batch route, whose values agree to rounding only.  Parameter gradients against the
float64 per-scene oracle: the gates of tests/test_ragged_backward_gpu.py — TOL_CLEAN (2e-5 of max|grad|) where every live
scene is clean by relu_probe, TOL_ANY (2e-3) otherwise.  Isolation and empty slots: exact zeros, `torch.equal`."""
import copy

import pytest
import torch

import agent_subset_cases as AS
import ragged_backward_cases as RB
import ragged_cases as C
import ragged_graph_cases as RG
import ragged_train_graph_cases as TG
from test_backward_gpu import TOL_ANY, TOL_CLEAN, _check

pytestmark = pytest.mark.gpu

SEED = 4321
D = TG.D


def dev():
    return torch.device("cuda:0")


@pytest.fixture
def deterministic():
    import groupnet_amd as G
    G.set_deterministic(True)
    yield
    G.set_deterministic(None)


def block_of(scales, nmp, seed):
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(seed)
    return MultiScaleHGNN(list(scales), nmp_layers=nmp).to(dev()).eval()


def train_step(blk, loss_fn, B, N, lr, ragged, warmup=1):
    from groupnet_amd.graphs import GraphedTrainStep
    return GraphedTrainStep(blk, torch.optim.SGD(blk.parameters(), lr=lr), loss_fn, B, N,
                            target_shapes=[(B, N, blk.out_features - D)], seed=SEED, warmup=warmup, ragged=ragged)


def rewind(step, k=0):
    """The next replay draws what replay k drew."""
    step.counter.fill_((k - 1) * step.draws_per_step)


def grads_of(blk):
    return {n: p.grad.clone() for n, p in blk.named_parameters() if p.grad is not None}


def twin_of(blk, step, lr):
    """A copy of the block on the weights the capture left, with its own SGD."""
    from groupnet_amd import MS_HGNN_batch as M
    ref = copy.deepcopy(blk)
    M.invalidate_weight_caches(ref)
    return ref, torch.optim.SGD(ref.parameters(), lr=lr)


def eager_step(ref, opt, loss_fn, f, target, n_agents, valid, offset):
    """The eager step of the contract: the opt-in, device noise of the capture's seed at ``offset``, forward with
    ``n_agents``, the loss with ``valid``, backward, the optimizer."""
    import groupnet_amd as G
    G.set_ragged_training(True)
    G.set_noise_mode("device", seed=SEED, offset=offset)
    try:
        opt.zero_grad(set_to_none=True)
        out, H = ref(f, n_agents=n_agents)
        loss = loss_fn(out, H, target, valid=valid)
        loss.backward()
        opt.step()
    finally:
        G.set_noise_mode("host", seed=0, offset=0)
        G.set_ragged_training(None)
    return loss.detach()


def assert_same_weights(blk, ref, tag):
    for (n1, p1), (_, p2) in zip(blk.named_parameters(), ref.named_parameters()):
        assert torch.equal(p1, p2), (tag, n1, float((p1 - p2).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# 1. a replay is the eager step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", TG.SHAPES, ids=lambda s: s.id)
def test_replay_equals_the_eager_twin_bit_for_bit(shape, deterministic):
    from groupnet_amd import ops
    B, N = shape.B, shape.N
    blk = block_of(shape.scales, shape.nmp, shape.seed)
    f, target = [t.to(dev()) for t in TG.features(shape, blk.out_features - D)]
    loss_g, loss_e = TG.MaskedMSE(), TG.MaskedMSE()
    step = train_step(blk, loss_g, B, N, 0.05, True)
    assert step.draws_per_step == shape.nmp * sum(b * e * k for b, e, k in blk.noise_shapes(B, N))    # the padded shapes
    assert isinstance(step.counts, ops.StaticAgentCounts) and step.counts.dev.cpu().tolist() == [N] * B
    ref, opt = twin_of(blk, step, 0.05)
    buf = step.counts.dev.data_ptr()
    losses = []
    for k, (given, used) in enumerate(zip(shape.replays, TG.counts_in_force(shape.replays))):
        kw = {} if given is None else dict(n_agents=list(given) if k else torch.tensor(given))
        lg = step(f if k == 0 else None, target, **kw).clone()
        n_agents = ops.AgentCounts(tuple(used), N, dev()) if all(c == N for c in used) else list(used)
        le = eager_step(ref, opt, loss_e, f, target, n_agents, TG.prefix_valid(used, N).to(dev()), k * step.draws_per_step)
        assert torch.equal(lg, le), (shape.id, k, float(lg), float(le))
        assert_same_weights(blk, ref, (shape.id, k))
        assert int(step.counter.item()) == k * step.draws_per_step
        assert step.counts.dev.cpu().tolist() == list(used) and step.counts.dev.data_ptr() == buf
        assert torch.equal(loss_g.seen[2].cpu(), TG.prefix_valid(used, N))          # `valid`, made inside the graph
        losses.append(float(lg))
    assert len(set(losses)) == len(losses) and all(l > 0 for l in losses)
    # an all-empty replay moves no weight (lr 0.05: a non-zero gradient would)
    before = {n: p.detach().clone() for n, p in blk.named_parameters()}
    step(None, target, n_agents=[0] * B)
    assert all(not bool(p.grad.any()) for p in blk.parameters() if p.grad is not None)
    assert all(torch.equal(p, before[n]) for n, p in blk.named_parameters())
    assert not bool(loss_g.seen[2].any())


# ---------------------------------------------------------------------------------------------------------------------
# the n7 step at lr 0 that tests 2, 4 and 5 share: weights never move, the counter is rewound, gradients are read
# ---------------------------------------------------------------------------------------------------------------------
class _N7:
    pass


@pytest.fixture(scope="module")
def n7():
    import groupnet_amd as G
    counts = TG.EMPTY_COUNTS
    for redraw in range(64):        # the settled-case rule of ragged_backward_cases, over the scenes that hold agents
        case = RB.module_case(7, counts, [3, 7], seed=7, redraw=redraw)
        h = C.inputs(case)[0]
        if C.min_gap(dict(case, counts=[max(c, 1) for c in counts]), h) >= C.MIN_GAP:
            break
    else:
        raise AssertionError("no draw with the affinity gaps the case needs")
    s = _N7()
    s.case, s.h = case, h
    s.B, s.N, s.scales = case["B"], case["N"], case["scales"]
    blk, s.sp, s.shs = C.cpu_block(case)
    s.blk = blk.to(dev()).eval()
    s.x = C.with_garbage(case, h).to(dev())             # whole scenes of finite garbage x 100 in the empty slots
    s.Rm = torch.randn(s.B, s.N, D * (1 + len(s.scales)), generator=torch.Generator().manual_seed(6)).to(dev())
    s.loss = TG.PaddedDot()
    G.set_deterministic(True)
    try:
        s.step = train_step(s.blk, s.loss, s.B, s.N, 0.0, True)
    finally:
        G.set_deterministic(None)
    s.weights = {n: p.detach().clone() for n, p in s.blk.named_parameters()}
    return s


def replay_n7(s, x, k=0, **kw):
    rewind(s.step, k)
    loss = s.step(x, s.Rm, **kw).clone()
    return loss, grads_of(s.blk)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the mask entry
# ---------------------------------------------------------------------------------------------------------------------
def test_mask_entry(n7):
    from groupnet_amd import _lib
    counts = [7, 4, 3, 2, 1]
    loss_c, grads_c = replay_n7(n7, n7.x, n_agents=counts)
    m = RG.prefix_mask(counts, n7.N)
    for valid in (torch.from_numpy(m).to(dev()), torch.from_numpy(m.astype("uint8") * 9).to(dev())):
        n7.step.counts.set([n7.N] * n7.B)
        loss_m, grads_m = replay_n7(n7, None, agent_mask=valid)
        assert torch.equal(loss_m, loss_c) and grads_m.keys() == grads_c.keys()
        assert all(torch.equal(grads_m[n], grads_c[n]) for n in grads_c)
    assert not n7.step.status() & _lib.COUNTS_NOT_PREFIX
    holed = m.copy()
    holed[2, 5] = True                                      # scene 2: agents 0..2, and agent 5 behind two invalid slots
    loss_h, grads_h = replay_n7(n7, None, agent_mask=torch.from_numpy(holed).to(dev()))
    assert n7.step.status() & _lib.COUNTS_NOT_PREFIX        # ... which is not counted: the leading run trains
    assert torch.equal(loss_h, loss_c) and all(torch.equal(grads_h[n], grads_c[n]) for n in grads_c)
    assert n7.step.counts.dev.cpu().tolist() == counts


# ---------------------------------------------------------------------------------------------------------------------
# 3. masks with holes
# ---------------------------------------------------------------------------------------------------------------------
def test_subset_replay_equals_the_eager_twin_bit_for_bit(deterministic):
    import groupnet_amd as G
    from groupnet_amd import ops
    case = AS.BY_ID["n7"]
    B, N = case["B"], case["N"]
    blk = block_of(case["scales"], 1, 70)
    h = AS.inputs(case)[0]
    target = torch.randn(B, N, blk.out_features - D, generator=torch.Generator().manual_seed(8)).to(dev())
    loss_g, loss_e = TG.MaskedMSE(), TG.MaskedMSE()
    step = train_step(blk, loss_g, B, N, 0.05, "subset")
    assert isinstance(step.counts, ops.StaticAgentSubset)
    ref, opt = twin_of(blk, step, 0.05)
    losses = []
    for k, mask in enumerate(TG.subset_masks(case["mask"])):
        f = AS.with_nan(dict(case, mask=mask), h).to(dev())             # NaN in every invalid row
        assert bool(torch.isnan(f).any())
        lg = step(f, target, agent_mask=mask.to(dev())).clone()
        sub = G.agent_subset(mask, dev())
        assert isinstance(sub, ops.AgentSubset)
        le = eager_step(ref, opt, loss_e, f, target, sub, mask.to(dev()), k * step.draws_per_step)
        assert bool(torch.isfinite(lg)) and torch.equal(lg, le), (k, float(lg), float(le))
        assert_same_weights(blk, ref, k)
        assert torch.equal(loss_g.seen[2].cpu(), mask)                  # `valid` = slot >= 0
        final = loss_g.seen[0]
        assert bool(torch.isfinite(final).all()) and not bool(final[~mask.to(dev())].any())
        losses.append(float(lg))
    assert step.status() == 0 and len(set(losses)) == 3


# ---------------------------------------------------------------------------------------------------------------------
# 4. empty slots
# ---------------------------------------------------------------------------------------------------------------------
def test_empty_slots_outputs_are_zero(n7):
    counts = TG.EMPTY_COUNTS
    empty = [b for b, c in enumerate(counts) if c == 0]
    live = [b for b, c in enumerate(counts) if c]
    loss, grads = replay_n7(n7, n7.x, n_agents=counts)
    final, new_H, valid = n7.loss.seen
    assert valid.dtype == torch.bool and torch.equal(valid.cpu(), TG.prefix_valid(counts, n7.N))
    assert not bool(valid[empty].any())
    assert bool(torch.isfinite(final).all()) and torch.equal(final[..., :D], n7.x)      # f copied through, garbage included
    assert not bool(final[empty][..., D:].any()) and not bool(new_H[empty].any())
    assert bool(final[live][..., D:].any()) and bool(new_H[live].any())
    assert bool(torch.isfinite(loss)) and all(bool(torch.isfinite(g).all()) for g in grads.values())


def test_empty_slots_gradients_against_the_oracle(n7):
    """Parameter gradients of the replay with counts (7, 0, 3, 0, 1) against the float64 oracle of the three live scenes
    alone, fed the replay's own draws."""
    from groupnet_amd import ops
    case, counts, B, N, scales = n7.case, TG.EMPTY_COUNTS, n7.B, n7.N, n7.scales
    live = [b for b, c in enumerate(counts) if c]
    _, grads = replay_n7(n7, n7.x, n_agents=counts)
    shapes = C.noise_shapes(case)
    offsets, total = RG.draw_offsets(shapes, 1)
    assert total == n7.step.draws_per_step
    U = [[ops.philox_uniform(sh, SEED, o, dev()).cpu() for o in per] for sh, per in zip(shapes, offsets)]
    Rm = n7.Rm.cpu()
    refs = []
    for i, (state, s) in enumerate(zip([n7.sp, *n7.shs], [None, *scales])):
        E = N * N if s is None else (1 if s == N else N)
        K = C.K_PAIR if s is None else C.K_HYPER
        refs.append(RB.module_oracle(state, s is None, s, case, n7.h, U[i], Rm[..., D * i:D * (i + 1)], torch.zeros(B, E, K),
                                     scenes=live))
    clean = torch.stack([r["clean"][live] for r in refs]).all()
    tol = TOL_CLEAN if bool(clean) else TOL_ANY
    final = n7.loss.seen[0]
    want = torch.cat([r["node_feat"] for r in refs], dim=-1)
    assert float((final[..., D:].double().cpu() - want).abs().max()) <= 1e-5
    worst = []
    for prefix, r in zip(["interaction."] + [f"interaction_hyper.{i}." for i in range(len(scales))], refs):
        used = [k for k, v in r["grads"].items() if v is not None and float(v.abs().max()) > 0]
        assert len(used) >= 30
        hip = {k[len(prefix):]: g for k, g in grads.items() if k.startswith(prefix)}
        worst.append(_check(hip, r["grads"], used, tol))
    print(f"\nragged train graph n7 counts {list(counts)}: worst parameter per module {worst}; clean {bool(clean)}, gate {tol:g}")


def test_empty_slots_influence_nothing(n7):
    counts = TG.EMPTY_COUNTS
    loss, grads = replay_n7(n7, n7.x, n_agents=counts)
    other = C.with_garbage(n7.case, n7.h, seed=1234).to(dev())          # other finite values x 100 in the empty slots
    assert not torch.equal(other[1], n7.x[1]) and torch.equal(other[0], n7.x[0])
    loss2, grads2 = replay_n7(n7, other, n_agents=counts)
    assert torch.equal(loss, loss2) and grads.keys() == grads2.keys() and len(grads) >= 100
    for n in grads:
        assert bool(grads[n].any()), n
        assert torch.equal(grads[n], grads2[n]), (n, float((grads[n] - grads2[n]).abs().max()))
    assert all(torch.equal(p, n7.weights[n]) for n, p in n7.blk.named_parameters())


def test_all_empty_replay_has_zero_gradients(n7):
    _, grads = replay_n7(n7, n7.x, n_agents=[0] * n7.B)
    assert len(grads) >= 100 and all(not bool(g.any()) for g in grads.values())
    assert not bool(n7.loss.seen[2].any()) and not bool(n7.loss.seen[0][..., D:].any())
    assert all(torch.equal(p, n7.weights[n]) for n, p in n7.blk.named_parameters())
    _, again = replay_n7(n7, n7.x, n_agents=TG.EMPTY_COUNTS)             # ... and the next replay trains
    assert all(bool(g.any()) for g in again.values())


def test_subset_with_an_empty_scene(deterministic):
    from groupnet_amd import _lib
    case = AS.BY_ID["n7"]
    B, N = case["B"], case["N"]
    blk = block_of(case["scales"], 1, 71)
    mask = (case["mask"] != 0).clone()
    mask[2] = False                                                     # one scene without a valid agent
    h = AS.inputs(case)[0]
    f = AS.with_nan(dict(case, mask=mask), h).to(dev())
    assert bool(torch.isnan(f[2]).all())
    target = torch.randn(B, N, blk.out_features - D, generator=torch.Generator().manual_seed(9)).to(dev())
    loss_fn = TG.MaskedMSE()
    step = train_step(blk, loss_fn, B, N, 0.0, "subset")
    gm = mask.to(dev())
    loss = step(f, target, agent_mask=gm).clone()
    grads = grads_of(blk)
    assert step.status() == _lib.COUNTS_EMPTY
    final, new_H, valid = loss_fn.seen
    assert torch.equal(valid.cpu(), mask) and not bool(final[2].any()) and not bool(new_H[2].any())
    assert bool(torch.isfinite(final).all())
    assert bool(torch.isfinite(loss)) and len(grads) >= 100
    assert all(bool(torch.isfinite(g).all()) and bool(g.any()) for g in grads.values())
    other = f.clone()
    other[2] = torch.randn(N, D, generator=torch.Generator().manual_seed(10)).to(dev()) * 100.0
    rewind(step)
    loss2 = step(other, target, agent_mask=gm).clone()
    grads2 = grads_of(blk)
    assert torch.equal(loss, loss2)
    for n in grads:
        assert torch.equal(grads[n], grads2[n]), (n, float((grads[n] - grads2[n]).abs().max()))


def test_the_single_factor_row_of_an_empty_slot_gets_no_gradient(deterministic):
    """A scale-N module on its own, whose `factors` the caller's loss does read (the block does not return them): the
    gradient the loss puts on the single row of an empty scene is dropped, as the forward zeroed that row — the
    gradients are those of the loss with the empty scene's rows of R1 and R2 set to zero, bit for bit."""
    import groupnet_amd as G
    from groupnet_amd import MS_HGNN_batch as M, ops
    B, N = 3, 7
    torch.manual_seed(5)
    mod = G.MS_HGNN_hyper(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=1,
                          scale=N).to(dev())
    g = torch.Generator().manual_seed(12)
    h, corr = torch.randn(B, N, 64, generator=g).to(dev()), torch.randn(B, N, N, generator=g).to(dev())
    U = torch.rand(B, 1, mod.edge_types, generator=g).to(dev())
    R1, R2 = torch.randn(B, N, 64, generator=g).to(dev()), torch.randn(B, 1, mod.edge_types, generator=g).to(dev())
    held = ops.StaticAgentCounts(B, N, dev())
    held.set([7, 0, 3])

    def run(R1, R2):
        for p in mod.parameters():
            p.grad = None
        x = h.clone().requires_grad_(True)
        with M.ragged_train_graph_scope():
            nf, fac, H = mod(x, corr, noise_u=U, n_agents=held)
            ((nf * R1).sum() + (fac * R2).sum()).backward()
        return fac.detach(), H, x.grad.clone(), grads_of(mod)

    fac, H, gx, got = run(R1, R2)
    assert fac.shape == (B, 1, mod.edge_types) and not bool(fac[1].any()) and bool(fac[0].any()) and not bool(H[1].any())
    R1z, R2z = R1.clone(), R2.clone()
    R1z[1], R2z[1] = 0, 0
    _, _, gx0, want = run(R1z, R2z)
    assert bool(R2[1].any()) and not bool(gx[1].any()) and torch.equal(gx, gx0)
    assert got.keys() == want.keys() and sum(bool(v.any()) for v in got.values()) >= 30
    for n in got:
        assert torch.equal(got[n], want[n]), (n, float((got[n] - want[n]).abs().max()))
    assert not M.trains_empty_slots()
    with pytest.raises(NotImplementedError):                # outside the scope the holder stays inference-only
        G.set_ragged_training(True)
        try:
            mod(h.clone().requires_grad_(True), corr, noise_u=U, n_agents=held)
        finally:
            G.set_ragged_training(None)


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch_or_copy(n7, monkeypatch):
    from groupnet_amd import ops
    from groupnet_amd.multiscale import MultiScaleHGNN
    B, N, counts = n7.B, n7.N, [7, 4, 3, 2, 1]
    g = n7.step
    plain_blk = block_of(n7.scales, 1, 72)
    plain = train_step(plain_blk, lambda out, H, t: ((out[..., D:] - t) ** 2).mean(), B, N, 0.0, False)
    assert plain.counts is None
    replay_n7(n7, n7.x, n_agents=counts)
    plain(n7.x, n7.Rm)
    torch.cuda.synchronize()
    was = (g.f_in.clone(), g.counts.dev.clone(), g.targets[0].clone(), plain.f_in.clone(), plain.targets[0].clone())
    launches, real = [], ops.stream_handle
    monkeypatch.setattr(ops, "stream_handle", lambda: launches.append(1) or real())
    monkeypatch.setattr(type(g.graph), "replay", lambda self: launches.append("replay"))
    other, tgt = n7.x + 1.0, n7.Rm + 1.0
    mask = torch.from_numpy(RG.prefix_mask(counts, N)).to(dev())
    for call in (lambda: plain(other, tgt, n_agents=counts), lambda: plain(other, tgt, agent_mask=mask), plain.status,
                 lambda: g(other, tgt, n_agents=counts, agent_mask=mask),
                 lambda: g(other, tgt, n_agents=counts[:-1]), lambda: g(other, tgt, n_agents=[N + 1] + counts[1:]),
                 lambda: g(other, tgt, n_agents=torch.tensor(counts, device=dev())),
                 lambda: g(other, tgt, agent_mask=mask.cpu()), lambda: g(other, tgt, agent_mask=mask.float()),
                 lambda: g(other, tgt, agent_mask=mask[:-1]), lambda: g(other, tgt, agent_mask=mask[:, :-1].contiguous())):
        with pytest.raises(ValueError):
            call()
    # at construction
    loss_fn = TG.MaskedMSE()
    with pytest.raises(ValueError):
        train_step(n7.blk, loss_fn, B, N, 0.0, "x")
    n7.blk.interaction_hyper[0].listall = True
    try:
        for ragged in (True, "subset"):
            with pytest.raises(NotImplementedError):
                train_step(n7.blk, loss_fn, B, N, 0.0, ragged)
    finally:
        n7.blk.interaction_hyper[0].listall = False
    with pytest.raises(NotImplementedError):
        train_step(n7.blk, loss_fn, 2, 141, 0.0, True)       # beyond the per-scene node->edge backward
    with pytest.raises(RuntimeError):
        train_step(n7.blk, loss_fn, B, 6, 0.0, True)         # scale 7 > N = 6
    assert not launches
    assert loss_fn.seen is None
    for got, w in zip((g.f_in, g.counts.dev, g.targets[0], plain.f_in, plain.targets[0]), was):
        assert torch.equal(got, w)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the scope does not leak
# ---------------------------------------------------------------------------------------------------------------------
def test_the_eager_refusals_stand_beside_a_ragged_train_graph(n7):
    import groupnet_amd as G
    from groupnet_amd import MS_HGNN_batch as M
    replay_n7(n7, n7.x, n_agents=TG.EMPTY_COUNTS)
    assert not M.trains_empty_slots() and M._TRAIN_GRAPH_SCOPE[0] == 0
    x = n7.x.clone().requires_grad_(True)
    try:
        for on in (None, False, True):                      # (True: the holder admits empty slots, which stay inference-only)
            G.set_ragged_training(on)
            with pytest.raises(NotImplementedError):
                n7.blk(x, n_agents=n7.step.counts)
        G.set_ragged_training(False)
        with pytest.raises(NotImplementedError):
            n7.blk(x, n_agents=[7, 4, 3, 2, 1])
        with pytest.raises(ValueError):                     # ... and eagerly a count of 0 is no count at all
            n7.blk(x, n_agents=list(TG.EMPTY_COUNTS))
    finally:
        G.set_ragged_training(None)
    with torch.no_grad():                                   # inference with the holder is what it was
        out, _ = n7.blk(n7.x, n_agents=n7.step.counts)
    assert not bool(out[1][..., D:].any())


def test_an_exception_in_the_loss_closes_the_scope():
    from groupnet_amd import MS_HGNN_batch as M
    shape = TG.BY_ID["n7"]
    blk = block_of(shape.scales, 1, 73)

    def bad_loss(out, H, t, valid):
        assert M.trains_empty_slots()
        raise KeyError("the caller's loss")

    with pytest.raises(KeyError):
        train_step(blk, bad_loss, shape.B, shape.N, 0.0, True)
    torch.cuda.synchronize()
    assert M._TRAIN_GRAPH_SCOPE[0] == 0 and not M.trains_empty_slots()


# ---------------------------------------------------------------------------------------------------------------------
# 7. an eval graph beside the train graph
# ---------------------------------------------------------------------------------------------------------------------
def test_eval_graph_refreshes_after_a_ragged_train_replay():
    import groupnet_amd as G
    from groupnet_amd.graphs import GraphedMultiScale
    shape = TG.BY_ID["n7"]
    B, N, counts = shape.B, shape.N, list(shape.replays[0])
    blk = block_of(shape.scales, 1, 74)
    f, target = [t.to(dev()) for t in TG.features(shape, blk.out_features - D)]
    g = GraphedMultiScale(blk, B, N, seed=SEED, ragged=True)
    first = g(f, n_agents=counts)[0].clone()
    step = train_step(blk, TG.MaskedMSE(), B, N, 0.05, True)
    step(f, target, n_agents=counts)
    out, H = [t.clone() for t in g(n_agents=counts)]        # no refresh_weights(): the replay sees the epoch moved
    G.set_noise_mode("device", seed=SEED, offset=g.draws_per_step)
    try:
        with torch.no_grad():
            e_out, e_H = blk(f, n_agents=counts)
    finally:
        G.set_noise_mode("host", seed=0, offset=0)
    assert torch.equal(out, e_out) and torch.equal(H, e_H)
    assert not torch.equal(out[..., D:], first[..., D:])
