"""Ragged batches replayed from a captured graph ("Ragged batches"): the counts kernel against the
NumPy rule of tests/ragged_graph_cases.py, the static holder of the counts, and `GraphedMultiScale(ragged=True)` — every
replay against the eager ragged forward under the same device noise, bit for bit, with new counts on every replay; the
empty slots (count 0); the mask entry; the forked capture; the refusals.

Gates.  Replay against eager: bit equality (the same kernels on the same numbers).  All counts N against the full-batch
route: H bit for bit; features 2e-5 for fp32 storage — both routes are gated at the project's 1e-5 against the same
float64 oracle — and, for bf16, twice the gate of tests/test_ragged_gpu.py, TOL_ORACLE of the module's largest oracle
feature; that scale is taken from the full-batch output, which the same gate puts within TOL_ORACLE of the oracle's, so
it is divided by 1 + TOL_ORACLE: never the wider bound.  Against the per-scene oracle: ragged_cases.TOL, incidence exact.
"""
import contextlib

import numpy as np
import pytest
import torch

import ragged_cases as C
import ragged_graph_cases as RG
from test_bf16_gpu import TOL_ORACLE

pytestmark = pytest.mark.gpu

SEED = 4321


def dev():
    return torch.device("cuda:0")


def block_of(case, nmp=1):
    return C.cpu_block(case, nmp)[0].to(dev()).eval()


def inputs_of(case, counts, bf16):
    """The case's features with finite garbage in every row that `counts` pads (whole scenes where the count is 0)."""
    h, _ = C.inputs(case, bf16=bf16)
    x = C.with_garbage(dict(case, counts=list(counts)), h).to(dev())
    return x.bfloat16() if bf16 else x


def count_vectors(case):
    """The case's own counts, a permutation of them, and another vector that is not all N."""
    N, c = case["N"], case["counts"]
    return [list(c), list(reversed(c)), [max(1, N - 1 - b) for b in range(case["B"])]]


@contextlib.contextmanager
def device_noise(blk, offset, tail=None):
    import groupnet_amd as G
    prev = blk.affinity_tail
    if tail is not None:
        blk.affinity_tail = tail
    G.set_noise_mode("device", seed=SEED, offset=offset)
    try:
        with torch.no_grad():
            yield
    finally:
        G.set_noise_mode("host", seed=0, offset=0)
        blk.affinity_tail = prev


def eager(blk, x, counts, k, draws, tail=None):
    with device_noise(blk, k * draws, tail):
        return blk(x, n_agents=counts)


def graph_of(blk, case, bf16=False, **kw):
    from groupnet_amd.graphs import GraphedMultiScale
    return GraphedMultiScale(blk, case["B"], case["N"], seed=SEED, dtype=torch.bfloat16 if bf16 else torch.float32,
                             ragged=True, **kw)


def rewind(g):
    """The next replay draws what replay 0 drew."""
    g.counter.fill_(-g.draws_per_step)


# ---------------------------------------------------------------------------------------------------------------------
# the counts kernel and the holder
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_bool", [False, True], ids=["uint8", "bool"])
@pytest.mark.parametrize("N", RG.MASK_NS)
def test_counts_kernel_equals_the_rule(N, as_bool):
    from groupnet_amd import ops
    m = RG.mask_rows(N)                                   # B = 5: two workgroups, the second with three idle waves
    want, want_status = RG.mask_rule(m)
    valid = torch.from_numpy(m).to(dev())
    valid = valid != 0 if as_bool else valid
    out = torch.full((m.shape[0] + 3,), -7, dtype=torch.int32, device=dev())
    counts, status = ops.counts_from_mask(valid, out=out[:m.shape[0]])
    assert counts.dtype == torch.int32 and counts.cpu().numpy().tolist() == want.tolist()
    assert out[m.shape[0]:].cpu().tolist() == [-7] * 3                          # nothing behind the B counts is written
    assert int(status.item()) == want_status
    clean = torch.ones(2, N, dtype=valid.dtype, device=dev())
    c2, s2 = ops.counts_from_mask(clean, status=status)
    assert c2.cpu().tolist() == [N, N] and s2 is status
    assert int(status.item()) == want_status                                    # sticky: a clean launch clears nothing
    assert int(ops.counts_from_mask(clean)[1].item()) == 0                      # a fresh word starts at 0


def test_counts_kernel_refusals():
    from groupnet_amd import ops
    ok = torch.ones(3, 7, dtype=torch.uint8, device=dev())
    for bad in (ok.cpu(), ok.float(), ok[:, ::2], ok[0], ok.int(), [[1, 1]]):
        with pytest.raises(ValueError):
            ops.counts_from_mask(bad)
    with pytest.raises(ValueError):
        ops.counts_from_mask(ok, out=torch.zeros(4, dtype=torch.int32, device=dev()))
    with pytest.raises(ValueError):
        ops.counts_from_mask(ok, status=torch.zeros(1, dtype=torch.int64, device=dev()))


def test_static_holder_on_the_device():
    from groupnet_amd import ops
    B, N = 6, 7
    held = ops.StaticAgentCounts(B, N, dev(), slots=2)
    buf = held.dev
    assert buf.cpu().tolist() == [N] * B and held.admits_empty and (held.B, held.N) == (B, N)
    assert ops.agent_counts(held, B, N, dev()) is held                  # passes through: the ragged route, even at all N
    with pytest.raises(ValueError):
        ops.agent_counts(held, B, N + 1, dev())
    with pytest.raises(RuntimeError):
        held.counts                                                     # the values live on the device only
    seen = []
    for k in range(5):                                                  # more sets than staging rows, no synchronisation
        vals = [(b + k) % (N + 1) for b in range(B)]
        held.set(vals if k % 2 else torch.tensor(vals))
        seen.append((vals, held.dev.clone()))                           # (the clone is ordered behind the copy)
    assert held.dev is buf and all(got.cpu().tolist() == vals for vals, got in seen)
    for bad in ([N + 1] + [1] * (B - 1), [1] * (B - 1), [-1] + [1] * (B - 1), torch.ones(B, dtype=torch.int32, device=dev())):
        with pytest.raises(ValueError):
            held.set(bad)
    assert held.dev.cpu().tolist() == seen[-1][0]                       # a refused set copies nothing
    m = RG.prefix_mask([0, 7, 3, 1, 0, 2], N)
    held.set_from_mask(torch.from_numpy(m).to(dev()))
    assert held.dev is buf and buf.cpu().tolist() == [0, 7, 3, 1, 0, 2] and int(held.status.item()) == RG.EMPTY
    with pytest.raises(ValueError):
        held.set_from_mask(torch.ones(B, N + 1, dtype=torch.bool, device=dev()))


def test_zero_empty_scenes_launch():
    from groupnet_amd import ops
    B, N = 6, 7
    held = ops.StaticAgentCounts(B, N, dev())
    held.set([0, 2, 7, 0, 5, 1])
    one = torch.rand(B, 1, 10, device=dev()) + 1.0
    odd = (torch.rand(B, 1, 9, device=dev()) + 1.0).bfloat16()             # 18-byte rows: 2-byte stores
    wide = torch.rand(B, 1, 32, device=dev()) + 1.0
    before = [t.clone() for t in (one, odd, wide)]
    ops.zero_empty_scenes([one, odd, wide[..., 8:20]], held)
    for got, was in zip((one, odd), before):
        assert not got[[0, 3]].any() and torch.equal(got[[1, 2, 4, 5]], was[[1, 2, 4, 5]])
    want = before[2].clone()
    want[[0, 3], :, 8:20] = 0
    assert torch.equal(wide, want)
    with pytest.raises(ValueError):
        ops.zero_empty_scenes([torch.rand(B, 2, 10, device=dev())], held)
    with pytest.raises(ValueError):
        ops.zero_empty_scenes([one], [0, 2, 7, 0, 5, 1])


# ---------------------------------------------------------------------------------------------------------------------
# replay equals eager
# ---------------------------------------------------------------------------------------------------------------------
REPLAYS = ([(c, d, 1, t) for c, d in (("n7", "fp32"), ("n17", "fp32"), ("n50", "bf16")) for t in (True, False)]
           + [("n7", "fp32", 2, True)])


@pytest.mark.parametrize("case_id,dtype,nmp,tail", REPLAYS,
                         ids=[f"{c}-{d}-nmp{n}-{'tail' if t else 'own-launch'}" for c, d, n, t in REPLAYS])
def test_replay_equals_eager_bit_for_bit(case_id, dtype, nmp, tail):
    """Replay k with count vector k against the eager ragged forward at offset k * draws_per_step."""
    case, bf16 = C.BY_ID[case_id], dtype == "bf16"
    blk = block_of(case, nmp)
    x = inputs_of(case, case["counts"], bf16)
    g = graph_of(blk, case, bf16, affinity_tail=tail)
    assert g.draws_per_step == nmp * sum(b * e * k for b, e, k in C.noise_shapes(case))       # the padded shapes
    buf = g.counts.dev.data_ptr()
    for k, counts in enumerate(count_vectors(case)):
        out, H = g(x if k == 0 else None, n_agents=counts if k != 1 else torch.tensor(counts))
        out, H = out.clone(), H.clone()
        e_out, e_H = eager(blk, x, counts, k, g.draws_per_step, tail)
        assert torch.equal(out, e_out) and torch.equal(H, e_H), f"replay {k}, counts {counts}"
        assert int(g.counter.item()) == k * g.draws_per_step
    assert g.counts.dev.data_ptr() == buf and blk.affinity_tail is True
    # no counts given: the previous ones stay
    out, H = [t.clone() for t in g()]
    e_out, e_H = eager(blk, x, count_vectors(case)[2], 3, g.draws_per_step, tail)
    assert torch.equal(out, e_out) and torch.equal(H, e_H)


def test_back_to_back_sets_without_a_synchronisation():
    case = C.BY_ID["n7"]
    blk = block_of(case)
    x = inputs_of(case, case["counts"], False)
    g = graph_of(blk, case)
    c0, c1 = count_vectors(case)[:2]
    o0 = g(x, n_agents=c0)[0].clone()
    o1 = g(n_agents=c1)[0].clone()
    h0 = g.H.clone()
    assert torch.equal(o0, eager(blk, x, c0, 0, g.draws_per_step)[0])
    e1 = eager(blk, x, c1, 1, g.draws_per_step)
    assert torch.equal(o1, e1[0]) and torch.equal(h0, e1[1])


@pytest.mark.parametrize("case_id,dtype", [("n7", "fp32"), ("n17", "fp32"), ("n50", "bf16")])
def test_all_counts_n_under_a_ragged_capture(case_id, dtype):
    """The ragged route on a batch without padding against the full-batch route: H bit for bit, features at the derived
    gate of the module docstring."""
    case, bf16 = C.BY_ID[case_id], dtype == "bf16"
    N, D = case["N"], 64
    blk = block_of(case)
    x = inputs_of(case, [N] * case["B"], bf16)
    g = graph_of(blk, case, bf16)
    out, H = [t.clone() for t in g(x)]                                  # the holder starts filled with N
    with device_noise(blk, 0):
        f_out, f_H = blk(x)
    assert torch.equal(H, f_H) and torch.equal(out[..., :D], f_out[..., :D])
    bad = []
    for i in range(1 + len(case["scales"])):
        a, b = out[..., D * (1 + i):D * (2 + i)].float(), f_out[..., D * (1 + i):D * (2 + i)].float()
        err = float((a - b).abs().max())
        gate = 2 * TOL_ORACLE * float(b.abs().max()) / (1 + TOL_ORACLE) if bf16 else 2e-5
        print(f"\n{case_id} {dtype} module {i}: ragged route against the full-batch route {err:.2e} (gate {gate:.2e})", end="")
        if not err <= gate:
            bad.append((i, err, gate))
    assert not bad, bad


def test_replay_against_the_per_scene_oracle():
    """Case n7: the valid positions of one replay against `block_oracle`, fed the replay's draws as tensors."""
    from groupnet_amd import ops
    case = C.BY_ID["n7"]
    B, N, counts, scales = case["B"], case["N"], case["counts"], case["scales"]
    blk, sp, shs = C.cpu_block(case)
    blk = blk.to(dev()).eval()
    h, _ = C.inputs(case)
    x = inputs_of(case, counts, False)
    shapes = C.noise_shapes(case)
    offsets, total = RG.draw_offsets(shapes, 1)
    g = graph_of(blk, case)
    assert g.draws_per_step == total
    out, H = [t.clone().cpu() for t in g(x, n_agents=counts)]
    U = [[ops.philox_uniform(s, SEED, o, dev()).cpu() for o in per] for s, per in zip(shapes, offsets)]
    assert torch.equal(H, torch.cat([C.padded_incidence(case, h, s) for s in scales], dim=1))
    assert torch.equal(out[..., :64], x.cpu())
    worst = 0.0
    for b, n in enumerate(counts):
        feats, _, _ = C.scene_oracle(sp, shs, case, h, U, b)
        assert not out[b, n:, 64:].any()
        for i, ref in enumerate(feats):
            worst = max(worst, float((out[b, :n, 64 * (1 + i):64 * (2 + i)].double() - ref).abs().max()))
    print(f"\nn7 replay against the per-scene oracle: {worst:.2e} (gate {C.TOL:g})", end="")
    assert worst <= C.TOL


# ---------------------------------------------------------------------------------------------------------------------
# empty slots
# ---------------------------------------------------------------------------------------------------------------------
EMPTY = {"n7": [0, 2, 7, 0, 5, 1], "n50": [0, 23, 50]}


@pytest.mark.parametrize("case_id,dtype", [("n7", "fp32"), ("n50", "bf16")])
def test_empty_slots(case_id, dtype, monkeypatch):
    from groupnet_amd import MS_HGNN_batch as M, multiscale
    case, bf16 = C.BY_ID[case_id], dtype == "bf16"
    counts = EMPTY[case_id]
    empty = [b for b, n in enumerate(counts) if n == 0]
    live = [b for b, n in enumerate(counts) if n > 0]
    filled = [n if n else 3 for n in counts]
    blk = block_of(case)
    x = inputs_of(case, counts, bf16)                       # whole scenes of garbage x 100 in the empty slots
    calls, orig = [], M.run_message_passing
    monkeypatch.setattr(multiscale, "run_message_passing", lambda *a, **k: calls.append(orig(*a, **k)) or calls[-1])
    g = graph_of(blk, case, bf16)
    facs = [fac for _, fac in calls[-1]]                    # the factors of the captured forward: static too, kept alive here
    assert [f.shape[1] for f in facs] == [case["N"] ** 2] + [C.n_edges(case["N"], s) for s in case["scales"]]
    out, H = [t.clone() for t in g(x, n_agents=counts)]
    got = [f.clone() for f in facs]
    assert bool(torch.isfinite(out.float()).all()) and all(bool(torch.isfinite(f.float()).all()) for f in got)
    assert torch.equal(out[..., :64], x)                                            # f copied through, garbage included
    assert not out[empty][..., 64:].any() and not H[empty].any()
    for f, s in zip(got, [None] + case["scales"]):
        assert not f[empty].any(), f"factors of the module of scale {s}"
    assert all(bool(f[live].any()) for f in got) and bool(out[live][..., 64:].any())
    # an empty scene never influences another one: the same replay with the empty slots at count 3
    rewind(g)
    out3, H3 = [t.clone() for t in g(n_agents=filled)]
    assert torch.equal(out[live], out3[live]) and torch.equal(H[live], H3[live])
    assert all(torch.equal(f[live], f3[live]) for f, f3 in zip(got, facs))
    assert bool(out3[empty][..., 64:].any())
    # ... and they equal the eager forward of that batch
    e_out, e_H = eager(blk, x, filled, 0, g.draws_per_step)
    assert torch.equal(out3, e_out) and torch.equal(H3, e_H)


def test_the_eager_forward_keeps_refusing_an_empty_scene():
    case = C.BY_ID["n7"]
    blk = block_of(case)
    with torch.no_grad(), pytest.raises(ValueError):
        blk(inputs_of(case, case["counts"], False), n_agents=EMPTY["n7"])


# ---------------------------------------------------------------------------------------------------------------------
# the mask entry
# ---------------------------------------------------------------------------------------------------------------------
def test_mask_entry():
    from groupnet_amd import _lib
    case = C.BY_ID["n7"]
    N, counts = case["N"], case["counts"]                   # [1, 2, 3, 5, 6, 7]
    blk = block_of(case)
    x = inputs_of(case, counts, False)
    g = graph_of(blk, case)
    by_counts = [t.clone() for t in g(x, n_agents=counts)]
    m = RG.prefix_mask(counts, N)
    for valid in (torch.from_numpy(m).to(dev()), torch.from_numpy(m.astype(np.uint8) * 9).to(dev())):
        g.counts.set([N] * case["B"])
        rewind(g)
        by_mask = g(agent_mask=valid)
        assert torch.equal(by_mask[0], by_counts[0]) and torch.equal(by_mask[1], by_counts[1])
    assert g.status() == 0
    holed = m.copy()
    holed[2, 5] = True                                      # scene 2: agents 0..2, and agent 5 behind two invalid slots
    rewind(g)
    by_hole = g(agent_mask=torch.from_numpy(holed).to(dev()))
    assert g.status() == _lib.COUNTS_NOT_PREFIX             # ... which is not counted: the leading run computes
    assert torch.equal(by_hole[0], by_counts[0]) and torch.equal(by_hole[1], by_counts[1])
    rewind(g)
    g(agent_mask=torch.from_numpy(RG.prefix_mask(EMPTY["n7"], N)).to(dev()))
    assert g.status() == _lib.COUNTS_NOT_PREFIX | _lib.COUNTS_EMPTY                 # sticky, and an empty slot is reported


# ---------------------------------------------------------------------------------------------------------------------
# the forked capture
# ---------------------------------------------------------------------------------------------------------------------
def test_forked_capture(monkeypatch):
    """B * N = 32800 >= 32768: inside the capture the ragged affinity + top-k launch runs on the side stream."""
    from groupnet_amd import multiscale
    from groupnet_amd.graphs import GraphedMultiScale
    B, N, scales = 656, 50, [2, 4, 8, 16]
    torch.manual_seed(9)
    blk = multiscale.MultiScaleHGNN(scales).to(dev()).eval()
    x = (torch.randn(B, N, 64, generator=torch.Generator().manual_seed(10)) * 1.0).to(dev()).bfloat16()
    counts = [(50, 23, 5, 0)[b % 4] for b in range(B)]
    live = torch.tensor([n > 0 for n in counts], device=dev())
    forks, real = [], multiscale._fork_stream
    monkeypatch.setattr(multiscale, "_fork_stream", lambda d: forks.append(1) or real(d))
    g = GraphedMultiScale(blk, B, N, seed=SEED, dtype=torch.bfloat16, ragged=True, warmup=1)
    assert len(forks) == 1                                  # the captured forward alone forks
    out, H = g(x, n_agents=counts)
    e_out, e_H = eager(blk, x, [max(n, 1) for n in counts], 0, g.draws_per_step)
    assert not forks[1:]                                    # ... the eager forward stays on one stream
    assert torch.equal(out[live], e_out[live]) and torch.equal(H[live], e_H[live])
    assert not out[~live][..., 64:].any() and not H[~live].any()


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(monkeypatch):
    from groupnet_amd import ops
    from groupnet_amd.graphs import GraphedMultiScale
    case = C.BY_ID["n7"]
    B, N, counts = case["B"], case["N"], case["counts"]
    blk = block_of(case)
    x = inputs_of(case, counts, False)
    plain = GraphedMultiScale(blk, B, N, seed=SEED)
    g = graph_of(blk, case)
    g(x, n_agents=counts)
    torch.cuda.synchronize()
    was = (g.f_in.clone(), g.counts.dev.clone(), plain.f_in.clone())
    launches, real = [], ops.stream_handle
    monkeypatch.setattr(ops, "stream_handle", lambda: launches.append(1) or real())
    monkeypatch.setattr(type(g.graph), "replay", lambda self: launches.append("replay"))
    other = x + 1.0
    mask = torch.from_numpy(RG.prefix_mask(counts, N)).to(dev())
    for call in (lambda: plain(other, n_agents=counts), lambda: plain(other, agent_mask=mask), plain.status,
                 lambda: g(other, n_agents=counts, agent_mask=mask),
                 lambda: g(other, n_agents=counts[:-1]), lambda: g(other, n_agents=[N + 1] + counts[1:]),
                 lambda: g(other, n_agents=torch.tensor(counts, device=dev())),
                 lambda: g(other, agent_mask=mask.cpu()), lambda: g(other, agent_mask=mask.float()),
                 lambda: g(other, agent_mask=mask[:-1]), lambda: g(other, agent_mask=mask[:, :-1].contiguous())):
        with pytest.raises(ValueError):
            call()
    blk.interaction_hyper[0].listall = True
    try:
        with pytest.raises(NotImplementedError):
            graph_of(blk, case)
    finally:
        blk.interaction_hyper[0].listall = False
    blk.train()
    try:
        with pytest.raises(NotImplementedError):
            graph_of(blk, case)
    finally:
        blk.eval()
    assert not launches
    assert torch.equal(g.f_in, was[0]) and torch.equal(g.counts.dev, was[1]) and torch.equal(plain.f_in, was[2])
