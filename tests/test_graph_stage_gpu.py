"""The three callers of the graph stage — `MultiScaleHGNN.forward`, `multiscale_autograd` and the trajectory encoders —
follow `route.graph_stage_route` through `multiscale.build_graphs`: `ops.AffinityTail.launch`, `ops.affinity`,
`ops.topk_incidence`, `ops.counter_add`, `ops.node_stage_grouped` and `run_message_passing` are wrapped with recording
pass-throughs, one small forward runs per case, and the recorded sequence is the one the route states for the case's
facts.  Every case also names, as literals, the fields of the route its behaviour rests on.  The cases are the smallest
that sit on each boundary of the graph stage."""
import pytest
import torch

from launch_forms import largest_fused_n

pytestmark = pytest.mark.gpu

D = 64
T, IN_DIM = 5, 4                               # the smallest encoder of tests/test_past_encoder.py: 20 raw inputs per agent
BLOCK_BANDED_N = largest_fused_n(D) + 1                        # 113
ENCODER_BANDED_N = largest_fused_n(D, T * IN_DIM) + 1          # 108
ADVANCE = 12345                                # what a forward adds to the device counter

# the block (`MultiScaleHGNN.forward`; "training": through `multiscale_autograd`): the case, and what its route must say
BLOCK_CASES = {
    # latency form at a tail-sized N: the job rides in the first node stage, the closing stage is asked
    "tail": (dict(B=3, N=11, scales=[2, 11]), dict(kind="fused", deferred=True, fork=False, masks=False, ask_closing=True)),
    "own-launch": (dict(B=3, N=11, scales=[2, 11], affinity_tail=False), dict(kind="fused", deferred=False, ask_closing=False)),
    "ungrouped": (dict(B=3, N=11, scales=[2, 11], grouped=False), dict(kind="fused", deferred=False, ask_closing=False)),
    "masks": (dict(B=3, N=17, scales=[2, 17], mask_form=True), dict(kind="fused", masks=True, deferred=False, ask_closing=True)),
    "masks-ragged": (dict(B=3, N=17, scales=[2, 17], mask_form=True, counts=[17, 9, 4]),
                     dict(kind="fused", masks=False, deferred=True)),
    "ragged": (dict(B=3, N=11, scales=[2, 11], counts=[11, 7, 3]), dict(kind="fused", masks=False, deferred=True)),
    "banded": (dict(B=2, N=BLOCK_BANDED_N, scales=[2]), dict(kind="banded", own_copy=True, deferred=False, masks=False)),
    "banded-bf16": (dict(B=2, N=BLOCK_BANDED_N, scales=[2], dtype=torch.bfloat16), dict(kind="banded", own_copy=True)),
    "banded-ragged": (dict(B=2, N=BLOCK_BANDED_N, scales=[2], counts=[BLOCK_BANDED_N, 40]), dict(kind="banded", own_copy=True)),
    "no-scales": (dict(B=3, N=11, scales=[]), dict(kind="none", own_copy=True, H_cat=False, deferred=False)),
    "training": (dict(B=3, N=11, scales=[2, 11], training=True),
                 dict(kind="fused", own_copy=False, deferred=False, masks=False, ask_closing=False)),
    "training-masks": (dict(B=3, N=17, scales=[2, 17], mask_form=True, training=True),
                       dict(kind="fused", own_copy=False, deferred=False, masks=True)),
    # B*N = 32769 under capture: the job on the side stream, a join handed on
    "fork": (dict(B=2979, N=11, scales=[2, 11], capture=True), dict(kind="fused", fork=True, deferred=False, ask_closing=True)),
    "no-fork": (dict(B=3, N=11, scales=[2, 11], capture=True), dict(kind="fused", fork=False, deferred=True)),
}
# the encoders' eval forward: fused front-end and banded, S = 0, 1, 2; the mask form
ENCODER_CASES = {f"{name}-S{len(s)}": (dict(B=2, N=N, scales=s), dict(kind=kind, masks=False, own_copy=kind != "fused",
                                                                     H_cat=len(s) > 1))
                 for name, N in (("fused", 11), ("banded", ENCODER_BANDED_N))
                 for s, kind in (([], "fused" if name == "fused" else "none"), ([5], name), ([5, 11], name))}
ENCODER_CASES["masks"] = (dict(B=2, N=17, scales=[5, 17], mask_form=True), dict(kind="fused", masks=True, H_cat=True))
ENCODER_ALWAYS = dict(fork=False, deferred=False, ask_closing=False)


def dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------------
# recording
# ---------------------------------------------------------------------------------------------------------------------
def record(monkeypatch):
    """Wrap the entry points -> (calls, seen): the list the calls are appended to, and per `run_message_passing` call
    the features and dense incidences it was handed."""
    from groupnet_amd import MS_HGNN_batch, multiscale, ops, past_encoder
    calls, seen, depth = [], [], [0]
    launch = ops.AffinityTail.launch

    def launching(job):
        if not job.done:
            side = torch.cuda.current_stream(dev()) == multiscale._fork_stream(dev())
            calls.append(("launch", "node-stage" if depth[0] else "alone", job.masks is not None, job.counts is not None,
                          bool(job._ex.x_dim), side))
        return launch(job)
    monkeypatch.setattr(ops.AffinityTail, "launch", launching)

    def wrap(name, what):
        real = getattr(ops, name)

        def through(*args, **kwargs):
            calls.append((name, *what(*args, **kwargs)))
            return real(*args, **kwargs)
        monkeypatch.setattr(ops, name, through)
    wrap("affinity", lambda f: (f.dtype,))
    wrap("topk_incidence", lambda corr, scales, n_agents=None: (n_agents is not None,))
    wrap("counter_add", lambda counter, add: ())
    node_stage = ops.node_stage_grouped

    def node_stage_through(items, keep=None, a_specs=None, affinity=None):
        calls.append(("node_stage", affinity is not None))
        depth[0] += 1
        try:
            out = node_stage(items, keep, a_specs, affinity)
        finally:
            depth[0] -= 1
        assert affinity is None or affinity.done, "the node stage leaves the job it was handed done"
        return out
    monkeypatch.setattr(ops, "node_stage_grouped", node_stage_through)
    engine = MS_HGNN_batch.run_message_passing

    def engine_through(mods, hs, Hs, noises, outs, **kw):
        incs = [H for H in Hs if H is not None]
        calls.append(("mp", kw.get("fuse_closing", False), kw.get("join") is not None, kw.get("n_agents") is not None,
                      tuple(isinstance(H, ops.Incidence) and H.masks is not None for H in incs),
                      kw.get("affinity") is not None))
        seen.append((hs[0], [H.H if isinstance(H, ops.Incidence) else H for H in incs]))
        return engine(mods, hs, Hs, noises, outs, **kw)
    for mod in (MS_HGNN_batch, multiscale, past_encoder):
        monkeypatch.setattr(mod, "run_message_passing", engine_through)
    return calls, seen


def stated(r, form, S, *, ragged=False, embed=False, advance=True, one_call=True):
    """The recorded calls of a forward that follows the route `r`."""
    from groupnet_amd import ops, route as R
    ev = []
    if r.kind == R.FUSED and not r.deferred:
        ev.append(("launch", "alone", r.masks, ragged, embed, r.fork))
    if r.kind == R.BANDED:
        ev += [("affinity", torch.float32), ("topk_incidence", ragged)]
    if r.own_copy and advance:
        ev.append(("counter_add",))
    if not one_call:       # the ungrouped block: one engine call per module, no job, no join, no closing stage
        for i in range(1 + S):
            ev += [("mp", False, False, ragged, (r.masks,) * min(i, 1), False), ("node_stage", False)]
        return ev
    ev += [("mp", r.ask_closing, r.fork, ragged, (r.masks,) * S, r.deferred), ("node_stage", r.deferred)]
    # a deferred job rides as tail workgroups where the library says "tail" (16-bit-core node kernels, never a ragged
    # job); elsewhere the node stage issues it on its own
    if r.deferred and not (form == "tail" and not ragged and ops.precision() != "fp32"):
        ev.append(("launch", "node-stage", False, ragged, embed, False))
    return ev


def route_of(case, x_dim=0, facts=None):
    """(route, the library's answer) for a case, from the test's own statement of the caller's facts."""
    from groupnet_amd import ops, route as R
    S, ragged = len(case["scales"]), case.get("counts") is not None
    masked = ops.incidence_form() == "mask" and R.masks_in_range(case["N"])
    facts = facts or R.StageFacts(grouped=case.get("grouped", True), latency_form=case.get("affinity_tail", True),
                                  capturing=case.get("capture", False), embed=False, may_defer=True)
    words = S if R.graph_stage_masks(S, masked, ragged) and not x_dim else 0     # the front-end's question leaves them out
    form = ops.graph_form(case["N"], D, x_dim, words)
    return R.graph_stage_route(S, form, case["B"] * case["N"], masked=masked, ragged=ragged,
                               training=case.get("training", False), facts=facts), form


def says(r, expect):
    return {k: getattr(r, k) for k in expect} == expect


# ---------------------------------------------------------------------------------------------------------------------
# the block
# ---------------------------------------------------------------------------------------------------------------------
def run_block(case, before=lambda: None):
    """One forward of a BLOCK_CASES case with seeded inputs and uniforms -> dict(f, out, new_H, counter)."""
    from groupnet_amd.multiscale import MultiScaleHGNN
    B, N, scales = case["B"], case["N"], case["scales"]
    training, dtype = case.get("training", False), case.get("dtype", torch.float32)
    torch.manual_seed(N)
    blk = MultiScaleHGNN(scales, grouped=case.get("grouped", True)).to(dev())
    blk.train(training)
    blk.affinity_tail = case.get("affinity_tail", True)
    gen = torch.Generator().manual_seed(B)
    f = torch.randn(B, N, D, generator=gen).to(dev()).to(dtype)
    U = [[torch.rand(s, generator=gen).to(dev())] for s in blk.noise_shapes(B, N)]
    counter = torch.zeros(1, dtype=torch.int64, device=dev())
    kw = dict(noise_u=U, n_agents=case.get("counts"), advance=None if training else (counter, ADVANCE))
    if case.get("capture"):
        side = torch.cuda.Stream(device=dev())
        side.wait_stream(torch.cuda.current_stream(dev()))
        with torch.no_grad(), torch.cuda.stream(side):      # packs the weights, sizes the pool
            blk(f, **kw)
        torch.cuda.current_stream(dev()).wait_stream(side)
        torch.cuda.synchronize()
        counter.zero_()
        graph = torch.cuda.CUDAGraph()
        before()
        with torch.no_grad(), torch.cuda.graph(graph):
            out, new_H = blk(f, **kw)
        graph.replay()
    else:
        before()
        with torch.enable_grad() if training else torch.no_grad():
            out, new_H = blk(f, **kw)
    torch.cuda.synchronize()
    return dict(f=f, out=out, new_H=new_H, counter=int(counter.item()))


@pytest.mark.parametrize("name", list(BLOCK_CASES))
def test_block_follows_the_graph_stage_route(name, monkeypatch):
    from groupnet_amd import ops
    case, expect = BLOCK_CASES[name]
    if case.get("mask_form"):
        monkeypatch.setattr(ops, "_INCIDENCE_FORM", "mask")
    B, N, S = case["B"], case["N"], len(case["scales"])
    training, ragged = case.get("training", False), case.get("counts") is not None
    r, form = route_of(case)
    assert says(r, expect), (r, expect)
    if name == "tail":
        assert form == "tail"
    calls, seen = record(monkeypatch)
    got = run_block(case, before=lambda: (calls.clear(), seen.clear()))
    assert calls == stated(r, form, S, ragged=ragged, advance=not training,
                           one_call=training or case.get("grouped", True)), (calls, r)
    f, out, new_H = got["f"], got["out"], got["new_H"]
    assert out.shape == (B, N, D * (2 + S)) and torch.equal(out[..., :D], f)
    assert bool(out.requires_grad) == training                   # a training forward concatenates: no final is written
    assert got["counter"] == (0 if training else ADVANCE)         # ... and leaves the counter to its caller
    Hs = [H for _, hs in seen for H in hs]
    assert len(Hs) == S and all(x is f or training for x, _ in seen)
    if S:
        assert new_H.dtype == f.dtype and torch.equal(new_H, torch.cat(Hs, dim=1).to(f.dtype))
    else:
        assert new_H is None


# ---------------------------------------------------------------------------------------------------------------------
# the encoders
# ---------------------------------------------------------------------------------------------------------------------
def run_encoder(case, before=lambda: None, future=False):
    """One eval forward of an ENCODER_CASES case, seeded device noise -> dict(out, new_H, counter)."""
    from groupnet_amd import MS_HGNN_batch as M
    from test_past_encoder import _inputs, make, make_future
    B, N, scales = case["B"], case["N"], case["scales"]
    enc = (make_future if future else make)(scales, seed=N).to(dev())
    gen = torch.Generator().manual_seed(B)
    x = _inputs(B, N, 10 if future else T, gen).to(dev())
    counter = torch.zeros(1, dtype=torch.int64, device=dev())
    enc._advance = (counter, ADVANCE)
    prev = (M._NoiseState.mode, M._NoiseState.seed, M._NoiseState.offset, M._NoiseState.counter)
    M.set_noise_mode("device", seed=7)
    try:
        before()
        with torch.no_grad():
            if future:
                past = torch.randn(B * N, D * (2 + len(scales)), generator=gen).to(dev())
                out, new_H = enc(x, B, N, past), None
            else:
                out, new_H = enc(x, B, N)
        torch.cuda.synchronize()
    finally:
        M.set_noise_mode(*prev)
    return dict(out=out, new_H=new_H, counter=int(counter.item()))


@pytest.mark.parametrize("name", list(ENCODER_CASES))
def test_past_encoder_follows_the_graph_stage_route(name, monkeypatch):
    from groupnet_amd import ops, route as R
    case, expect = ENCODER_CASES[name]
    if case.get("mask_form"):
        monkeypatch.setattr(ops, "_INCIDENCE_FORM", "mask")
    B, N, S = case["B"], case["N"], len(case["scales"])
    facts = R.StageFacts(grouped=True, latency_form=False, capturing=False, embed=True, may_defer=False)
    r, form = route_of(case, x_dim=T * IN_DIM, facts=facts)
    assert says(r, {**expect, **ENCODER_ALWAYS}), (r, expect)
    assert (form == "banded") == (N == ENCODER_BANDED_N)
    calls, seen = record(monkeypatch)
    got = run_encoder(case, before=lambda: (calls.clear(), seen.clear()))
    assert calls == stated(r, form, S, embed=r.kind == R.FUSED), (calls, r)
    (f, Hs), = seen
    assert got["out"].shape == (B * N, D * (2 + S)) and torch.equal(got["out"].view(B, N, -1)[..., :D], f)
    assert got["counter"] == ADVANCE and len(Hs) == S             # at S = 0 the launch's all-ones edge is dropped
    if S > 1:
        assert torch.equal(got["new_H"], torch.cat(Hs, dim=1))
    else:
        assert got["new_H"] is None


def test_future_encoder_follows_the_graph_stage_route(monkeypatch):
    """The same `_encode` behind the second drop-in: launched at once, no tail, no closing stage."""
    from groupnet_amd import route as R
    case = dict(B=2, N=11, scales=[5, 11])
    facts = R.StageFacts(grouped=True, latency_form=False, capturing=False, embed=True, may_defer=False)
    r, form = route_of(case, x_dim=10 * IN_DIM, facts=facts)
    assert says(r, dict(kind="fused", **ENCODER_ALWAYS))
    calls, seen = record(monkeypatch)
    got = run_encoder(case, before=lambda: (calls.clear(), seen.clear()), future=True)
    assert calls == stated(r, form, 2, embed=True), (calls, r)
    assert got["counter"] == ADVANCE and torch.isfinite(got["out"]).all()
