"""`run_message_passing` follows `route.message_passing_route`: the seven `ops.*_grouped` entry points (and
`ops.agg_mlp_closing`, through which the engine asks for the closing stage) are wrapped with recording pass-throughs, one
forward runs per case, and the recorded calls — which launch, which modules it carries, which Spec each item is — are
the ones the route states.  The cases are the smallest that sit on each boundary of the route."""
import pytest
import torch

from launch_forms import K_HYPER, K_PAIR, expected_forms

pytestmark = pytest.mark.gpu

B = 3
GROUPED = ("node_stage_grouped", "node2edge_grouped", "edge_mlp_gumbel_grouped", "agg_gather_grouped", "agg_mlp_grouped",
           "agg_scatter_grouped", "mlp2_grouped")


def dev():
    return torch.device("cuda:0")


def record(monkeypatch):
    """Wrap the entry points; -> the list their calls are appended to, as (name, items, further arguments, result)."""
    from groupnet_amd import ops
    calls = []

    def wrap(name):
        real = getattr(ops, name)

        def through(items, *args, **kwargs):
            out = real(items, *args, **kwargs)
            calls.append((name, list(items), args, out))
            return out
        monkeypatch.setattr(ops, name, through)
    for name in GROUPED + ("agg_mlp_closing",):
        wrap(name)
    return calls


def module_of(H, N):
    """Which module an item belongs to, from its incidence: 'pair', or the hyper module's E (scales [2, N]: N and 1)."""
    return "pair" if H is None else H.shape[1]


def expected_calls(rt, names, N, nmp=1):
    """The calls of a forward that follows `rt`, up to the closing stage of each round (which the launcher's plan may
    take): (name, what the call carries)."""
    from groupnet_amd import ops, route as R
    sub = lambda idx: [names[i] for i in idx]
    src = {R.PAIR: ops.PairSpec, R.PAIR_NODE: ops.PairSpec, R.SCENE: ops.GatherSpec, R.TWIN_PAIR: ops.GatherSpec,
           R.FUSED_GATHER: ops.GatherSpec, R.EO: torch.Tensor}
    clo = {R.NODE_AGG: ops.NodeAggSpec, R.SCATTER_SPEC: ops.ScatterSpec, R.SCATTER: torch.Tensor}
    one = [("node_stage_grouped", [m.first_layer for m in rt.modules])]
    if rt.node2edge:
        one.append(("node2edge_grouped", (sub(rt.node2edge), rt.masks)))
    one.append(("edge_mlp_gumbel_grouped", [ops.PoolSpec if m.pool_in_edge_kernel else torch.Tensor for m in rt.modules]))
    if rt.gather:
        one.append(("agg_gather_grouped", (sub(rt.gather), rt.masks)))
    if rt.ask_closing:
        one.append(("agg_mlp_closing", [(src[m.source], m.node_form) for m in rt.modules]))
    tail = [("agg_mlp_grouped", [(src[m.source], m.node_form) for m in rt.modules])]
    if rt.scatter:
        tail.append(("agg_scatter_grouped", (sub(rt.scatter), rt.masks)))
    tail.append(("mlp2_grouped", [clo[m.closing_input] for m in rt.modules]))
    return one, tail


def carried(call, N):
    """A recorded call in the terms of `expected_calls`."""
    from groupnet_amd import ops
    name, items, args, _ = call
    kind = lambda x: type(x) if isinstance(x, (ops.PoolSpec, ops.PairSpec, ops.GatherSpec, ops.NodeAggSpec, ops.ScatterSpec)) \
        else torch.Tensor
    hyper_masks = lambda H, mk: [m is not None for h, m in zip(H, mk) if h is not None]
    if name == "node_stage_grouped":
        return name, [s is not None for s in args[1]]
    if name == "node2edge_grouped":
        Hs, mks = [it[2] for it in items], [it[6] for it in items]
    elif name == "agg_gather_grouped":
        Hs, mks = [it[1] for it in items], [it[3] for it in items]
    elif name == "agg_scatter_grouped":
        Hs, mks = [it[1] for it in items], [it[4] for it in items]
    elif name in ("agg_mlp_grouped", "agg_mlp_closing"):
        return name, [(kind(it[0]), bool(getattr(it[0], "node", False))) for it in items]
    else:
        return name, [kind(it[0]) for it in items]
    assert all(m is None for h, m in zip(Hs, mks) if h is None), "masks belong to hyper modules"
    got = hyper_masks(Hs, mks)
    assert len(set(got)) <= 1, "every hyper module of a launch in one form"
    return name, ([module_of(H, N) for H in Hs], bool(got and got[0]))


def check_follows(calls, rt, names, N, nmp=1, fused=None):
    """`calls` is `nmp` rounds of the route's calls; fused (where known): whether the launcher takes the closing stage."""
    one, tail = expected_calls(rt, names, N)
    got = [carried(c, N) for c in calls]
    want = []
    taken = [c[3] is not None for c in calls if c[0] == "agg_mlp_closing"]
    assert len(taken) == (nmp if rt.ask_closing else 0), "the closing stage is asked once per round, where the route asks"
    if fused is not None:
        assert all(t == fused for t in taken), (taken, fused)
    for r in range(nmp):
        want += one + ([] if rt.ask_closing and taken[r] else tail)
    assert got == want, "\n".join(f"{g}\n{w}" for g, w in zip(got, want))


def engine_route(N, modules, dtype, training, closing_asked):
    from groupnet_amd import MS_HGNN_batch as M, ops, route as R
    return R.message_passing_route(
        N, tuple(modules), twin=dtype == torch.bfloat16, training=training, matrix16=ops.BF16X6,
        knobs=R.Knobs(M._FUSE_POOL, ops.POOL_MAX_N, ops.node_form_enabled(), ops.incidence_form() == "mask"),
        closing_asked=closing_asked)


def run_block(N, dtype, training, monkeypatch, mask_form=False):
    from groupnet_amd import ops
    from groupnet_amd.multiscale import MultiScaleHGNN
    if mask_form:
        monkeypatch.setattr(ops, "_INCIDENCE_FORM", "mask")
    torch.manual_seed(N)
    blk = MultiScaleHGNN([2, N]).to(dev())
    blk.train(training)
    f = torch.randn(B, N, 64, device=dev()).to(dtype)
    U = [[torch.rand(s, device=dev())] for s in blk.noise_shapes(B, N)]
    calls = record(monkeypatch)
    with torch.enable_grad() if training else torch.no_grad():
        out, _ = blk(f, noise_u=U)
    torch.cuda.synchronize()
    assert bool(out.requires_grad) == training
    # the block asks for the closing stage in its latency form (the default); a training forward never does
    rt = engine_route(N, [(True, K_PAIR), (False, K_HYPER), (False, K_HYPER)], dtype, training, closing_asked=not training)
    forms = expected_forms(B, N, [2, N], ops.precision(), "bf16" if dtype == torch.bfloat16 else "fp32", training)
    assert [m.node_form for m in rt.modules] == [g["node_form"] for g in forms["groups"]]
    check_follows(calls, rt, ["pair", N, 1], N, fused=forms["fused_closing"])
    return rt


@pytest.mark.parametrize("N", [16, 17])
def test_fp32_forward_follows_the_route(N, monkeypatch):
    rt = run_block(N, torch.float32, False, monkeypatch)
    assert (rt.gather, rt.scatter) == (((), ()) if N == 16 else ((1, 2), (0, 1, 2)))


@pytest.mark.parametrize("N", [64, 65])
def test_twin_forward_follows_the_route(N, monkeypatch):
    from groupnet_amd import route as R
    rt = run_block(N, torch.bfloat16, False, monkeypatch)
    assert rt.modules[0].source == (R.SCENE if N == 64 else R.TWIN_PAIR) and rt.scatter == ((1, 2) if N == 64 else (0, 1, 2))


@pytest.mark.parametrize("N", [11, 17])
def test_training_forward_follows_the_route(N, monkeypatch):
    rt = run_block(N, torch.float32, True, monkeypatch)
    assert rt.node2edge == (0, 1, 2) and not rt.ask_closing


def test_mask_form_forward_follows_the_route(monkeypatch):
    rt = run_block(17, torch.float32, False, monkeypatch, mask_form=True)
    assert rt.masks and rt.node2edge == (1, 2)


def test_one_hyper_module_follows_the_route(monkeypatch):
    from groupnet_amd.MS_HGNN_batch import MS_HGNN_hyper
    N = 11
    torch.manual_seed(3)
    mod = MS_HGNN_hyper(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=1,
                        scale=2).to(dev()).eval()
    h, corr = torch.randn(B, N, 64, device=dev()), torch.randn(B, N, N, device=dev())
    calls = record(monkeypatch)
    with torch.no_grad():
        mod(h, corr, noise_u=torch.rand(B, N, K_HYPER, device=dev()))
    torch.cuda.synchronize()
    rt = engine_route(N, [(False, K_HYPER)], torch.float32, False, closing_asked=False)
    check_follows(calls, rt, [N], N)
    assert not rt.ask_closing and (rt.node2edge, rt.gather, rt.scatter) == ((), (), ())
