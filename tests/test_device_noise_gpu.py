"""The in-kernel Philox draws of every edge kernel, pinned to the stream.

Device noise mode draws the Gumbel uniforms inside the edge kernel: element (row, k) of a (B, E, K) draw is element
host offset + device counter + row*K + k of the Philox4x32-10 stream `seed` (oracle.philox_uniform; gn_philox_uniform_f32
is its device twin).  A wrong draw gives no NaN and no parity failure, only other samples, so every check here is a direct
comparison:

  a. the stand-alone generator against the numpy oracle, bit for bit, at the table's positions and with a device counter;
  b. every edge kernel x every case of tests/device_noise_cases.py: the launch fed `PhiloxNoise` against the SAME launch
     fed the tensor `philox_uniform` writes for those positions — same kernel, same inputs, so `torch.equal`;
  c. one grouped launch of the production shape (pairwise + two hyper groups at their own offsets), per kernel;
  d. the f16x3 range-vote fallback, whose second pass draws again;
  e. the host bookkeeping (per-module offsets, module-major order over the rounds, graph replays and their counter
     convention, training, shards) against offsets written out by hand, and against the float64-free CPU oracle at the
     gates the suite already applies (TOL of test_parity_gpu.py, TOL_ORACLE of test_bf16_gpu.py, 1e-6 where the launch
     forms differ).

Every test prints one line per launch compared: kernel, case, rows and how many rows took which route of fetch_uniforms.
Shapes are a few hundred rows at the most.  No MI355X timing figure was available when these tests were specified.
Measured since on an MI355X: the whole file (280 tests) in 3.5 s, the slowest single test 0.30 s (the first launch of
the process), every other one 0.16 s or less.
"""
import ctypes

import numpy as np
import pytest
import torch

from device_noise_cases import (KERNEL_CASES, KERNELS, M64, POSITION_CASES, SEED_ALL, SEED_HI, SEED_TOP, STEP, describe,
                                draw_route, effective_base, ordered_edges, select_kernel)
from oracle import ms_hgnn_oracle as O
from test_bf16_gpu import TOL_ORACLE, relerr, safe_rows
from test_parity_gpu import TOL, maxerr

pytestmark = pytest.mark.gpu

def dev():
    return torch.device("cuda:0")


def _counter(value):
    return None if value is None else torch.tensor([value], dtype=torch.int64, device=dev())


def _oracle(shape, seed, base):
    n = int(np.prod(shape))
    return torch.from_numpy(O.philox_uniform(n, seed, base & M64)).view(*shape)


def _spy_edge_plans(monkeypatch, log):
    """Ask the library, at every edge launch, for the plan of that launch with the very arguments the product passes
    (static LDS from the runtime, as the launcher does): log gets (rc, kernel name, precision)."""
    from groupnet_amd import _lib, ops
    real = ops._fn

    def fn(stem, dt):
        f = real(stem, dt)
        if stem != "gn_edge_mlp_gumbel":
            return f

        def call(*a):
            plan = _lib.LaunchPlan()
            rc = real(stem + "_plan", dt)(*a[:-1], -1, ctypes.byref(plan))
            log.append((rc, (_lib.load().gn_kernel_name(plan.kernel) or b"").decode(), plan.precision))
            return f(*a)
        return call
    monkeypatch.setattr(ops, "_fn", fn)


def _assert_kernel(plans, kernel, launches):
    assert len(plans) == launches, plans
    assert all(p == (0, kernel.plan_kernel, kernel.plan_precision) for p in plans), (kernel.id, plans)


def _same(a, b):
    """Outputs [(edge_feat, dist or None)] of two launches are bit-identical."""
    assert len(a) == len(b)
    for (ef_a, d_a), (ef_b, d_b) in zip(a, b):
        if not torch.equal(ef_a, ef_b):
            return False
        if (d_a is None) != (d_b is None) or (d_a is not None and not torch.equal(d_a, d_b)):
            return False
    return True


# ---- a. the stand-alone generator --------------------------------------------------------------------------------------
def test_standalone_generator_matches_the_oracle_at_the_carries():
    """Host offset alone, and host offset + device counter, at every position case: spans over 2^32, over 2^34 (block
    index 2^32) and the wrapped sum of the graphs' counter convention."""
    from groupnet_amd import ops
    held = []                                 # (no buffer is handed out twice: a skipped element cannot look right)
    for c in POSITION_CASES:
        n, base = c.B * ordered_edges(c) * c.K, effective_base(c)
        want = O.philox_uniform(n, c.seed, base)
        u = ops.philox_uniform((n,), c.seed, base, dev())
        held.append(u)
        assert np.array_equal(u.cpu().numpy(), want), (c.id, "host offset")
        if c.counter is not None:
            v = ops.philox_uniform((n,), c.seed, c.offset, dev(), offset_dev=_counter(c.counter))
            held.append(v)
            assert np.array_equal(v.cpu().numpy(), want), (c.id, "offset + counter")
        print(f"\nphilox_uniform_kernel: {c.id}, {n} elements at {base:#x}"
              f"{'' if c.counter is None else f' = {c.offset:#x} + counter {c.counter}'}", end="")


@pytest.mark.parametrize("n", [1, 2, 5, 4 * 7 + 2])
def test_standalone_generator_with_a_device_counter_at_every_residue(n):
    """With a device-side base the launcher cannot know the first block's fill and sizes the launch with one spare
    block: every residue of (offset + counter) mod 4, offsets of every residue, small and carrying counters, and the
    counter one step back."""
    from groupnet_amd import ops
    held, seen = [], set()
    splits = [(10, 2), (11, 1 << 20), (12, (1 << 32) - 9), (13, (1 << 34) - 14), ((1 << 33) + 2, (1 << 33) - 3)]
    for off0, ctr0 in splits:
        for r in range(4):
            off, ctr = off0, ctr0 + r
            base = (off + ctr) & M64
            u = ops.philox_uniform((n,), SEED_HI, off, dev(), offset_dev=_counter(ctr))
            held.append(u)
            assert np.array_equal(u.cpu().numpy(), O.philox_uniform(n, SEED_HI, base)), (n, off, ctr)
            seen.add((off & 3, base & 3))
    for r in range(4):                        # counter = -d, offset = d + r: position r modulo 2^64
        u = ops.philox_uniform((n,), SEED_TOP, STEP + r, dev(), offset_dev=_counter(-STEP))
        held.append(u)
        assert np.array_equal(u.cpu().numpy(), O.philox_uniform(n, SEED_TOP, r)), (n, r)
    assert {b for _, b in seen} == {0, 1, 2, 3} and {o for o, _ in seen} == {0, 1, 2, 3}
    print(f"\nphilox_uniform_kernel with offset_dev: n = {n}, {len(held)} draws, every residue of the base", end="")


# ---- b. every kernel x every case ------------------------------------------------------------------------------------
def _edge_module(K):
    from groupnet_amd.MS_HGNN_batch import MLP_dict_softmax
    torch.manual_seed(100 + K)
    return MLP_dict_softmax(64, 64, (128,), edge_types=K).to(dev())


@pytest.mark.parametrize("case", KERNEL_CASES, ids=[c.id for c in KERNEL_CASES])
@pytest.mark.parametrize("kernel", KERNELS, ids=[k.id for k in KERNELS])
def test_edge_kernel_draws_the_stream(kernel, case, monkeypatch):
    """PhiloxNoise(seed, offset, counter) against the tensor of the same positions through the same kernel: exact.  The
    tensor itself is checked against the numpy oracle, and the tensor one position further must give another result
    (K = 1 excepted: a one-type softmax is 1 whatever the noise, so there the draw cannot be observed at all)."""
    from groupnet_amd import ops
    dtype = select_kernel(kernel, monkeypatch)
    plans = []
    _spy_edge_plans(monkeypatch, plans)
    K, B, Eo, base = case.K, case.B, ordered_edges(case), effective_base(case)
    pk = _edge_module(K)._packed()
    torch.manual_seed(7 + case.B * case.E)
    edges = torch.randn(B, case.E, 64, device=dev()).to(dtype)
    U = ops.philox_uniform((B, Eo, K), case.seed, base, dev())
    assert torch.equal(U.cpu(), _oracle((B, Eo, K), case.seed, base))

    def run(u):
        return ops.edge_mlp_gumbel_grouped([(edges, u, pk, K, case.sym_N, case.want_dist)])
    from_tensor = run(U)
    in_kernel = run(ops.PhiloxNoise(case.seed, case.offset, _counter(case.counter)))
    shifted = run(ops.philox_uniform((B, Eo, K), case.seed, (base + 1) & M64, dev()))
    print("\n" + describe(kernel, case), end="")
    _assert_kernel(plans, kernel, 3)
    (ef, dist), = from_tensor
    assert ef.shape == (B, case.E, K) and bool(torch.isfinite(ef).all())
    assert (dist is None) == (bool(case.sym_N) and not case.want_dist)
    assert dist is None or (dist.shape == (B, Eo, K) and dist.dtype == dtype)
    assert _same(from_tensor, in_kernel), f"{kernel.name} drew other uniforms than the stream holds ({case.id})"
    if K > 1:
        a, b = (ef, shifted[0][0]) if dist is None else (dist, shifted[0][1])
        assert not torch.equal(a, b), "the comparison is blind: shifted uniforms give the same result"


# ---- c. the production shape in one grouped launch --------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS, ids=[k.id for k in KERNELS])
def test_grouped_launch_draws_every_group_at_its_own_offset(kernel, monkeypatch):
    """Pairwise (K = 6, unordered pairs), hyper with E = N and hyper with E = 1 (K = 10) in ONE launch, sharing seed and
    counter, their spans back to back as `noise_shapes` lays them out.  Rows formed in the kernel (PoolSpec) where the
    kernel can, read from `edges` on the fp32 cores."""
    from groupnet_amd import ops
    from groupnet_amd.multiscale import MultiScaleHGNN
    dtype = select_kernel(kernel, monkeypatch)
    plans = []
    _spy_edge_plans(monkeypatch, plans)
    torch.manual_seed(51)
    B, N, scales = 5, 11, [5, 11]
    blk = MultiScaleHGNN(scales).to(dev()).eval()
    f = torch.randn(B, N, 64, device=dev()).to(dtype)
    shapes = blk.noise_shapes(B, N)
    assert shapes == [(5, 121, 6), (5, 11, 10), (5, 1, 10)]
    seed, off0, ctr = SEED_TOP, 17, 1 << 33
    offs = [off0, off0 + 3630, off0 + 3630 + 550]          # 5 * 121 * 6 = 3630, 5 * 11 * 10 = 550: residues 1, 3, 1 (pair rows at o = 1 and 3)
    with torch.no_grad():
        _, Hs, _ = ops.affinity_topk(f, scales, want_corr=False)
        mods = [blk.interaction, *blk.interaction_hyper]
        rows = []
        for m, H in zip(mods, [None, *Hs]):
            pk = m._packed_n2e(0)
            xp, pq = ops.node_mlp(f, pk)
            sym = H is None
            rows.append(ops.PoolSpec(xp, pq, H, pk["w2"], pk["b2"], sym) if kernel.pool
                        else ops.node2edge(xp, pq, H, pk["w2"], pk["b2"], sym))

        def run(noise):
            return ops.edge_mlp_gumbel_grouped([(r, u, m.nmp_mlp_start._packed(), m.edge_types, N if H is None else 0, True)
                                                for r, u, m, H in zip(rows, noise, mods, [None, *Hs])])
        counter = _counter(ctr)
        in_kernel = run([ops.PhiloxNoise(seed, o, counter) for o in offs])
        U = [ops.philox_uniform(s, seed, o + ctr, dev()) for s, o in zip(shapes, offs)]
        for u, s, o in zip(U, shapes, offs):
            assert torch.equal(u.cpu(), _oracle(s, seed, o + ctr))
        from_tensor = run(U)
        U[2] = ops.philox_uniform(shapes[2], seed, offs[2] + ctr + 1, dev())
        third_shifted = run(U)
    _assert_kernel(plans, kernel, 3)
    for g in range(3):
        assert _same(from_tensor[g:g + 1], in_kernel[g:g + 1]), f"group {g} of the grouped launch ({kernel.name})"
    assert _same(from_tensor[:2], third_shifted[:2]) and not torch.equal(from_tensor[2][1], third_shifted[2][1])
    routes = [dict((r, sum(draw_route(s[2], (o + ctr + i * s[2]) & M64) == r for i in range(s[0] * s[1])))
                   for r in ("swap", "runs", "runs_cross")) for s, o in zip(shapes, offs)]
    print(f"\n{kernel.name}: grouped launch, {'PoolSpec' if kernel.pool else 'edges'} rows "
          f"{[B * 66, B * 11, B]}, ordered {[s[0] * s[1] for s in shapes]}, routes {routes}", end="")


# ---- d. the fallback pass draws again --------------------------------------------------------------------------------
def _record_edge_outputs(monkeypatch, log):
    from groupnet_amd import ops
    real = ops.edge_mlp_gumbel_grouped

    def record(items, *a, **k):
        outs = real(items, *a, **k)
        log.append([t.clone() for pair in outs for t in pair if t is not None])
        return outs
    monkeypatch.setattr(ops, "edge_mlp_gumbel_grouped", record)
    return real


@pytest.mark.parametrize("variant", ["all", "some"])
def test_fallback_pass_draws_from_the_same_positions(variant, monkeypatch):
    """f16x3 with rows beyond the fp16 range: the workgroups that meet one run the whole body, draws included, a second
    time on the bf16x6 path.  "all": the inputs of test_fallback_stages_again_over_a_used_ring (every workgroup falls
    back), where that test demands the bf16x6 mode's bits — so the in-kernel draws of both modes and both tensor-fed runs
    are one result.  "some": the inputs of test_partial_fallback_matches_the_oracle (four scenes out of range)."""
    from groupnet_amd import ops
    from groupnet_amd.multiscale import MultiScaleHGNN
    f16x3 = next(k for k in KERNELS if k.id == "f16x3")
    select_kernel(f16x3, monkeypatch)
    monkeypatch.setattr(ops, "POOL_MAX_N", ops.POOL_KERNEL_MAX_N)
    if variant == "all":
        torch.manual_seed(43)
        B, N, scales = 40, 11, [2, 5]
        blk = MultiScaleHGNN(scales).to(dev()).eval()
        f = torch.randn(B, N, 64, device=dev()) * 1.0e6
    else:
        torch.manual_seed(44)
        B, N, scales = 48, 11, [2, 5, 11]
        blk = MultiScaleHGNN(scales).to(dev()).eval()
        h = torch.randn(B, N, 64)
        h[[3, 17, 18, 40]] *= 1.0e6
        f = h.to(dev())
    seed, offs, cur = SEED_ALL, [], (1 << 32) - 1000
    shapes = blk.noise_shapes(B, N)
    for b, e, k in shapes:
        offs.append(cur)
        cur += b * e * k
    U = [[ops.philox_uniform(s, seed, o, dev())] for s, o in zip(shapes, offs)]
    P = [[ops.PhiloxNoise(seed, o)] for o in offs]
    got = {}
    for mode in ("f16x3", "bf16x6"):
        ops.set_precision(mode)
        for name, noise in (("tensor", U), ("kernel", P)):
            log = []
            real = _record_edge_outputs(monkeypatch, log)
            with torch.no_grad():
                out, H = blk(f, noise_u=noise)
            monkeypatch.setattr(ops, "edge_mlp_gumbel_grouped", real)
            assert len(log) == 1 and bool(torch.isfinite(out).all())
            got[mode, name] = (out.clone(), H.clone(), log[0])

    def same(a, b):
        return (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and len(a[2]) == len(b[2])
                and all(torch.equal(x, y) for x, y in zip(a[2], b[2])))
    for mode in ("f16x3", "bf16x6"):
        assert same(got[mode, "tensor"], got[mode, "kernel"]), f"{mode}: in-kernel draws differ from the stream ({variant})"
    if variant == "all":
        assert same(got["f16x3", "kernel"], got["bf16x6", "kernel"]) and same(got["f16x3", "tensor"], got["bf16x6", "tensor"])
    else:
        assert not same(got["f16x3", "kernel"], got["bf16x6", "kernel"])      # (the in-range workgroups stayed on fp16)
    print(f"\nedge_x_kernel<2,float> with fallback ({variant} rows out of range): rows {[s[0] * s[1] for s in shapes]} ordered, "
          f"offsets {[hex(o) for o in offs]}", end="")


# ---- e. host bookkeeping ---------------------------------------------------------------------------------------------
MODES = ["fp32", "bf16x6", "f16x3", "bf16"]
SCALES = [2, 5, 11]
# B = 6, N = 11: one draw of the pairwise module is 6 * 121 * 6 = 4356 uniforms, of the hyper modules 6 * 11 * 10 = 660,
# 660 and (scale = N: one hyperedge) 6 * 1 * 10 = 60.  Module-major, round by round inside a module, pairwise first:
SHAPES_B6 = [(6, 121, 6), (6, 11, 10), (6, 11, 10), (6, 1, 10)]
OFFSETS_B6 = {1: ([[0], [4356], [5016], [5676]], 5736),
              2: ([[0, 4356], [8712, 9372], [10032, 10692], [11352, 11412]], 11472)}
SEED_E, OFF_E = SEED_TOP, 1123


def _mode(mode, monkeypatch):
    from groupnet_amd import ops
    monkeypatch.setattr(ops, "BF16X6", ops.BF16X6)
    monkeypatch.setattr(ops, "F16X3", ops.F16X3)
    monkeypatch.delenv("GN_EDGE_RB2", raising=False)
    if mode != "bf16":
        ops.set_precision(mode)
    return torch.bfloat16 if mode == "bf16" else torch.float32


def _block(nmp, seed=61):
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(seed)
    blk = MultiScaleHGNN(SCALES, nmp_layers=nmp)
    sp = {k: v.detach().clone() for k, v in blk.interaction.state_dict().items()}
    shs = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in blk.interaction_hyper]
    return blk.to(dev()).eval(), sp, shs


def _tensors(shapes, offsets, base):
    from groupnet_amd import ops
    return [[ops.philox_uniform(s, SEED_E, base + o, dev()) for o in per] for s, per in zip(shapes, offsets)]


@pytest.fixture
def device_noise():
    """set_noise_mode('device', ...) for the test, the default host mode afterwards."""
    import groupnet_amd as G
    yield G.set_noise_mode
    G.set_noise_mode("host", seed=0, offset=0)


@pytest.mark.parametrize("nmp", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_block_in_device_mode_draws_at_the_offsets_written_out_by_hand(mode, nmp, monkeypatch, device_noise):
    from groupnet_amd import MS_HGNN_batch as M
    dtype = _mode(mode, monkeypatch)
    blk, sp, shs = _block(nmp)
    B, N = 6, 11
    assert blk.noise_shapes(B, N) == SHAPES_B6
    offsets, total = OFFSETS_B6[nmp]
    torch.manual_seed(62)
    h = torch.randn(B, N, 64).to(dtype)
    f = h.to(dev())
    device_noise("device", seed=SEED_E, offset=OFF_E)
    with torch.no_grad():
        out_d, H_d = blk(f)
        assert M._NoiseState.offset == OFF_E + total
        out_t, H_t = blk(f, noise_u=_tensors(SHAPES_B6, offsets, OFF_E))
    assert torch.equal(out_d, out_t) and torch.equal(H_d, H_t)
    # the same forward on the CPU oracle with the numpy stream at those offsets
    Uo = [[_oracle(s, SEED_E, OFF_E + o) for o in per] for s, per in zip(SHAPES_B6, offsets)]
    with torch.no_grad():
        ref, Href, corr = O.ms_hgnn_multiscale_forward(sp, shs, SCALES, h.float(), Uo[0], Uo[1:], decomposed=True,
                                                       nmp_layers=nmp)
    if dtype == torch.float32:
        err = maxerr(out_d, ref)
        assert torch.equal(H_d.cpu(), Href)
        gate = TOL
    else:
        err = max(relerr(out_d[..., 64 * (1 + i):64 * (2 + i)], ref[..., 64 * (1 + i):64 * (2 + i)]) for i in range(4))
        row0 = 0
        for s in SCALES:
            E = 1 if s == N else N
            ok = safe_rows(corr, s) if s != N else torch.ones(B, E, dtype=torch.bool)
            assert torch.equal(H_d.float().cpu()[:, row0:row0 + E][ok], Href[:, row0:row0 + E][ok])
            row0 += E
        gate = TOL_ORACLE
    print(f"\nblock in device mode, {mode}, nmp_layers {nmp}: rows {[s[0] * s[1] for s in SHAPES_B6]} ordered x {nmp} rounds, "
          f"{total} draws from {OFF_E}; against the oracle {err:.2e} (gate {gate:g})", end="")
    assert err <= gate


@pytest.mark.parametrize("nmp", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_graph_replay_k_draws_at_k_steps(mode, nmp, monkeypatch):
    """The captured forward draws at offset 0 + device counter, the counter starting at -draws_per_step and advanced at the
    start of every replay: replay k equals the eager tensor-fed forward at k * draws_per_step."""
    from groupnet_amd.graphs import GraphedMultiScale
    dtype = _mode(mode, monkeypatch)
    blk, _, _ = _block(nmp)
    B, N = 6, 11
    offsets, total = OFFSETS_B6[nmp]
    torch.manual_seed(63)
    f = torch.randn(B, N, 64, device=dev()).to(dtype)
    g = GraphedMultiScale(blk, B, N, seed=SEED_E, dtype=dtype)
    assert g.draws_per_step == total
    for k in range(3):
        out, H = g(f)
        out, H = out.clone(), H.clone()
        assert int(g.counter.item()) == k * total
        with torch.no_grad():
            out_t, H_t = blk(f, noise_u=_tensors(SHAPES_B6, offsets, k * total))
        assert torch.equal(out, out_t) and torch.equal(H, H_t), f"replay {k} ({mode}, nmp_layers {nmp})"
    print(f"\ngraph replays 0..2, {mode}, nmp_layers {nmp}: rows {[s[0] * s[1] for s in SHAPES_B6]} ordered, {total} draws a step",
          end="")


@pytest.mark.parametrize("nmp", [1, 2])
@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "f16x3"])
def test_training_forward_in_device_mode_draws_at_the_same_offsets(precision, nmp, monkeypatch, device_noise):
    """blk.train()(f) under autograd against the tensor-fed inference forward (the gate of
    test_seeded_training_forward_sees_the_noise_of_the_seeded_inference_forward: the training path runs other forms).
    fp32 tensors: the bf16 twins are forward-only."""
    _mode(precision, monkeypatch)
    blk, _, _ = _block(nmp)
    B, N = 6, 11
    offsets, total = OFFSETS_B6[nmp]
    torch.manual_seed(64)
    f = torch.randn(B, N, 64, device=dev())
    with torch.no_grad():
        a, Ha = blk(f, noise_u=_tensors(SHAPES_B6, offsets, OFF_E))
    device_noise("device", seed=SEED_E, offset=OFF_E)
    try:
        b, Hb = blk.train()(f)
    finally:
        blk.eval()
    assert b.requires_grad and torch.equal(Ha, Hb)
    err = float((a - b.detach()).abs().max())
    print(f"\ntraining forward in device mode, {precision}, nmp_layers {nmp}: rows {[s[0] * s[1] for s in SHAPES_B6]} ordered, "
          f"against the inference forward {err:.2e} (gate 1e-6)", end="")
    assert err <= 1e-6


@pytest.mark.parametrize("nmp", [1, 2])
@pytest.mark.parametrize("precision", ["fp32", "bf16x6", "f16x3"])
def test_shards_draw_their_rows_of_the_full_batch_stream(precision, nmp, monkeypatch, device_noise):
    """B = 5 split 2 | 3: a shard's draws start at  module's offset + first scene * E * K  in every round.  One draw of the
    full batch: 5 * 121 * 6 = 3630, 5 * 11 * 10 = 550, 550, 5 * 10 = 50; a scene: 726, 110, 110, 10.  Factors of the shard
    against its rows of the full batch at the 1e-6 of test_full_size_properties (other launch sizes, other summation order:
    no bit-identity owed); fp32 tensors (a bf16 factor is rounded to 8 bits after that)."""
    from groupnet_amd import multiscale, sharding
    _mode(precision, monkeypatch)
    blk, _, _ = _block(nmp)
    B, N = 5, 11
    sizes, scene = [3630, 550, 550, 50], [726, 110, 110, 10]
    torch.manual_seed(65)
    f = torch.randn(B, N, 64, device=dev())
    got = {}
    orig = multiscale.run_message_passing

    def spy(*a, **k):
        got["res"] = orig(*a, **k)
        return got["res"]
    monkeypatch.setattr(multiscale, "run_message_passing", spy)
    device_noise("device", seed=SEED_E, offset=OFF_E)
    with torch.no_grad():
        full, _ = blk(f)
    fac_full = [r[1].clone() for r in got["res"]]
    worst_fac = worst_feat = 0.0
    for start, stop in ((0, 2), (2, 5)):
        device_noise("device", seed=SEED_E, offset=OFF_E)
        noise = sharding.default_shard_noise(blk, B, N, start, stop, dev())
        want, cur = [], OFF_E
        for size, per_scene in zip(sizes, scene):
            want.append([cur + r * size + start * per_scene for r in range(nmp)])
            cur += nmp * size
        assert [[u.offset for u in per] for per in noise] == want
        assert all(u.seed == SEED_E and u.counter is None for per in noise for u in per)
        with torch.no_grad():
            part, _ = blk(f[start:stop].contiguous(), noise_u=noise)
        for a, b in zip(got["res"], fac_full):
            worst_fac = max(worst_fac, maxerr(a[1], b[start:stop]))
        worst_feat = max(worst_feat, maxerr(part, full[start:stop]))
    # (the comparison sees the offsets: scenes [2:5) drawing the rows of scenes [0:3) get other factors)
    device_noise("device", seed=SEED_E, offset=OFF_E)
    with torch.no_grad():
        blk(f[2:5].contiguous(), noise_u=sharding.default_shard_noise(blk, B, N, 0, 3, dev()))
    assert maxerr(got["res"][0][1], fac_full[0][2:5]) > 1e-3
    print(f"\nshards 2 | 3 of B = 5, {precision}, nmp_layers {nmp}: rows {[2 * 121, 22, 22, 2]} and {[3 * 121, 33, 33, 3]} ordered; "
          f"factors {worst_fac:.2e} (gate 1e-6), features {worst_feat:.2e} from the full batch", end="")
    assert worst_fac <= 1e-6
