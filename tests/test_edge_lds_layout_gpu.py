"""The edge kernel's pool stage lives in the LDS region of its weight ring (one dynamic allocation: stage first, ring
afterwards, one barrier in between; only what the largest stage needs beyond the ring is extra), and the f16x3 node stage
and edge kernel are compiled for three waves per SIMD.  Method of test_hyper_pool_stage_gpu.py: same inputs and injected
uniforms, GN_POOL_STAGE=0 (per-member reference form, no stage) against 1, bit for bit — on shapes whose largest stage is
smaller than the ring and larger than it, with ragged last workgroups and two message-passing rounds, in every mode; the
fallback pass, which stages AGAIN over a ring the first pass has used; and the residency the runtime grants."""
import ctypes

import pytest
import torch

from oracle import ms_hgnn_oracle as O

pytestmark = pytest.mark.gpu

RING_F32 = 36864        # weight ring of edge_x_kernel<2 | 3, float>: 3 chunks x 12 pieces x 1 KiB
CU_LDS = 160 * 1024


def dev():
    return torch.device("cuda:0")


# (B, N, scales, nmp_layers).  Stage bytes of a 128-row workgroup, fp32: hyper ((127 // E + 2) * N nodes x 272 B),
# pairwise (2 x ((127 // P + 2) * N) x 272 B, P = N (N + 1) / 2):
#   N = 3  : hyper E = 3: 35 904, pairwise 37 536 (> ring 36 864: 23 scenes of 6 pairs) — B = 5: a few rows only
#   N = 11 : hyper E = 11: 38 896 (> ring), pairwise 17 952 (< ring)
#   N = 16 : hyper E = 16: 39 168 (> ring), pairwise 17 408
#   N = 4  : hyper E = 4: 35 904, pairwise 30 464 — every stage below the ring
# B * E and B * P are no multiples of 128: the last workgroup of every group is ragged.
CASES = [(5, 3, [1, 2, 3], 1), (37, 4, [2, 4], 1), (300, 11, [2, 5, 11], 1), (150, 16, [3, 16], 1), (29, 11, [2, 5, 11], 2),
         (45, 4, [2, 3], 2)]
MODES = ["f16x3", "bf16x6", "bf16-rb1", "bf16-rb2"]


def _setup(mode, monkeypatch):
    from groupnet_amd import ops
    monkeypatch.setattr(ops, "BF16X6", ops.BF16X6)
    monkeypatch.setattr(ops, "F16X3", ops.F16X3)
    monkeypatch.setattr(ops, "POOL_MAX_N", ops.POOL_KERNEL_MAX_N)     # every hyper module here pools in the edge kernel
    if mode in ("f16x3", "bf16x6"):
        ops.set_precision(mode)
        return torch.float32
    monkeypatch.setenv("GN_EDGE_RB2", "1" if mode == "bf16-rb2" else "0")
    return torch.bfloat16


def _spy_launches(monkeypatch, log):
    """Ask the library, at every fp32 node-stage (with affinity tail) and edge launch, for the launch's dynamic LDS and
    the workgroups per CU the runtime grants: log gets (stem, rc, dyn_lds, wgs_per_cu)."""
    from groupnet_amd import ops
    from groupnet_amd._lib import load
    real = ops._fn

    def fn(stem, dt):
        f = real(stem, dt)
        if dt != torch.float32 or stem not in ("gn_edge_mlp_gumbel", "gn_node_mlp_affinity"):
            return f

        def call(*a):
            lds, occ = ctypes.c_size_t(0), ctypes.c_int(0)
            if stem == "gn_edge_mlp_gumbel":
                rc = load().gn_edge_mlp_gumbel_launch_info_f32(a[0], a[1], ctypes.byref(lds), ctypes.byref(occ))
            else:
                rc = load().gn_node_mlp_affinity_launch_info_f32(a[0], a[1], a[2], a[3], ctypes.byref(lds), ctypes.byref(occ))
            log.append((stem, rc, lds.value, occ.value))
            return f(*a)

        return call

    monkeypatch.setattr(ops, "_fn", fn)


def _forward(blk, f, U):
    with torch.no_grad():
        out, H = blk(f, noise_u=U)
    return out.clone(), H.clone()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,N,scales,nmp", CASES)
def test_stage_in_the_ring_region_is_bit_identical(B, N, scales, nmp, mode, monkeypatch):
    from groupnet_amd.multiscale import MultiScaleHGNN
    dtype = _setup(mode, monkeypatch)
    torch.manual_seed(41)
    blk = MultiScaleHGNN(scales, nmp_layers=nmp).to(dev()).eval()
    f = torch.randn(B, N, 64, device=dev()).to(dtype)
    U = [[torch.rand(s, device=dev()) for _ in range(nmp)] for s in blk.noise_shapes(B, N)]
    outs = {}
    for st in ("0", "1", "1"):          # (a second staged forward: nothing of the first one lingers)
        monkeypatch.setenv("GN_POOL_STAGE", st)
        got = _forward(blk, f, U)
        assert bool(torch.isfinite(got[0].float()).all())
        if st in outs:
            assert torch.equal(outs[st][0], got[0]) and torch.equal(outs[st][1], got[1])
        outs[st] = got
    assert torch.equal(outs["0"][0], outs["1"][0]) and torch.equal(outs["0"][1], outs["1"][1])


@pytest.mark.parametrize("B,N,scales,want", [(300, 11, [2, 5, 11], 38896), (150, 16, [3, 16], 39168), (37, 4, [2, 4], RING_F32),
                                              (5, 3, [1, 2, 3], 37536)])
def test_launcher_sizes_the_region_from_the_largest_stage(B, N, scales, want, monkeypatch):
    """Dynamic LDS of the fp32 edge launch = max(ring, largest stage that fits); GN_POOL_STAGE=0: the ring alone.  The
    scale = N group (one hyperedge per scene: (127 + 2) N nodes) never fits and keeps the global-memory form."""
    from groupnet_amd.multiscale import MultiScaleHGNN
    _setup("f16x3", monkeypatch)
    torch.manual_seed(42)
    blk = MultiScaleHGNN(scales).to(dev()).eval()
    f = torch.randn(B, N, 64, device=dev())
    U = [[torch.rand(s, device=dev())] for s in blk.noise_shapes(B, N)]
    for st, lds in (("1", want), ("0", RING_F32)):
        log = []
        monkeypatch.setenv("GN_POOL_STAGE", st)
        _spy_launches(monkeypatch, log)
        _forward(blk, f, U)
        monkeypatch.undo()
        _setup("f16x3", monkeypatch)
        edge = [e for e in log if e[0] == "gn_edge_mlp_gumbel"]
        assert edge and all(rc == 0 for _, rc, _, _ in edge), log
        assert [e[2] for e in edge] == [lds] * len(edge), log


def test_fallback_stages_again_over_a_used_ring(monkeypatch):
    """Inputs scaled so that every workgroup falls back (as test_f16x3_fallback_is_the_bf16x6_path): the fallback re-runs
    the whole body, i.e. fills the stage a second time over a ring the first pass has streamed 80 sub-steps through, then
    streams the bf16 image through it.  Hyper (38 896-byte stage: beyond the ring) and pairwise groups pool from the stage.
    Every output of the edge launch and the whole forward are bit-identical to the bf16x6 mode on the same inputs."""
    from groupnet_amd import ops
    from groupnet_amd.multiscale import MultiScaleHGNN
    _setup("f16x3", monkeypatch)
    torch.manual_seed(43)
    B, N, scales = 40, 11, [2, 5]
    blk = MultiScaleHGNN(scales).to(dev()).eval()
    f = torch.randn(B, N, 64, device=dev()) * 1.0e6
    U = [[torch.rand(s, device=dev())] for s in blk.noise_shapes(B, N)]
    real, real_fn = ops.edge_mlp_gumbel_grouped, ops._fn
    got = {}
    for mode in ("f16x3", "bf16x6"):
        edge_outs, log = [], []
        monkeypatch.setattr(ops, "_fn", real_fn)

        def record(items, *a, **k):
            outs = real(items, *a, **k)
            edge_outs.append([t.clone() for pair in outs for t in pair if t is not None])
            return outs

        monkeypatch.setattr(ops, "edge_mlp_gumbel_grouped", record)
        _spy_launches(monkeypatch, log)
        ops.set_precision(mode)
        got[mode] = (_forward(blk, f, U), edge_outs, log)
    (fa, ea, la), (fb, eb, lb) = got["f16x3"], got["bf16x6"]
    assert [e[2] for e in la if e[0] == "gn_edge_mlp_gumbel"] == [38896] and [e[2] for e in lb if e[0] == "gn_edge_mlp_gumbel"] == [38896]
    assert len(ea) == len(eb) == 1 and len(ea[0]) == len(eb[0]) >= 5
    for a, b in zip(ea[0], eb[0]):
        assert bool(torch.isfinite(a.float()).all()) and torch.equal(a, b)
    assert bool(torch.isfinite(fa[0]).all())
    assert torch.equal(fa[1], fb[1]) and torch.equal(fa[0], fb[0])


def test_partial_fallback_matches_the_oracle(monkeypatch):
    """Only some scenes are out of the fp16 range: the workgroups that hold one of their rows fall back (and with them the
    in-range rows they share a workgroup with), the others stay on the fp16 path; both pool from the stage.  Gate: the
    suite's 1e-5 (absolute) on every in-range scene; an out-of-range scene's features are ~1e5 .. 1e6, where an fp32 ulp is
    6e-2, so there the same 1e-5 is taken relative to the scene's own largest feature."""
    from groupnet_amd.multiscale import MultiScaleHGNN
    _setup("f16x3", monkeypatch)
    torch.manual_seed(44)
    B, N, scales = 48, 11, [2, 5, 11]
    blk = MultiScaleHGNN(scales)
    sp = {k: v.detach().clone() for k, v in blk.interaction.state_dict().items()}
    shs = [{k: v.detach().clone() for k, v in m.state_dict().items()} for m in blk.interaction_hyper]
    blk.to(dev()).eval()
    h = torch.randn(B, N, 64)
    big = torch.zeros(B, dtype=torch.bool)
    big[[3, 17, 18, 40]] = True                     # 128 pair rows ~ 2 scenes, 128 hyper rows ~ 12 scenes per workgroup
    h[big] *= 1.0e6
    noise = [[torch.rand(s)] for s in blk.noise_shapes(B, N)]
    with torch.no_grad():
        ref, Href, _ = O.ms_hgnn_multiscale_forward(sp, shs, scales, h, noise[0], noise[1:], decomposed=True)
    out, H = _forward(blk, h.to(dev()), [[u.to(dev()) for u in n] for n in noise])
    assert torch.equal(H.cpu(), Href)
    err = (out.cpu().double() - ref.double()).abs().flatten(1).max(1).values
    scale = ref.abs().flatten(1).max(1).values.double()
    print(f"\npartial fallback: in-range scenes max abs err {float(err[~big].max()):.2e}; out-of-range scenes max err / scale "
          f"{float((err[big] / scale[big]).max()):.2e}")
    assert bool(torch.isfinite(out).all())
    assert float(err[~big].max()) <= 1e-5
    assert bool((err[big] <= 1e-5 * scale[big]).all())


def test_runtime_grants_three_workgroups_per_cu_at_config_2(monkeypatch):
    """B = 512, N = 11, scales {2, 5, 11} on the f16x3 path: with the dynamic LDS the launchers really pass (the affinity
    tail's scene tile; ring + 2 032 bytes of stage), hipOccupancyMaxActiveBlocksPerMultiprocessor reports >= 3 workgroups
    per CU for the node stage and for the edge kernel, and a workgroup's LDS stays within a third of the CU's."""
    from groupnet_amd.multiscale import MultiScaleHGNN
    _setup("f16x3", monkeypatch)
    monkeypatch.delenv("GN_POOL_STAGE", raising=False)
    torch.manual_seed(45)
    B, N = 512, 11
    blk = MultiScaleHGNN([2, 5, 11]).to(dev()).eval()
    f = torch.randn(B, N, 64, device=dev())
    log = []
    _spy_launches(monkeypatch, log)
    with torch.no_grad():
        blk(f)
    print("\n" + "\n".join(f"{stem}: rc {rc}, dynamic LDS {lds} B, {occ} workgroups per CU" for stem, rc, lds, occ in log))
    stems = [e[0] for e in log]
    assert "gn_node_mlp_affinity" in stems and "gn_edge_mlp_gumbel" in stems, log
    for stem, rc, lds, occ in log:
        assert rc == 0 and occ >= 3, (stem, rc, lds, occ)
        if stem == "gn_edge_mlp_gumbel":
            assert lds == 38896 and lds + 256 <= CU_LDS // 3            # (+ the kernel's 256 B of static LDS)
        else:
            assert lds + 37120 <= CU_LDS // 3                           # (+ the node stage's static weight ring)
