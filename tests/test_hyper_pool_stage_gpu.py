"""Fused node->edge pooling of the hyper modules (N <= 16, ops.POOL_MAX_N = 16) inside the edge kernels: the LDS-staged
two-phase form (pq rows, then x' rows through one buffer) and the batched global-memory form (groups whose scenes do not
fit a stage, e.g. scale == N: one hyperedge per scene) against the per-member reference form (GN_POOL_STAGE=0), bit for
bit; the fused inference forward against the node2edge launch; and which forwards still issue that launch."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


# (B, N, scales): ragged last workgroups, s = 1 (one member per row), s = N (E = 1), N = 3 / 11 / 16, and batches large
# enough that a 128-row (256-row: two row blocks per wave) workgroup spans the most scenes a stage holds
CASES = [(7, 11, [1, 2, 5, 11]), (29, 3, [1, 2, 3]), (13, 16, [1, 4, 16]), (300, 11, [2, 5, 11]), (150, 16, [3, 16])]
MODES = ["f16x3", "bf16x6", "bf16-rb1", "bf16-rb2"]


def _setup(mode, monkeypatch):
    from groupnet_amd import ops
    monkeypatch.setattr(ops, "BF16X6", ops.BF16X6)
    monkeypatch.setattr(ops, "F16X3", ops.F16X3)
    if mode in ("f16x3", "bf16x6"):
        ops.set_precision(mode)
        return torch.float32
    monkeypatch.setenv("GN_EDGE_RB2", "1" if mode == "bf16-rb2" else "0")
    return torch.bfloat16


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B,N,scales", CASES)
def test_staged_hyper_pooling_is_bit_identical(B, N, scales, mode, monkeypatch):
    from groupnet_amd import ops
    from groupnet_amd.multiscale import MultiScaleHGNN
    monkeypatch.setattr(ops, "POOL_MAX_N", ops.POOL_KERNEL_MAX_N)     # every hyper module here pools in the edge kernel
    dtype = _setup(mode, monkeypatch)
    torch.manual_seed(31)
    blk = MultiScaleHGNN(scales).to(dev()).eval()
    f = torch.randn(B, N, 64, device=dev()).to(dtype)
    U = [[torch.rand(s, device=dev())] for s in blk.noise_shapes(B, N)]
    outs = {}
    with torch.no_grad():
        for st in ("0", "1"):
            monkeypatch.setenv("GN_POOL_STAGE", st)
            outs[st] = blk(f, noise_u=U)
    for a, b in zip(outs["0"], outs["1"]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,N,scales", [(7, 11, [1, 2, 5, 11]), (300, 11, [2, 5, 11]), (13, 16, [1, 4, 16])])
def test_fused_hyper_pooling_equals_the_node2edge_launch(B, N, scales, monkeypatch):
    """Within 1e-6 of the output scale (the fused pooling sums the 32 attention channels in two halves), incidence
    identical."""
    from groupnet_amd import ops
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(23)
    blk = MultiScaleHGNN(scales).to(dev()).eval()
    f = torch.randn(B, N, 64, device=dev())
    U = [[torch.rand(s, device=dev())] for s in blk.noise_shapes(B, N)]
    with torch.no_grad():
        monkeypatch.setattr(ops, "POOL_MAX_N", ops.POOL_KERNEL_MAX_N)
        fused = blk(f, noise_u=U)
        monkeypatch.setattr(ops, "POOL_MAX_N", 0)
        ref = blk(f, noise_u=U)
    err = float((fused[0] - ref[0]).abs().max()) / float(ref[0].abs().max())
    print(f"\nhyper pooling in the edge kernel vs node2edge launch: max rel diff {err:.2e}")
    assert err <= 1e-6 and torch.equal(fused[1], ref[1])


def test_inference_forward_issues_no_node2edge_launch_but_training_does(monkeypatch):
    from groupnet_amd import ops
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(5)
    B, N, scales = 6, 11, [2, 5, 11]
    blk = MultiScaleHGNN(scales).to(dev())
    f = torch.randn(B, N, 64, device=dev())
    U = [[torch.rand(s, device=dev())] for s in blk.noise_shapes(B, N)]
    real = ops.node2edge_grouped
    monkeypatch.setattr(ops, "POOL_MAX_N", ops.POOL_KERNEL_MAX_N)

    def refuse(items):
        raise AssertionError("node2edge launch in an inference forward at N <= POOL_MAX_N")

    monkeypatch.setattr(ops, "node2edge_grouped", refuse)
    blk.eval()
    with torch.no_grad():
        blk(f, noise_u=U)
    calls = []

    def count(items):
        calls.append(len(items))
        return real(items)

    monkeypatch.setattr(ops, "node2edge_grouped", count)
    blk.train()
    out, _ = blk(f, noise_u=U)
    out.sum().backward()
    assert calls, "a training forward keeps the node2edge launch (its backward reads `edges`)"
