"""Ragged batches from a captured graph ("Ragged batches") without a device: the plan queries of the
two ABI 40 launches, the host validation of the static holder of the counts, the mask -> counts rule that
tests/test_ragged_graph_gpu.py holds the kernel against, and the counts under sharding."""
import ctypes
import inspect
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import ragged_graph_cases as RG

P = 4096            # an aligned non-NULL "device address": a plan query tests addresses, it never reads through them


def lib():
    from groupnet_amd import _lib
    return _lib, _lib.load()


# ---------------------------------------------------------------------------------------------------------------------
# plan queries
# ---------------------------------------------------------------------------------------------------------------------
def test_abi_40_is_additive():
    L, lb = lib()
    assert lb.gn_abi_version() == L.ABI_VERSION == 40
    assert (L.COUNTS_NOT_PREFIX, L.COUNTS_EMPTY) == (RG.NOT_PREFIX, RG.EMPTY)
    assert L.K_LAST == L.K_ZERO_PADDING == 31 and lb.gn_kernel_name(L.K_LAST + 1) is None       # no kernel id was added


def test_agent_counts_plan():
    L, lb = lib()
    plan = L.LaunchPlan()
    q = lambda valid=P, B=5, N=65, out=P, status=P: lb.gn_agent_counts_plan_u8(valid, B, N, out, status, ctypes.byref(plan))
    assert q(valid=None) == L.GN_ERR_NULL and q(out=None) == L.GN_ERR_NULL and q(status=None) == L.GN_ERR_NULL
    assert lb.gn_agent_counts_plan_u8(P, 5, 65, P, P, None) == L.GN_ERR_NULL
    assert q(out=P + 2) == L.GN_ERR_ALIGN and q(status=P + 1) == L.GN_ERR_ALIGN
    assert q(valid=P + 3) == L.GN_OK                                     # the mask is read byte by byte
    for bad in (dict(B=0), dict(B=-1), dict(N=0), dict(N=-7)):
        assert q(**bad) == L.GN_ERR_SHAPE, bad
    for B, N in ((1, 1), (5, 65), (4, 64), (1025, 100000)):              # one wave per scene, four to a workgroup
        assert q(B=B, N=N) == L.GN_OK
        assert list(plan.grid) == [(B + 3) // 4, 1, 1] and plan.dyn_lds == 0 and plan.kernel == 0
    # errors launch nothing: the launcher answers them with a NULL stream and no device
    assert lb.gn_agent_counts_u8(None, 5, 65, P, P, None) == L.GN_ERR_NULL
    assert lb.gn_agent_counts_u8(P, 5, 0, P, P, None) == L.GN_ERR_SHAPE


def test_zero_empty_scenes_plan():
    L, lb = lib()
    B = 5
    it = (L.ZeroItem * 2)(L.ZeroItem(ptr=P, pitch=4 * 10, width=4 * 10), L.ZeroItem(ptr=P, pitch=2 * 9, width=2 * 9))
    plan = L.LaunchPlan()
    q = lambda n=2, counts=P, B=B: lb.gn_zero_empty_scenes_plan(it, n, B, counts, ctypes.byref(plan))
    assert q(counts=None) == L.GN_ERR_NULL and q(counts=P + 2) == L.GN_ERR_ALIGN
    assert lb.gn_zero_empty_scenes_plan(None, 2, B, P, ctypes.byref(plan)) == L.GN_ERR_NULL
    assert lb.gn_zero_empty_scenes_plan(it, 2, B, P, None) == L.GN_ERR_NULL
    assert q(n=0) == L.GN_ERR_SHAPE and q(n=L.MAX_ZERO_ITEMS + 1) == L.GN_ERR_SHAPE and q(B=0) == L.GN_ERR_SHAPE
    assert q() == L.GN_OK
    assert list(plan.grid) == [1, 2, 1] and plan.kernel == 0
    it[1].width = 9                                                  # rows are written as 4- or 2-byte words, never as bytes
    assert q() == L.GN_ERR_ALIGN
    it[1].width, it[1].pitch = 20, 16
    assert q() == L.GN_ERR_SHAPE
    it[1].pitch, it[1].ptr = 20, None
    assert q() == L.GN_ERR_NULL


# ---------------------------------------------------------------------------------------------------------------------
# the static holder's host validation
# ---------------------------------------------------------------------------------------------------------------------
def test_static_counts_admit_zero_to_n_and_nothing_else():
    from groupnet_amd import ops
    B, N = 3, 7
    for good in ([0, 7, 3], [0, 0, 0], [7, 7, 7], (1, 2, 3), torch.tensor([0, 7, 3]),
                 torch.tensor([0, 7, 3], dtype=torch.int32), torch.tensor([0, 7, 3], dtype=torch.uint8)):
        assert ops.count_values(good, B, N, lowest=0) == [int(v) for v in good]
    for bad in ([8, 7, 7], [7, 7, N + 1], [-1, 7, 7], [True, 7, 7], [False, 7, 7], [7.0, 7, 7], [7, 7], [7, 7, 7, 7], 5,
                torch.tensor([7.0, 7.0, 7.0]), torch.tensor([[0, 7, 3]]), torch.tensor([0, 7]), torch.tensor([0, 8, 3]),
                torch.tensor([True, False, True])):
        with pytest.raises(ValueError):
            ops.count_values(bad, B, N, lowest=0)
    # a GPU tensor is refused by its device alone, before anything is read (a stand-in that says is_cuda without a GPU)
    class OnGpu(torch.Tensor):
        is_cuda = True
    with pytest.raises(ValueError, match="GPU tensor"):
        ops.count_values(torch.tensor([0, 7, 3]).as_subclass(OnGpu), B, N, lowest=0)
    # the same function, as a call's n_agents= uses it, keeps refusing 0
    with pytest.raises(ValueError):
        ops.count_values([0, 7, 3], B, N)
    with pytest.raises(ValueError):
        ops.agent_counts([0, 7, 3], B, N, torch.device("cpu"))
    with pytest.raises(ValueError, match="GPU"):                       # the holder itself has no CPU form
        ops.StaticAgentCounts(B, N, "cpu")


def test_the_new_keywords_come_last():
    from groupnet_amd import sharding
    from groupnet_amd.graphs import GraphedMultiScale
    ps = list(inspect.signature(GraphedMultiScale.__init__).parameters.values())
    assert ps[-1].name == "ragged" and ps[-1].default is False
    assert [p.name for p in ps[1:9]] == ["block", "B", "N", "seed", "device", "warmup", "dtype", "affinity_tail"]
    ps = list(inspect.signature(GraphedMultiScale.__call__).parameters.values())
    assert [(p.name, p.default) for p in ps[1:]] == [("f", None), ("n_agents", None), ("agent_mask", None)]
    ps = list(inspect.signature(sharding.sharded_forward).parameters.values())
    assert ps[-1].name == "n_agents" and ps[-1].default is None


# ---------------------------------------------------------------------------------------------------------------------
# the mask rule
# ---------------------------------------------------------------------------------------------------------------------
def test_mask_rule_by_hand():
    counts, status = RG.mask_rule(np.array([[1, 1, 1, 1], [0, 0, 0, 0], [1, 9, 0, 0], [1, 0, 1, 0], [0, 0, 0, 1]]))
    assert counts.tolist() == [4, 0, 2, 1, 0] and status == RG.NOT_PREFIX | RG.EMPTY
    assert RG.mask_rule(np.array([[1, 1], [1, 0]]))[1] == 0
    assert RG.mask_rule(np.array([[1, 1], [0, 0]]))[1] == RG.EMPTY
    assert RG.mask_rule(np.array([[1, 0, 1]]))[1] == RG.NOT_PREFIX
    counts, status = RG.mask_rule(np.array([[0, 1, 1]], dtype=np.uint8))
    assert counts.tolist() == [0] and counts.dtype == np.int32 and status == RG.NOT_PREFIX | RG.EMPTY


@pytest.mark.parametrize("N", RG.MASK_NS)
def test_mask_rows_are_what_their_names_say(N):
    m = RG.mask_rows(N)
    counts, status = RG.mask_rule(m)
    prefix = max(N // 2, 1) if N > 1 else 0
    hole = N // 3 + 1 if N > 2 else 0
    assert counts.tolist() == [N, 0, prefix, hole, 1 if N == 1 else 0]
    assert 0 < prefix < N or N == 1
    assert status == (RG.EMPTY | (RG.NOT_PREFIX if N > 1 else 0))
    assert (RG.mask_rule(RG.prefix_mask(counts, N))[0] == counts).all()          # a prefix mask gives its counts back
    # the rule against a scan written out element by element
    for b in range(m.shape[0]):
        n = 0
        while n < N and m[b, n]:
            n += 1
        assert n == counts[b]


# ---------------------------------------------------------------------------------------------------------------------
# sharding
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class _Recorder:
    """A block that records what it was called with and returns its input as the features."""

    def __init__(self):
        self.calls = []

    def __call__(self, f_local, **kw):
        self.calls.append({k: (v.tolist() if isinstance(v, torch.Tensor) else v) for k, v in kw.items()})
        return torch.cat((f_local, 2.0 * f_local), dim=-1), None


def _shard_worker(rank, world, port, B, counts, out_dir):
    from groupnet_amd import sharding
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        f = torch.arange(B * 3 * 4, dtype=torch.float32).view(B, 3, 4)
        blk = _Recorder()
        out = [sharding.sharded_forward(blk, f, noise_full=[])[0],
               sharding.sharded_forward(blk, f, noise_full=[], n_agents=counts)[0],
               sharding.sharded_forward(blk, f, noise_full=[], n_agents=torch.tensor(counts))[0]]
        with pytest.raises(ValueError):
            sharding.sharded_forward(blk, f, noise_full=[], n_agents=counts[:-1])
        torch.save(dict(calls=blk.calls, out=out), os.path.join(out_dir, f"shard{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_every_rank_passes_its_slice_of_the_counts_on(tmp_path):
    from groupnet_amd import sharding
    world, B = 2, 5
    counts = [3, 1, 2, 3, 3]             # rank 0 owns scenes 0..2, rank 1 scenes 3..4: all N = 3 there
    mp.spawn(_shard_worker, args=(world, _free_port(), B, counts, str(tmp_path)), nprocs=world, join=True)
    f = torch.arange(B * 3 * 4, dtype=torch.float32).view(B, 3, 4)
    for r in range(world):
        d = torch.load(os.path.join(tmp_path, f"shard{r}.pt"))
        s, e = sharding.shard_range(B, r, world)
        assert len(d["calls"]) == 3                                      # the refused call never reached the block
        assert d["calls"][0] == dict(noise_u=[])                         # no keyword: the block is not handed counts
        assert d["calls"][1] == dict(noise_u=[], n_agents=counts[s:e])
        assert d["calls"][2] == dict(noise_u=[], n_agents=counts[s:e])
        for out in d["out"]:
            assert torch.equal(out, torch.cat((f, 2.0 * f), dim=-1))
