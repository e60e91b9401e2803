"""Agents missing anywhere, the parts that need no GPU ("Agents missing anywhere"): the numpy statement of
the rule, what `ops.agent_subset` makes of a host mask, the two new entry points' place in the C ABI and their launch
plans, and the case table of tests/agent_subset_cases.py, whose seeds must keep every top-k selection of the compacted
scenes apart."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import agent_subset_cases as S
import ragged_cases as C
from test_capi_cpu import declared_structs, declared_symbols

P = ctypes.c_void_p


def test_the_rule_by_hand():
    n, order, slot, status = S.subset_rule([[0, 1, 1, 0, 1], [1, 1, 1, 1, 1], [0, 0, 0, 0, 9], [255, 0, 0, 0, 0]])
    assert n.tolist() == [3, 5, 1, 1] and status == 0
    assert order.tolist() == [[1, 2, 4, -1, -1], [0, 1, 2, 3, 4], [4, -1, -1, -1, -1], [0, -1, -1, -1, -1]]
    assert slot.tolist() == [[-1, 0, 1, -1, 2], [0, 1, 2, 3, 4], [-1, -1, -1, -1, 0], [0, -1, -1, -1, -1]]
    assert all(a.dtype == np.int32 for a in (n, order, slot))
    n, order, slot, status = S.subset_rule(np.zeros((2, 3), dtype=np.uint8))
    assert n.tolist() == [0, 0] and status == S.EMPTY and (order == -1).all() and (slot == -1).all()
    # stable: valid agents keep their relative order, and slot inverts order on the valid ranks
    v = np.random.default_rng(0).random((5, 70)) < 0.5
    n, order, slot, _ = S.subset_rule(v)
    for b in range(5):
        o = order[b, :n[b]]
        assert (np.diff(o) > 0).all() and v[b, o].all() and (slot[b, o] == np.arange(n[b])).all()
        assert (order[b, n[b]:] == -1).all() and (slot[b][~v[b]] == -1).all()


def test_the_torch_moves_are_each_others_inverse_on_valid_positions():
    case = S.BY_ID["n7"]
    mask = case["mask"]
    h, U = S.inputs(case)
    hc = S.compact_nodes(h, mask)
    for b, n in enumerate(case["counts"]):
        assert torch.equal(hc[b, :n], h[b, mask[b] != 0]) and not hc[b, n:].any()
    back = S.expand_nodes(hc, mask)
    assert torch.equal(back[mask != 0], h[mask != 0]) and not back[mask == 0].any()
    u = U[0][0]
    uc = S.compact_pairs(u, mask)
    N = case["N"]
    V = torch.nonzero(mask[1]).reshape(-1).tolist()
    for r, i in enumerate(V):
        for c, j in enumerate(V):
            assert torch.equal(uc[1, r * N + c], u[1, i * N + j])
    assert torch.equal(S.expand_pairs(uc, mask)[1, V[0] * N + V[-1]], u[1, V[0] * N + V[-1]])
    assert not S.expand_pairs(uc, mask)[1, 0].any()                  # slot 0 of scene 1 is invalid


def test_agent_subset_of_a_host_mask_has_three_return_kinds():
    from groupnet_amd import agent_subset, ops
    assert agent_subset is ops.agent_subset
    assert ops.agent_subset(torch.ones(3, 5, dtype=torch.bool)) is None
    assert ops.agent_subset(np.ones((3, 5), dtype=np.uint8)) is None
    pre = ops.agent_subset([[1, 1, 0, 0], [1, 1, 1, 1], [1, 0, 0, 0]])
    assert type(pre) is ops.AgentCounts and pre.counts == (2, 4, 1) and pre.N == 4 and pre._dev is None
    sub = ops.agent_subset(torch.tensor([[0, 1, 1, 0], [1, 1, 1, 1], [0, 0, 0, 9]], dtype=torch.uint8))
    assert isinstance(sub, ops.AgentSubset) and isinstance(sub, ops.AgentCounts)
    assert (sub.counts, sub.B, sub.N, sub.admits_empty) == ((2, 4, 1), 3, 4, False)
    assert sub._dev is None and sub._order is None and sub._slot is None            # nothing uploaded or launched yet
    assert sub._host.tolist() == [[0, 1, 1, 0], [1, 1, 1, 1], [0, 0, 0, 1]]
    plain = sub.compacted
    assert isinstance(plain, ops.AgentCounts) and not isinstance(plain, ops.AgentSubset)
    assert (plain.counts, plain.B, plain.N, plain.admits_empty) == ((2, 4, 1), 3, 4, False)
    assert ops.agent_counts(sub, 3, 4, "cuda") is sub                                # passes through as the counts it is
    with pytest.raises(ValueError):
        ops.agent_counts(sub, 3, 5, "cuda")
    assert isinstance(ops.agent_subset(np.array([[True, False, True]])), ops.AgentSubset)
    assert isinstance(ops.agent_subset([[True, False, True], [True, True, True]]), ops.AgentSubset)


@pytest.mark.parametrize("bad", [
    [[1, 0, 1], [0, 0, 0]],                                    # an empty scene
    [1, 0, 1],                                                 # 1-D
    torch.ones(2, 3, 4, dtype=torch.bool),                     # 3-D
    torch.ones(0, 3, dtype=torch.bool),                        # no scene
    torch.ones(2, 3),                                          # a float mask
    torch.ones(2, 3, dtype=torch.int64),                       # an integer tensor that is no byte mask
    np.ones((2, 3), dtype=np.float32),
    "mask",
], ids=["empty-scene", "1-d", "3-d", "no-scene", "float", "int64", "numpy-float", "str"])
def test_agent_subset_refuses(bad):
    from groupnet_amd import ops
    with pytest.raises(ValueError):
        ops.agent_subset(bad)


def test_agent_subset_wants_a_gpu_for_a_mask_with_holes():
    from groupnet_amd import ops
    with pytest.raises(ValueError):
        ops.agent_subset([[0, 1, 1]], device="cpu")


def test_abi_is_still_40_and_the_new_symbols_are_there():
    from groupnet_amd import _lib
    lib = _lib.load()
    assert lib.gn_abi_version() == 40 == _lib.ABI_VERSION
    names = declared_symbols()
    for n in ("gn_agent_subset_u8", "gn_agent_subset_plan", "gn_remap_rows", "gn_remap_rows_plan"):
        assert n in names and hasattr(lib, n) and n in _lib.SIGNATURES, n
    # the new ids have a range of their own: the forward launchers' table ends where the suite pins it
    assert (_lib.K_AGENT_SUBSET, _lib.K_REMAP_ROWS, _lib.K_LAST) == (40, 41, 31)
    assert lib.gn_kernel_name(_lib.K_AGENT_SUBSET) == b"agent_subset_kernel"
    assert lib.gn_kernel_name(_lib.K_REMAP_ROWS) == b"remap_rows_kernel"
    assert lib.gn_kernel_name(_lib.K_ZERO_PADDING) == b"zero_padding_kernel"         # the ids before keep their kernels
    assert all(lib.gn_kernel_name(k) is None for k in list(range(32, 40)) + [42, -1])


def test_remap_item_mirrors_the_header():
    from groupnet_amd import _lib
    fields = ["src", "dst", "src_scene", "dst_scene", "src_pitch", "dst_pitch", "width", "kind"]
    assert declared_structs()["gn_remap_item_t"] == fields == [n for n, _ in _lib.RemapItem._fields_]
    assert [getattr(_lib.RemapItem, n).offset for n in fields] == [0, 8, 16, 24, 32, 40, 48, 52]
    assert ctypes.sizeof(_lib.RemapItem) == 56
    assert (_lib.REMAP_NODE_ROWS, _lib.REMAP_PAIR_ROWS) == (0, 1)


def _subset_plan(valid=64, B=9, N=11, n_valid=64, order=64, slot=64, status=64):
    from groupnet_amd import _lib
    plan = _lib.LaunchPlan()
    rc = _lib.load().gn_agent_subset_plan(P(valid), B, N, P(n_valid), P(order), P(slot), P(status), ctypes.byref(plan))
    return rc, plan


def test_subset_plan_without_a_device():
    from groupnet_amd import _lib
    for B, grid in ((1, 1), (4, 1), (5, 2), (9, 3), (512, 128)):
        for N in (1, 64, 65, 200):
            rc, plan = _subset_plan(B=B, N=N)
            assert rc == 0 and plan.kernel == _lib.K_AGENT_SUBSET
            assert list(plan.grid) == [grid, 1, 1] and plan.dyn_lds == 0 and plan.n_groups == 0
    assert _subset_plan(valid=3)[0] == 0                                        # the mask bytes: any alignment
    for kw in (dict(valid=0), dict(n_valid=0), dict(order=0), dict(slot=0), dict(status=0)):
        assert _subset_plan(**kw)[0] == _lib.GN_ERR_NULL, kw
    for kw in (dict(n_valid=66), dict(order=66), dict(slot=66), dict(status=66)):
        assert _subset_plan(**kw)[0] == _lib.GN_ERR_ALIGN, kw
    for kw in (dict(B=0), dict(N=0), dict(N=-1)):
        assert _subset_plan(**kw)[0] == _lib.GN_ERR_SHAPE, kw
    assert _lib.load().gn_agent_subset_plan(P(64), 1, 1, P(64), P(64), P(64), P(64), None) == _lib.GN_ERR_NULL


def _item(N, rows_kind, width, es=4, src_pitch=None, dst_pitch=None, src_scene=None, dst_scene=None, src=4096, dst=1 << 20):
    """A descriptor of an (B,R,width elements) item at made-up addresses; pitches and scene strides in elements."""
    from groupnet_amd import _lib
    R = N * N if rows_kind == _lib.REMAP_PAIR_ROWS else N
    sp = width if src_pitch is None else src_pitch
    dp = width if dst_pitch is None else dst_pitch
    ss = R * sp if src_scene is None else src_scene
    ds = R * dp if dst_scene is None else dst_scene
    return _lib.RemapItem(src=src, dst=dst, src_scene=ss * es, dst_scene=ds * es, src_pitch=sp * es, dst_pitch=dp * es,
                          width=width * es, kind=rows_kind)


def _remap_plan(items, B=5, N=11, map_=64):
    from groupnet_amd import _lib
    plan = _lib.LaunchPlan()
    arr = (_lib.RemapItem * max(1, len(items)))(*items)
    rc = _lib.load().gn_remap_rows_plan(arr, len(items), B, N, P(map_), ctypes.byref(plan))
    return rc, plan


@pytest.mark.parametrize("N", [1, 11, 50, 65])
def test_remap_plan_picks_the_store_unit_of_every_item_shape(N):
    from groupnet_amd import _lib
    NODE, PAIR = _lib.REMAP_NODE_ROWS, _lib.REMAP_PAIR_ROWS
    wide = (1 + 2 * N) * N                      # scene stride of a (B, 1 + 2N, N) tensor
    items = [
        (_item(N, NODE, 64), 16),                                                     # fp32 feature rows, 256 bytes
        (_item(N, NODE, 64, src_pitch=320, src=4096 + 256), 16),                      # ... a column slice of (B,N,320)
        (_item(N, NODE, 64, es=2), 16),                                               # bf16 feature rows, 128 bytes
        (_item(N, NODE, 9, es=2), 2),                                                 # 18-byte bf16 factor rows
        (_item(N, NODE, 10), 8),                                                      # 40-byte fp32 factor rows
        (_item(N, PAIR, 6), 8),                                                       # 24-byte fp32 pair rows
        (_item(N, PAIR, 1), 4),                                                       # an (B,N,N) fp32 matrix
        (_item(N, PAIR, 1, es=2), 2),                                                 # ... in bf16
        (_item(N, PAIR, 1, dst_scene=wide, dst=(1 << 20) + 4 * N), 4),                # ... into a row block of (B,1+2N,N)
        (_item(N, NODE, 1, dst_scene=wide), 4),                                       # the (B,N,1) view of its first row
    ]
    rc, plan = _remap_plan([it for it, _ in items], N=N)
    assert rc == 0 and plan.kernel == _lib.K_REMAP_ROWS
    assert plan.n_groups == len(items) and list(plan.stage)[:len(items)] == [u for _, u in items]
    assert plan.stage_bytes == 2 and plan.grid[1] == len(items) and plan.grid[2] == 1
    most = max(5 * (N * N if it.kind == PAIR else N) * (it.width // u) for it, u in items)
    assert plan.grid[0] == min(max(1, -(-most // 512)), 4096)
    # a misaligned address lowers the unit of that item alone
    rc, plan = _remap_plan([_item(N, NODE, 64, src=4096 + 8), _item(N, NODE, 64, dst=(1 << 20) + 4), _item(N, NODE, 64)], N=N)
    assert rc == 0 and list(plan.stage)[:3] == [8, 4, 16] and plan.stage_bytes == 4


def test_remap_plan_refusals_without_a_device():
    from groupnet_amd import _lib
    ok = _item(11, _lib.REMAP_NODE_ROWS, 64)
    assert _remap_plan([ok] * 24)[0] == 0
    rc, plan = _remap_plan([ok] * 24)
    assert plan.n_groups == _lib.MAX_GROUPS and plan.grid[1] == 24
    assert _remap_plan([ok] * 25)[0] == _lib.GN_ERR_SHAPE
    assert _remap_plan([])[0] == _lib.GN_ERR_SHAPE
    for kw in (dict(N=0), dict(N=-3), dict(B=0), dict(N=32768)):
        assert _remap_plan([ok], **kw)[0] == _lib.GN_ERR_SHAPE, kw
    assert _remap_plan([ok], map_=0)[0] == _lib.GN_ERR_NULL
    assert _remap_plan([ok], map_=66)[0] == _lib.GN_ERR_ALIGN
    assert _remap_plan([_item(11, 0, 64, src=0)])[0] == _lib.GN_ERR_NULL
    assert _remap_plan([_item(11, 0, 64, dst=0)])[0] == _lib.GN_ERR_NULL
    assert _remap_plan([_item(11, 0, 64, src=4097)])[0] == _lib.GN_ERR_ALIGN
    assert _remap_plan([_item(11, 0, 9, es=1)])[0] == _lib.GN_ERR_ALIGN               # an odd width
    assert _remap_plan([_item(11, 2, 64)])[0] == _lib.GN_ERR_SHAPE                    # no such kind
    assert _remap_plan([_item(11, 0, 64, dst_pitch=32)])[0] == _lib.GN_ERR_SHAPE      # rows would overlap
    assert _remap_plan([_item(11, 0, 0)])[0] == _lib.GN_ERR_SHAPE
    assert _lib.load().gn_remap_rows_plan(None, 1, 5, 11, P(64), ctypes.byref(_lib.LaunchPlan())) == _lib.GN_ERR_NULL
    assert _lib.load().gn_remap_rows_plan((_lib.RemapItem * 1)(ok), 1, 5, 11, P(64), None) == _lib.GN_ERR_NULL


@pytest.mark.parametrize("case", S.CASES, ids=[c["id"] for c in S.CASES])
def test_case_table(case):
    """Every table holds an all-valid scene, a scene whose slot 0 is invalid and slot N - 1 valid, and a single-agent
    scene (the issue's cases; "n113h" is an addition); on the compacted scenes every top-k selection is MIN_GAP apart."""
    mask, N = case["mask"], case["N"]
    assert mask.shape == (case["B"], N) and mask.dtype == torch.uint8
    assert case["counts"] == S.subset_rule(mask.numpy())[0].tolist() and min(case["counts"]) >= 1
    assert any(bool(r.all()) for r in mask)
    assert any(r[0] == 0 and r[N - 1] != 0 for r in mask)
    if case["id"] != "n113h":
        assert 1 in case["counts"]
    ref = next(c for c in C.CASES if c["N"] == N)
    assert (case["scales"], case["B"]) == (ref["scales"], ref["B"])
    hc, Uc = S.compacted_inputs(case)
    gap = C.min_gap(case, hc)
    print(f"\n{case['id']}: counts {case['counts']}, smallest selection gap {gap:.2e}")
    assert gap >= C.MIN_GAP
    assert [tuple(u[0].shape) for u in Uc] == C.noise_shapes(case)
    from groupnet_amd import ops
    assert isinstance(ops.agent_subset(mask), ops.AgentSubset)


def test_signatures_keep_n_agents_last_and_gain_no_keyword():
    from groupnet_amd import graphs, multiscale, sharding
    from groupnet_amd.MS_HGNN_batch import MS_HGNN_hyper, MS_HGNN_oridinary
    for fn in (MS_HGNN_oridinary.forward, MS_HGNN_hyper.forward, multiscale.MultiScaleHGNN.forward, sharding.sharded_forward):
        assert list(inspect.signature(fn).parameters)[-1] == "n_agents", fn
    init = inspect.signature(graphs.GraphedMultiScale.__init__).parameters
    assert list(init)[-1] == "ragged" and init["ragged"].default is False
    assert list(inspect.signature(graphs.GraphedMultiScale.__call__).parameters) == ["self", "f", "n_agents", "agent_mask"]
