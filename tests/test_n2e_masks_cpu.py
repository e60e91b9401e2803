"""The node -> edge launch reading member words (gn_node2edge_masks_*; ABI 37, additive), host side only — no kernel is
launched: the four symbols exist and nothing else of the ABI moved, the plan with words equals the dense plan in every
field but `variant` (2 where the dense one says 1, 0 where it says 0), the all-NULL words array is exactly the old entry
point, and every refusal of the header's table comes back before a launch from both the plan and the launch entry points.
The two refusals of the Python face need device tensors (`ops` has no CPU path) and carry the gpu mark."""
import ctypes

import pytest
import torch

P = ctypes.c_void_p
OK, ERR_NULL, ERR_SHAPE, ERR_ALIGN = 0, -1, -2, -4
NAMES = ["gn_node2edge_masks_f32", "gn_node2edge_masks_bf16", "gn_node2edge_masks_plan_f32", "gn_node2edge_masks_plan_bf16"]
# (B, N, Es): small and banded by the launch-size rule; config 4 (E >= 24: rows); the full word; several scenes per
# workgroup with a ragged last one; many rows (hyper_rows >= 49152: rows at E = 24 either way)
CASES = [(2, 17, (17, 17, 1)), (6, 50, (50,) * 4), (2, 64, (64, 1)), (683, 17, (17, 17, 1)), (4096, 24, (24,))]


def _lib():
    from groupnet_amd import _lib as L
    return L, L.load()


def _hyper(E, **kw):
    return dict(dict(xp=16, pq=16, H=16, w2=16, edges=16, b2=16, E=E), **kw)


def _pair(N):
    return dict(xp=16, pq=16, w2=16, edges=16, b2=16, E=N * (N + 1) // 2, sym=1)


def _arr(groups):
    L, _ = _lib()
    return (L.N2EGroup * len(groups))(*[L.N2EGroup(**g) for g in groups])


def _words(ws):
    return (P * len(ws))(*ws)


def _dense_plan(groups, B, N, twin):
    L, lib = _lib()
    plan = L.LaunchPlan()
    rc = (lib.gn_node2edge_plan_bf16 if twin else lib.gn_node2edge_plan_f32)(_arr(groups), len(groups), B, N, ctypes.byref(plan))
    return rc, plan


def _masks_plan(groups, words, B, N, twin):
    L, lib = _lib()
    plan = L.LaunchPlan()
    fn = lib.gn_node2edge_masks_plan_bf16 if twin else lib.gn_node2edge_masks_plan_f32
    rc = fn(_arr(groups), None if words is None else _words(words), len(groups), B, N, ctypes.byref(plan))
    return rc, plan


def _masks_launch(groups, words, B, N, twin):
    _, lib = _lib()
    fn = lib.gn_node2edge_masks_bf16 if twin else lib.gn_node2edge_masks_f32
    return fn(_arr(groups), None if words is None else _words(words), len(groups), B, N, P(0))


def _fields(plan):
    """Every field of a plan as plain Python values."""
    out = {}
    for name, _ in plan._fields_:
        v = getattr(plan, name)
        out[name] = v if isinstance(v, int) else list(v)
    return out


def test_symbols_are_there_and_nothing_else_moved():
    L, lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name) and name in L.SIGNATURES, name
    assert lib.gn_abi_version() == L.ABI_VERSION >= 37
    names = [lib.gn_kernel_name(k) for k in range(1, L.K_LAST + 1)]
    assert names.count(b"node2edge_kernel") == 1 and lib.gn_kernel_name(L.K_LAST + 1) is None      # no kernel id of its own: the variant says it
    assert lib.gn_kernel_name(14) == b"node2edge_kernel"
    assert L.N2EGroup._fields_[-1][0] == "sym"                          # the descriptor got no trailing field


@pytest.mark.parametrize("rows", [None, "0", "1"], ids=["unset", "rows0", "rows1"])
@pytest.mark.parametrize("twin", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B,N,Es", CASES, ids=[f"B{B}-N{N}" for B, N, _ in CASES])
def test_plan_with_words_is_the_dense_plan_but_for_the_variant(B, N, Es, twin, rows, monkeypatch):
    if rows is None:
        monkeypatch.delenv("GN_N2E_ROWS", raising=False)
    else:
        monkeypatch.setenv("GN_N2E_ROWS", rows)                         # read per call
    hyper = [_hyper(E) for E in Es]
    for groups, words in ((hyper, [32] * len(Es)), (hyper + [_pair(N)], [32] * len(Es) + [None]),
                          ([_pair(N)] + hyper, [None] + [40] * len(Es))):
        rc_d, dense = _dense_plan(groups, B, N, twin)
        rc_m, masks = _masks_plan(groups, words, B, N, twin)
        assert rc_d == OK and rc_m == OK
        d, m = _fields(dense), _fields(masks)
        assert d["variant"] in (0, 1) and m["variant"] == (2 if d["variant"] == 1 else 0), (d["variant"], m["variant"])
        assert {k: v for k, v in m.items() if k != "variant"} == {k: v for k, v in d.items() if k != "variant"}
        assert m["kernel"] == 14 and m["precision"] == int(twin)        # GN_K_NODE2EDGE
        if m["variant"]:                                                # what tests/launch_forms.py reads as the row form
            assert m["EBh"] == 0
        # the switch's two ends, and the launch-size rule of the middle
        if rows == "0":
            assert m["variant"] == 0
        elif rows == "1" or max(Es) >= 24 or B * sum(Es) >= 49152:
            assert m["variant"] == 2
        else:
            assert m["variant"] == 0
        # all-NULL words: the old entry point, field for field
        rc_0, none = _masks_plan(groups, [None] * len(groups), B, N, twin)
        assert rc_0 == OK and _fields(none) == d


@pytest.mark.parametrize("twin", [False, True], ids=["f32", "bf16"])
def test_every_refusal_comes_before_a_launch(twin, monkeypatch):
    """The header's table, through the plan and the launch entry points; the stream is NULL and no GPU is needed because
    nothing is launched."""
    monkeypatch.delenv("GN_N2E_ROWS", raising=False)
    N = 17
    h, p = _hyper(N), _pair(N)
    table = [
        ([h], None, 2, N, ERR_NULL),                                   # rowmasks == NULL
        ([h, p], [32, 32], 2, N, ERR_SHAPE),                           # a word on a pairwise group
        ([_hyper(65)], [32], 2, 65, ERR_SHAPE),                        # a word holds 64 members
        ([_hyper(1)], [32], 2, 65, ERR_SHAPE),
        ([h, _hyper(1)], [32, None], 2, N, ERR_SHAPE),                 # one form per launch
        ([h, p, _hyper(1)], [None, None, 32], 2, N, ERR_SHAPE),
        ([h], [36], 2, N, ERR_ALIGN),                                  # a word pointer is 8-byte aligned
        ([h, h], [32, 44], 2, N, ERR_ALIGN),
    ]
    for groups, words, B, n, want in table:
        assert _masks_plan(groups, words, B, n, twin)[0] == want, (words, n)
        assert _masks_launch(groups, words, B, n, twin) == want, (words, n)
    # the forms beside the table that are fine: N = 64 with words, 8-byte (not 16-byte) aligned words, N > 64 without words
    assert _masks_plan([_hyper(64)], [32], 2, 64, twin)[0] == OK
    assert _masks_plan([h], [40], 2, N, twin)[0] == OK
    assert _masks_plan([_hyper(65)], [None], 2, 65, twin)[0] == OK
    # and the checks every group met before: they still come first or alike
    assert _masks_plan([_hyper(N, xp=0)], [32], 2, N, twin)[0] == ERR_NULL
    assert _masks_plan([_hyper(N, edges=20)], [32], 2, N, twin)[0] == ERR_ALIGN
    L, lib = _lib()
    fn = lib.gn_node2edge_masks_plan_bf16 if twin else lib.gn_node2edge_masks_plan_f32
    assert fn(_arr([h]), _words([32]), 1, 2, N, None) == ERR_NULL       # no plan to fill


def test_masks_apply_is_unchanged(monkeypatch):
    from groupnet_amd import ops
    from groupnet_amd.MS_HGNN_batch import masks_apply
    monkeypatch.delenv("GN_INC_MASKS", raising=False)
    assert ops.incidence_form() == "dense" and not any(masks_apply(N) for N in (11, 17, 50, 64, 65))
    try:
        ops.set_incidence_form("mask")
        assert [masks_apply(N) for N in (1, 11, 16, 17, 33, 50, 64, 65, 70)] == [False, False, False, True, True, True, True,
                                                                                False, False]
    finally:
        ops.set_incidence_form(None)


@pytest.mark.gpu
def test_python_face_refuses_wrong_masks():
    """`ops.node2edge_grouped`: masks whose row words are not (B,E), and masks on a pairwise item.  (Device tensors: `ops`
    refuses CPU tensors before it looks at anything else.)"""
    from groupnet_amd import ops
    dev = torch.device("cuda:0")
    B, N = 2, 17
    xp, pq = torch.randn(B, N, 64, device=dev), torch.randn(B, N, 64, device=dev)
    w2, b2 = torch.randn(32, device=dev), torch.randn(1, device=dev)
    H = (torch.rand(B, N, N, device=dev) < 0.3).float()
    good = ops.incidence_masks(H)
    assert ops.node2edge_grouped([(xp, pq, H, w2, b2, False, good)])[0].shape == (B, N, 64)
    one = ops.incidence_masks(H[:, :1].contiguous())                    # (B,1) row words for an E = N group
    short = ops.incidence_masks(H[:1].contiguous())                     # (1,E)
    for bad in (one, short):
        with pytest.raises(ValueError, match="masks.row"):
            ops.node2edge_grouped([(xp, pq, H, w2, b2, False, bad)])
    with pytest.raises(ValueError, match="IncidenceMasks"):
        ops.node2edge_grouped([(xp, pq, H, w2, b2, False, good.row)])
    for sym in (False, True):
        with pytest.raises(ValueError, match="hyper group"):
            ops.node2edge_grouped([(xp, pq, None, w2, b2, sym, good)])
    with pytest.raises(ValueError, match="hyper group"):
        ops.node2edge(xp, pq, None, w2, b2, masks=good)
