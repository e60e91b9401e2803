"""Agents missing anywhere, on the device ("Agents missing anywhere"): the subset kernel against the numpy
rule, the remap kernel against torch indexing, the three forwards against the existing ragged route on the compacted
batch (bit for bit: both sides run the same kernels on the same data) and against the per-scene CPU oracle, the route
selection of `ops.agent_subset`, the captured graph, training, and the refusals.

Gates.  Kernels and forwards against the route: exact, as bits.  Oracle: the gates of tests/test_ragged_gpu.py —
incidences bit for bit, features and factors within `ragged_cases.TOL`.  Training: the gates of
tests/test_ragged_backward_gpu.py — TOL_ANY on any batch, TOL_CLEAN on the scenes relu_probe calls clean, forward values
within 1e-5."""
import pytest
import torch

import agent_subset_cases as S
import ragged_backward_cases as RB
import ragged_cases as C
from test_backward_gpu import TOL_ANY, TOL_CLEAN, _check, _modules
from test_ragged_graph_gpu import SEED, device_noise

pytestmark = pytest.mark.gpu

IDS = [c["id"] for c in S.CASES]


def dev():
    return torch.device("cuda:0")


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# the subset kernel
# ---------------------------------------------------------------------------------------------------------------------
def _mask_rows(N, seed):
    """18 rows (two launches of B = 9): the shapes a row can take, valid bytes 1, 9 and 255."""
    gen = torch.Generator().manual_seed(seed)
    z = lambda: torch.zeros(N, dtype=torch.uint8)
    rows = []
    r = z(); r[:] = 1; rows.append(r)                                           # all valid
    rows.append(z())                                                            # none valid
    r = z(); r[0] = 1; rows.append(r)                                           # only slot 0
    r = z(); r[N - 1] = 255; rows.append(r)                                     # only slot N - 1
    r = z(); r[0::2] = 1; rows.append(r)                                        # alternating from 0
    r = z(); r[1::2] = 9; rows.append(r)                                        # alternating from 1
    r = z(); r[63:65] = 1; rows.append(r)                                       # valid only at 63 and 64 (where N has them)
    r = z(); r[:] = 1; r[min(64, N - 1)] = 0; rows.append(r)                    # a hole exactly at 64
    rows.append((torch.rand(N, generator=gen) < 0.5).to(torch.uint8))           # random, p = 0.5
    rows.append((torch.rand(N, generator=gen) < 0.9).to(torch.uint8) * 255)     # random, p = 0.9
    r = z(); r[:(N + 1) // 2] = 1; rows.append(r)                               # a prefix
    while len(rows) < 18:                                                       # further random rows: no empty one
        r = (torch.rand(N, generator=gen) < 0.7).to(torch.uint8) * 9
        r[int(torch.randint(0, N, (1,), generator=gen))] = 1
        rows.append(r)
    return torch.stack(rows)


def _run_subset(valid):
    """gn_agent_subset_u8 into the middle of guarded buffers -> (n_valid, order, slot, status, guards kept)."""
    from groupnet_amd import _lib
    B, N = valid.shape
    G = 0x5A5A5A5A
    nv = torch.full((B + 2,), G, dtype=torch.int32, device=dev())
    order = torch.full((B + 2, N), G, dtype=torch.int32, device=dev())
    slot = torch.full((B + 2, N), G, dtype=torch.int32, device=dev())
    status = torch.zeros(3, dtype=torch.int32, device=dev())
    status[0] = status[2] = G
    v = valid.to(dev())
    rc = _lib.load().gn_agent_subset_u8(_lib.addr(v), B, N, _lib.addr(nv[1:]), _lib.addr(order[1:]), _lib.addr(slot[1:]),
                                        _lib.addr(status[1:]), _lib.stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    kept = all(bool((t[0] == G).all()) and bool((t[-1] == G).all()) for t in (nv, order, slot, status))
    return nv[1:-1].cpu().numpy(), order[1:-1].cpu().numpy(), slot[1:-1].cpu().numpy(), int(status[1]), kept


@pytest.mark.parametrize("as_bool", [False, True], ids=["uint8", "bool"])
@pytest.mark.parametrize("N", [1, 7, 11, 63, 64, 65, 128, 129, 200])
def test_subset_kernel_equals_the_rule(N, as_bool):
    rows = _mask_rows(N, N)
    for part in (rows[:9], rows[9:]):                 # B = 9: the last workgroup is partial
        want_n, want_o, want_s, want_st = S.subset_rule(part.numpy())
        n, o, s, st, kept = _run_subset((part != 0) if as_bool else part)
        assert (n == want_n).all() and (o == want_o).all() and (s == want_s).all()
        assert st == want_st and kept
    assert S.subset_rule(rows[:9].numpy())[3] == S.EMPTY                # (the first launch holds the empty row)


def test_subset_kernel_status_is_empty_where_and_only_where_a_row_is_empty():
    from groupnet_amd import _lib
    for N in (1, 65):
        for r in _mask_rows(N, N)[:11]:
            n, _, _, st, kept = _run_subset(r[None])
            assert st == (_lib.COUNTS_EMPTY if not r.any() else 0) and st != _lib.COUNTS_NOT_PREFIX and kept
            assert n.tolist() == [int((r != 0).sum())]


def test_subset_holders():
    from groupnet_amd import _lib, ops
    case = S.BY_ID["n17"]
    mask = case["mask"]
    want_n, want_o, want_s, _ = S.subset_rule(mask.numpy())
    sub = ops.agent_subset(mask, device=dev())
    assert sub._dev is None
    assert (sub.dev.cpu().numpy() == want_n).all() and (sub.order.cpu().numpy() == want_o).all()
    assert (sub.slot.cpu().numpy() == want_s).all() and int(sub.status.item()) == 0
    assert sub.compacted.dev is sub.dev
    gsub = ops.agent_subset(mask.to(dev()).bool())
    assert gsub.admits_empty and (gsub.order.cpu().numpy() == want_o).all() and (gsub.B, gsub.N) == tuple(mask.shape)
    with pytest.raises(RuntimeError):
        gsub.counts
    st = ops.StaticAgentSubset(case["B"], case["N"], dev())
    ptrs = (st.dev.data_ptr(), st.order.data_ptr(), st.slot.data_ptr())
    ar = torch.arange(case["N"], dtype=torch.int32).expand(case["B"], -1)
    assert torch.equal(st.order.cpu(), ar) and torch.equal(st.slot.cpu(), ar) and st.dev.tolist() == [case["N"]] * case["B"]
    st.set_from_mask(mask.to(dev()))
    assert (st.dev.cpu().numpy() == want_n).all() and (st.order.cpu().numpy() == want_o).all()
    assert (st.slot.cpu().numpy() == want_s).all()
    counts = [0, 17, 3, 1, 9]
    st.set(counts)
    pn, po, ps, _ = S.subset_rule(ar.numpy() < torch.tensor(counts).numpy()[:, None])
    assert (st.dev.cpu().numpy() == pn).all() and (st.order.cpu().numpy() == po).all() and (st.slot.cpu().numpy() == ps).all()
    assert ptrs == (st.dev.data_ptr(), st.order.data_ptr(), st.slot.data_ptr())
    assert int(st.status.item()) == 0                                 # `set` reports nothing; the mask entry does
    empty = mask.clone()
    empty[2] = 0
    st.set_from_mask(empty.to(dev()))
    assert int(st.status.item()) == _lib.COUNTS_EMPTY
    for bad in (mask, mask.to(dev()).float(), mask.to(dev())[:, :5], mask.to(dev()).t()):
        with pytest.raises(ValueError):
            st.set_from_mask(bad)


# ---------------------------------------------------------------------------------------------------------------------
# the remap kernel
# ---------------------------------------------------------------------------------------------------------------------
def _item_shapes(B, N):
    """(name, base shape, dtype, the view of the base that is the item, kind, which torch reference)."""
    from groupnet_amd import ops
    f32, b16 = torch.float32, torch.bfloat16
    full = lambda t: t
    NODE, PAIR = ops.REMAP_NODE_ROWS, ops.REMAP_PAIR_ROWS
    return [
        ("fp32 w64", (B, N, 64), f32, full, NODE, "nodes"),
        ("fp32 w64, column slice of (B,N,320)", (B, N, 320), f32, lambda t: t[..., 64:128], NODE, "nodes"),
        ("bf16 w64", (B, N, 64), b16, full, NODE, "nodes"),
        ("bf16 w9", (B, N, 9), b16, full, NODE, "nodes"),
        ("fp32 w10", (B, N, 10), f32, full, NODE, "nodes"),
        ("fp32 pair rows w6", (B, N * N, 6), f32, full, PAIR, "pairs"),
        ("fp32 matrix", (B, N, N), f32, full, PAIR, "matrix"),
        ("bf16 matrix", (B, N, N), b16, full, PAIR, "matrix"),
        ("fp32 matrix, row block of (B,1+2N,N)", (B, 1 + 2 * N, N), f32, lambda t: t[:, 1:1 + N], PAIR, "matrix"),
        ("bf16 matrix, row block of (B,1+2N,N)", (B, 1 + 2 * N, N), b16, lambda t: t[:, 1 + N:1 + 2 * N], PAIR, "matrix"),
        ("(B,N,1) view of the first row of (B,1+2N,N)", (B, 1 + 2 * N, N), f32, lambda t: t[:, 0, :].unsqueeze(-1), NODE,
         "nodes"),
    ]


_FWD = {"nodes": S.compact_nodes, "pairs": S.compact_pairs, "matrix": S.compact_matrix}
_BACK = {"nodes": S.expand_nodes, "pairs": S.expand_pairs, "matrix": S.expand_matrix}


def _remap_mask(B, N, seed):
    gen = torch.Generator().manual_seed(seed)
    mask = (torch.rand(B, N, generator=gen) < 0.6).to(torch.uint8)
    mask[0] = 1                     # an all-valid scene, an empty one, one with a single agent in the last slot
    mask[1] = 0
    mask[2] = 0
    mask[2, N - 1] = 1
    return mask


@pytest.mark.parametrize("expand", [False, True], ids=["order", "slot"])
@pytest.mark.parametrize("N", [1, 11, 50, 65])
def test_remap_kernel_equals_torch_indexing(N, expand):
    from groupnet_amd import ops
    B = 5
    mask = _remap_mask(B, N, 40 + N)
    _, order, slot, _ = S.subset_rule(mask.numpy())
    map_ = torch.from_numpy(slot if expand else order).to(dev())
    move, undo = (_BACK, _FWD) if expand else (_FWD, _BACK)
    gen = torch.Generator().manual_seed(N)
    shapes = _item_shapes(B, N)
    items, checks = [], []
    for k in range(24):                                 # 24 items in one launch: the table is full
        name, shape, dt, take, kind, ref = shapes[k % len(shapes)]
        src_base = torch.randn(shape, generator=gen).to(dt)
        dst_base = torch.randn(shape, generator=gen).to(dt)
        src_view = take(src_base)
        mapped = undo[ref](move[ref](torch.ones_like(src_view), mask), mask) != 0      # the source positions a row is read from
        src_view[~mapped] = float("nan")
        want_base = dst_base.clone()
        want = move[ref](src_view.clone(), mask)
        assert not torch.isnan(want).any()
        take(want_base).copy_(want)
        take(dst_base).fill_(float("nan"))
        sd, dd = src_base.to(dev()), dst_base.to(dev())
        items.append((take(sd), take(dd), kind))
        checks.append((f"{name} #{k}", dd, want_base, take, mapped))
    ops.remap_rows(items, map_)
    torch.cuda.synchronize()
    for name, dd, want_base, take, mapped in checks:
        got = dd.cpu()
        assert not torch.isnan(take(got)).any(), name
        assert same(got, want_base), name               # the item, zeros at unmapped positions, and the bytes around a slice


@pytest.mark.parametrize("N", [1, 11, 50, 65])
def test_remap_round_trip(N):
    from groupnet_amd import ops
    B = 5
    mask = _remap_mask(B, N, 60 + N)
    sub = ops.agent_subset(mask.to(dev()))
    gen = torch.Generator().manual_seed(N)
    x = torch.randn(B, N, 64, generator=gen)
    p = torch.randn(B, N * N, 6, generator=gen).bfloat16()
    m = torch.randn(B, N, N, generator=gen)
    src = [t.to(dev()) for t in (x, p, m)]
    mid = [torch.full_like(t, float("nan")) for t in src]
    out = [torch.full_like(t, float("nan")) for t in src]
    kinds = [ops.REMAP_NODE_ROWS, ops.REMAP_PAIR_ROWS, ops.REMAP_PAIR_ROWS]
    ops.remap_rows(list(zip(src, mid, kinds)), sub.order)
    ops.remap_rows(list(zip(mid, out, kinds)), sub.slot)
    valid = mask != 0
    pair_ok = (valid[:, :, None] & valid[:, None, :])
    assert same(out[0], torch.where(valid[..., None], x, torch.zeros_like(x)))
    assert same(out[1], torch.where(pair_ok.reshape(B, N * N, 1), p, torch.zeros_like(p)))
    assert same(out[2], torch.where(pair_ok, m, torch.zeros_like(m)))
    assert int(sub.status.item()) == S.EMPTY


def test_remap_rows_refuses_what_it_cannot_move():
    from groupnet_amd import ops
    B, N = 3, 5
    map_ = torch.zeros(B, N, dtype=torch.int32, device=dev())
    x = torch.zeros(B, N, 8, device=dev())
    for src, dst, kind, m in ((x, x.clone().half(), 0, map_), (x, torch.zeros(B, N, 4, device=dev()), 0, map_),
                              (x, x.clone(), 1, map_), (x.cpu(), x.clone(), 0, map_), (x, x.clone(), 0, map_.long()),
                              (x.transpose(1, 2), x.transpose(1, 2).clone(), 0, map_), (x, x.clone(), 7, map_)):
        with pytest.raises(ValueError):
            ops.remap_rows([(src, dst, kind)], m)


# ---------------------------------------------------------------------------------------------------------------------
# the forwards against the existing route on the compacted batch
# ---------------------------------------------------------------------------------------------------------------------
def _to(case, t):
    t = t.to(dev())
    return t.bfloat16() if case["storage"] == "bf16" and t.dtype == torch.float32 and t.shape[-1] == 64 else t


def _noise_dev(U):
    return [[u.to(dev()) for u in us] for us in U]


def _block_pair(case, nmp=1, grouped=True, tail=True):
    """(subset forward on clean inputs, the same with NaN in every invalid input row, the expected results: the ragged
    route on the compacted batch, expanded by torch indexing)."""
    from groupnet_amd import ops
    mask = case["mask"]
    blk = C.cpu_block(case, nmp)[0].to(dev()).eval()
    blk.grouped, blk.affinity_tail = grouped, tail
    h, U = S.inputs(case, nmp)
    hc, Uc = S.compact_nodes(h, mask), S.compact_noise(U, mask)
    with torch.no_grad():
        outc, Hc = blk(_to(case, hc), noise_u=_noise_dev(Uc), n_agents=case["counts"])
        want = (S.expand_nodes(outc.cpu(), mask), S.expand_new_H(Hc.cpu(), mask, case["scales"]))
        sub = ops.agent_subset(mask, device=dev())
        assert isinstance(sub, ops.AgentSubset)
        clean = blk(_to(case, h), noise_u=_noise_dev(U), n_agents=sub)
        dirty = blk(_to(case, S.with_nan(case, h)), noise_u=_noise_dev(S.nan_noise(case, U)), n_agents=sub)
    return clean, dirty, want


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_block_equals_the_ragged_route_on_the_compacted_batch(case):
    clean, dirty, want = _block_pair(case)
    for got in (clean, dirty):
        assert same(got[0], want[0]) and same(got[1], want[1])
    mask = case["mask"]
    h = _to(case, S.inputs(case)[0]).cpu()
    assert same(clean[0][..., :64].cpu(), torch.where(mask[..., None] != 0, h, torch.zeros_like(h)))   # f at valid rows, zeros
    assert not clean[0].cpu()[mask == 0].any()


@pytest.mark.parametrize("nmp,grouped,tail", [(2, True, True), (1, True, False), (1, False, True)],
                         ids=["nmp2", "own-launch", "ungrouped"])
def test_block_forms_at_n7(nmp, grouped, tail):
    clean, dirty, want = _block_pair(S.BY_ID["n7"], nmp, grouped, tail)
    for got in (clean, dirty):
        assert same(got[0], want[0]) and same(got[1], want[1])


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_modules_equal_the_ragged_route_on_the_compacted_batch(case):
    from groupnet_amd import ops
    from oracle import ms_hgnn_oracle as O
    mask, N, B = case["mask"], case["N"], case["B"]
    blk = C.cpu_block(case)[0].to(dev()).eval()
    h, U = S.inputs(case)
    hc, Uc = S.compact_nodes(h, mask), S.compact_noise(U, mask)
    hn, Un = S.with_nan(case, h), S.nan_noise(case, U)
    corr = O.affinity(h)                                    # a caller's corr, NaN wherever an end is invalid
    corrc = S.compact_matrix(corr, mask)
    corrn = torch.where(S.expand_matrix(S.compact_matrix(torch.ones_like(corr), mask), mask) != 0, corr,
                        torch.full_like(corr, float("nan")))
    sub = ops.agent_subset(mask, device=dev())
    with torch.no_grad():
        nfc, facc = blk.interaction(_to(case, hc), noise_u=Uc[0][0].to(dev()), n_agents=case["counts"])
        want = (S.expand_nodes(nfc.cpu(), mask), S.expand_pairs(facc.cpu(), mask))
        wide = torch.full((B, N, 192), 3.0, device=dev(), dtype=nfc.dtype)
        for x, u, out in ((h, U, None), (hn, Un, wide[..., 64:128])):
            nf, fac = blk.interaction(_to(case, x), noise_u=u[0][0].to(dev()), out=out, n_agents=sub)
            assert same(nf, want[0]) and same(fac, want[1])
        assert bool((wide[..., :64] == 3).all()) and bool((wide[..., 128:] == 3).all())      # out=: a column block
        for i, (s, mod) in enumerate(zip(case["scales"], blk.interaction_hyper)):
            nfc, facc, Hc = mod(_to(case, hc), corrc.to(dev()), noise_u=Uc[1 + i][0].to(dev()), n_agents=case["counts"])
            want = (S.expand_nodes(nfc.cpu(), mask), S.expand_edges(facc.cpu(), mask), S.expand_incidence(Hc.cpu(), mask))
            for x, c, u in ((h, corr, U), (hn, corrn, Un)):
                got = mod(_to(case, x), c.to(dev()), noise_u=u[1 + i][0].to(dev()), n_agents=sub)
                assert all(same(g, w) for g, w in zip(got, want)), f"scale {s}"
            if s == N:                                      # the single row holds exactly V_b
                assert torch.equal(want[2][:, 0].float(), (mask != 0).float())


def test_default_host_draws_are_read_at_original_indices():
    """Without noise_u the host-mode draws keep the padded shapes in the original layout, module-major as the block
    draws them: the call equals the one that is handed those draws."""
    from groupnet_amd import ops
    case = S.BY_ID["n7"]
    blk = C.cpu_block(case)[0].to(dev()).eval()
    h, _ = S.inputs(case)
    sub = ops.agent_subset(case["mask"], device=dev())
    with torch.no_grad():
        torch.manual_seed(99)
        a = blk(h.to(dev()), n_agents=sub)
        torch.manual_seed(99)
        U = [[torch.rand(shp)] for shp in blk.noise_shapes(case["B"], case["N"])]
        b = blk(h.to(dev()), noise_u=_noise_dev(U), n_agents=sub)
    assert same(a[0], b[0]) and same(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------
# against the per-scene oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["n7", "n17"])
def test_block_and_modules_against_the_per_scene_oracle(case_id):
    """Per scene, the CPU oracle on h[b, V_b] with the noise taken at the original indices (`compact_noise` gathers it
    there by torch indexing)."""
    from groupnet_amd import ops
    case = S.BY_ID[case_id]
    mask, N, scales = case["mask"], case["N"], case["scales"]
    blk, sp, shs = C.cpu_block(case)
    blk = blk.to(dev()).eval()
    h, U = S.inputs(case)
    hc, Uc = S.compact_nodes(h, mask), S.compact_noise(U, mask)
    assert C.min_gap(case, hc) >= C.MIN_GAP
    sub = ops.agent_subset(mask, device=dev())
    corr = S.expand_matrix(C.padded_corr(case, hc), mask)            # each scene's own affinity at its original slots
    x, nd = S.with_nan(case, h).to(dev()), _noise_dev(S.nan_noise(case, U))
    with torch.no_grad():
        out, new_H = blk(x, noise_u=nd, n_agents=sub)
        facs = [blk.interaction(x, noise_u=nd[0], n_agents=sub)[1].cpu()]
        Hs = []
        for i, mod in enumerate(blk.interaction_hyper):
            _, fac, H = mod(x, corr.to(dev()), noise_u=nd[1 + i], n_agents=sub)
            facs.append(fac.cpu())
            Hs.append(H.cpu())
    out, bad = out.cpu(), []
    assert torch.equal(new_H.cpu(), torch.cat(Hs, dim=1))
    worst_f = worst_c = 0.0
    for b, n in enumerate(case["counts"]):
        V = torch.nonzero(mask[b]).reshape(-1)
        feats, rfacs, rHs = C.scene_oracle(sp, shs, case, hc, Uc, b)
        for i in range(1 + len(scales)):
            worst_f = max(worst_f, float((out[b, V, 64 * (1 + i):64 * (2 + i)].double() - feats[i]).abs().max()))
            f = facs[i][b]
            if i == 0:
                rows = (V[:, None] * N + V[None, :]).reshape(-1)
            else:
                rows = V if f.shape[0] == N and scales[i - 1] != N else torch.arange(1)
                Hb = Hs[i - 1][b]
                got = Hb[:, V] if Hb.shape[0] == 1 and N != 1 else Hb[V][:, V]
                if not torch.equal(got, rHs[i - 1][0]):
                    bad.append(f"scene {b} scale {scales[i - 1]}: incidence differs from the oracle")
            worst_c = max(worst_c, float((f[rows].double() - rfacs[i]).abs().max()))
            pad = torch.ones(f.shape[0], dtype=torch.bool)
            pad[rows] = False
            if f[pad].any():
                bad.append(f"scene {b} module {i}: factors at invalid positions are not zero")
    print(f"\n{case_id}: features {worst_f:.1e}, factors {worst_c:.1e} (gate {C.TOL:g})")
    assert not bad, "\n".join(bad)
    assert worst_f <= C.TOL and worst_c <= C.TOL


# ---------------------------------------------------------------------------------------------------------------------
# route selection
# ---------------------------------------------------------------------------------------------------------------------
def test_route_selection():
    from groupnet_amd import _lib, ops
    case = S.BY_ID["n7"]
    B, N, mask = case["B"], case["N"], case["mask"]
    blk = C.cpu_block(case)[0].to(dev()).eval()
    h, U = S.inputs(case)
    x, nd = h.to(dev()), _noise_dev(U)
    counts = [7, 3, 1, 4, 3, 6]
    prefix = (torch.arange(N)[None] < torch.tensor(counts)[:, None])
    with torch.no_grad():
        a = blk(x, noise_u=nd, n_agents=ops.agent_subset(prefix, device=dev()))
        b = blk(x, noise_u=nd, n_agents=counts)
        assert same(a[0], b[0]) and same(a[1], b[1])                   # a prefix everywhere: the n_agents= call
        a = blk(x, noise_u=nd, n_agents=ops.agent_subset(torch.ones(B, N, dtype=torch.bool)))
        b = blk(x, noise_u=nd)
        assert same(a[0], b[0]) and same(a[1], b[1])                   # everything valid: the full batch
        # a GPU mask with an empty scene: zeros there, the other scenes keep their bits
        full = blk(x, noise_u=nd, n_agents=ops.agent_subset(mask, device=dev()))
        holed = mask.clone()
        holed[3] = 0
        gsub = ops.agent_subset(holed.to(dev()))
        got = blk(x, noise_u=nd, n_agents=gsub)
        nf, fac = blk.interaction(x, noise_u=nd[0], n_agents=gsub)
        hy = [m(x, torch.zeros(B, N, N, device=dev()), noise_u=u, n_agents=gsub) for m, u in zip(blk.interaction_hyper, nd[1:])]
    keep = [b for b in range(B) if b != 3]
    for g, f in zip(got, full):
        assert not g[3].any() and same(g[keep], f[keep])
    assert not nf[3].any() and not fac[3].any()
    for r in hy:
        assert all(not t[3].any() for t in r)                           # the single factor row of the scale-N module too
    assert int(gsub.status.item()) == _lib.COUNTS_EMPTY


# ---------------------------------------------------------------------------------------------------------------------
# the captured graph
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["n7", "n50"])
def test_subset_replay_equals_eager_bit_for_bit(case_id):
    from groupnet_amd import _lib, ops
    from groupnet_amd.graphs import GraphedMultiScale
    case = S.BY_ID[case_id]
    B, N, mask, bf16 = case["B"], case["N"], case["mask"], case["storage"] == "bf16"
    blk = C.cpu_block(case)[0].to(dev()).eval()
    h = S.inputs(case)[0]
    g = GraphedMultiScale(blk, B, N, seed=SEED, dtype=torch.bfloat16 if bf16 else torch.float32, ragged="subset")
    assert isinstance(g.counts, ops.StaticAgentSubset)
    assert g.draws_per_step == sum(b * e * k for b, e, k in C.noise_shapes(case))
    ptrs = (g.counts.dev.data_ptr(), g.counts.order.data_ptr(), g.counts.slot.data_ptr())
    empty = mask.clone()
    empty[1] = 0
    counts = [max(0, N - 2 * b - (N if b == 2 else 0)) for b in range(B)]            # prefix counts, one empty slot
    prefix = (torch.arange(N)[None] < torch.tensor(counts)[:, None]).to(torch.uint8)
    replays = [("holes", dict(agent_mask=mask.to(dev())), mask), ("all valid", dict(agent_mask=torch.ones_like(mask).to(dev()).bool()), torch.ones_like(mask)),
               ("an empty slot", dict(agent_mask=empty.to(dev())), empty), ("n_agents=", dict(n_agents=counts), prefix),
               ("the previous values stay", {}, prefix)]
    seen = 0
    for k, (what, kw, m) in enumerate(replays):
        xk = _to(case, S.with_nan(dict(case, mask=m), h))               # NaN in every row this replay's mask leaves out
        out, H = [t.clone() for t in g(xk, **kw)]
        with device_noise(blk, k * g.draws_per_step):
            e_out, e_H = blk(xk, n_agents=ops.agent_subset(m.to(dev())))
        assert same(out, e_out) and same(H, e_H), what
        assert int(g.counter.item()) == k * g.draws_per_step
        seen |= _lib.COUNTS_EMPTY if what == "an empty slot" else 0
        assert g.status() == seen                                       # only ever COUNTS_EMPTY, and only from a mask
    assert ptrs == (g.counts.dev.data_ptr(), g.counts.order.data_ptr(), g.counts.slot.data_ptr())
    with pytest.raises(ValueError):
        g(agent_mask=mask)                                              # a CPU mask
    with pytest.raises(ValueError):
        g(agent_mask=mask.to(dev()), n_agents=counts)
    with pytest.raises(ValueError):
        GraphedMultiScale(blk, B, N, ragged="holes")


# ---------------------------------------------------------------------------------------------------------------------
# training
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def opted_in():
    import groupnet_amd as G
    G.set_ragged_training(True)
    try:
        yield
    finally:
        G.set_ragged_training(None)


def _rows_case(case, rows):
    mask = case["mask"][rows]
    return dict(case, mask=mask, counts=[int(v) for v in mask.sum(dim=1)], B=len(rows))


def _module_run(tag, module, state0, pairwise, scale, case, h, U_mod, R1, R2, rows, tol):
    """Scenes `rows` of the case as a batch of their own: the per-scene float64 oracle on h[b, V_b] (built as
    `ragged_backward_cases` builds it, on the compacted batch) against the subset route under autograd."""
    from groupnet_amd import ops
    sub = _rows_case(case, rows)
    mask, N = sub["mask"], sub["N"]
    hs, Us = h[rows].contiguous(), [u[rows].contiguous() for u in U_mod]
    R1s, R2s = R1[rows].contiguous(), R2[rows].contiguous()
    cp, ex = (S.compact_pairs, S.expand_pairs) if pairwise else (S.compact_edges, S.expand_edges)
    ref = RB.module_oracle(state0, pairwise, scale, sub, S.compact_nodes(hs, mask), [cp(u, mask) for u in Us],
                           S.compact_nodes(R1s, mask), cp(R2s, mask))
    for p in module.parameters():
        p.grad = None
    x = S.with_nan(sub, hs).to(dev()).requires_grad_(True)
    nz = [u.to(dev()) for u in Us]
    n_agents = ops.agent_subset(mask, device=dev())
    if pairwise:
        nf, fac = module(x, noise_u=nz, n_agents=n_agents)
    else:
        module.scale = scale
        corr = S.expand_matrix(C.padded_corr(sub, S.compact_nodes(hs, mask)), mask).to(dev())
        nf, fac, H = module(x, corr, noise_u=nz, n_agents=n_agents)
        assert torch.equal(H.cpu(), S.expand_incidence(C.padded_incidence(sub, S.compact_nodes(hs, mask), scale), mask))
    want_nf, want_fac = S.expand_nodes(ref["node_feat"], mask), ex(ref["factors"], mask)
    e_nf = float((nf.detach().double().cpu() - want_nf).abs().max())
    e_fac = float((fac.detach().double().cpu() - want_fac).abs().max())
    assert e_nf <= 1e-5 and e_fac <= 1e-5, (tag, e_nf, e_fac)
    assert not bool(nf.detach().cpu()[mask == 0].any()) and not bool(fac.detach().cpu()[want_fac == 0].any())
    g1, g2 = R1s.to(dev()), R2s.to(dev())                     # non-zero at invalid positions too: the backward drops them
    torch.autograd.backward([nf, fac], [g1, g2])
    assert same(g1, R1s) and same(g2, R2s)                    # the caller's gradient tensors are not written
    gx = x.grad.cpu()
    assert torch.equal(gx[mask == 0], torch.zeros_like(gx[mask == 0])), (tag, "invalid rows of dL/dh")
    g_h = S.expand_nodes(ref["g_h"], mask)
    eh = float((gx.double() - g_h).abs().max()) / float(g_h.abs().max())
    assert eh <= tol, (tag, "dL/dh", eh, tol)
    used = [k for k, v in ref["grads"].items() if v is not None and float(v.abs().max()) > 0]
    ew, where = _check({k: p.grad for k, p in module.named_parameters()}, ref["grads"], used, tol)
    return ref["clean"], eh, ew, where


@pytest.mark.parametrize("kind,scale", [("pair", None), ("hyper", 2), ("hyper", 7)], ids=["pairwise", "scale2", "scaleN"])
def test_module_gradients_at_n7(kind, scale, opted_in):
    case = S.BY_ID["n7"]
    B, N, pairwise = case["B"], case["N"], kind == "pair"
    h, U = S.inputs(case)
    pair, hyper = _modules(300 + N)
    module = pair if pairwise else hyper
    state0 = {k: v.detach().clone() for k, v in module.state_dict().items()}
    module.to(dev()).train()
    g = torch.Generator().manual_seed(5)
    E = N * N if pairwise else (1 if scale == N else N)
    R1, R2 = torch.randn(B, N, 64, generator=g), torch.randn(B, E, module.edge_types, generator=g)
    U_mod = U[0] if pairwise else U[1 + case["scales"].index(scale)]
    tag = f"subset {kind} N={N} scale={scale}"
    args = (module, state0, pairwise, scale, case, h, U_mod, R1, R2)
    clean, eh, ew, where = _module_run(tag, *args, list(range(B)), TOL_ANY)
    msg = f"\n{tag}: whole batch dL/dh {eh:.1e}, worst parameter {ew:.1e} ({where}); {int(clean.sum())}/{B} scenes clean"
    if bool(clean.all()):
        assert eh <= TOL_CLEAN and ew <= TOL_CLEAN, (tag, eh, ew, where)
    elif bool(clean.any()):
        rows = [b for b in range(B) if bool(clean[b])]
        _, eh2, ew2, where2 = _module_run(tag + " clean scenes", *args, rows, TOL_CLEAN)
        msg += f"; clean scenes {rows} alone dL/dh {eh2:.1e}, worst parameter {ew2:.1e} ({where2})"
    print(msg)


def _block_run(case_id, rows, tol):
    """Scenes `rows` of the case as a batch of their own, the block under autograd against the per-scene oracle."""
    from groupnet_amd import ops
    full = S.BY_ID[case_id]
    case = _rows_case(full, rows)
    B, N, mask, scales = case["B"], case["N"], case["mask"], case["scales"]
    blk, sp, shs = C.cpu_block(case)
    h, U = S.inputs(full)
    h, U = h[rows].contiguous(), [[u[rows].contiguous() for u in us] for us in U]
    hc, Uc = S.compact_nodes(h, mask), S.compact_noise(U, mask)
    n_mod = 1 + len(scales)
    g = torch.Generator().manual_seed(6)
    Rm = torch.randn(full["B"], N, 64 * n_mod, generator=g)[rows].contiguous()     # module columns of `final`, invalid rows too
    Rc = S.compact_nodes(Rm, mask)
    refs = []
    for i, (state, s) in enumerate(zip([sp, *shs], [None, *scales])):
        E = N * N if s is None else (1 if s == N else N)
        K = C.K_PAIR if s is None else C.K_HYPER
        refs.append(RB.module_oracle(state, s is None, s, case, hc, Uc[i], Rc[..., 64 * i:64 * (i + 1)], torch.zeros(B, E, K)))
    g_f = S.expand_nodes(sum(r["g_h"] for r in refs), mask)
    clean = torch.stack([r["clean"] for r in refs]).all(dim=0)
    blk.to(dev()).train()
    x = S.with_nan(case, h).to(dev()).requires_grad_(True)
    n_agents = ops.agent_subset(mask, device=dev())
    final, new_H = blk(x, noise_u=_noise_dev(S.nan_noise(case, U)), n_agents=n_agents)
    want = S.expand_nodes(torch.cat([r["node_feat"] for r in refs], dim=-1), mask)
    assert float((final[..., 64:].detach().double().cpu() - want).abs().max()) <= 1e-5
    if isinstance(n_agents, ops.AgentSubset):       # (clean scenes alone may all be prefixes: the n_agents= route, f copied)
        assert same(final[..., :64].detach(), torch.where(mask[..., None] != 0, h, torch.zeros_like(h)))
    gR = Rm.to(dev())
    final[..., 64:].backward(gR)
    assert same(gR, Rm)                                           # the caller's gradient tensor is not written
    gx = x.grad.cpu()
    assert torch.equal(gx[mask == 0], torch.zeros_like(gx[mask == 0]))
    eh = float((gx.double() - g_f).abs().max()) / float(g_f.abs().max())
    assert eh <= tol, ("dL/df", eh, tol)
    worst = []
    for prefix, r in zip(["interaction."] + [f"interaction_hyper.{i}." for i in range(len(scales))], refs):
        used = [k for k, v in r["grads"].items() if v is not None and float(v.abs().max()) > 0]
        hip = {k[len(prefix):]: p.grad for k, p in blk.named_parameters() if k.startswith(prefix)}
        worst.append(_check(hip, r["grads"], used, tol))
    with torch.no_grad():
        _, H_inf = blk.eval()(x.detach(), noise_u=_noise_dev(U), n_agents=ops.agent_subset(mask, device=dev()))
    assert torch.equal(new_H, H_inf)
    return clean, eh, max(w for w, _ in worst)


@pytest.mark.parametrize("case_id", ["n7", "n17"])
def test_block_gradients(case_id, opted_in):
    B = S.BY_ID[case_id]["B"]
    clean, eh, ew = _block_run(case_id, list(range(B)), TOL_ANY)
    msg = f"\nsubset block {case_id}: dL/df {eh:.1e}, worst parameter {ew:.1e}; {int(clean.sum())}/{B} scenes clean"
    if bool(clean.all()):
        assert eh <= TOL_CLEAN and ew <= TOL_CLEAN, (case_id, eh, ew)
    elif bool(clean.any()):
        rows = [b for b in range(B) if bool(clean[b])]
        _, eh2, ew2 = _block_run(case_id, rows, TOL_CLEAN)
        msg += f"; clean scenes {rows} alone dL/df {eh2:.1e}, worst parameter {ew2:.1e}"
    print(msg)


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(monkeypatch, opted_in):
    import groupnet_amd as G
    from groupnet_amd import ops, sharding
    from groupnet_amd.graphs import GraphedMultiScale
    case = S.BY_ID["n7"]
    B, N, mask = case["B"], case["N"], case["mask"]
    blk = C.cpu_block(case)[0].to(dev())
    x = S.inputs(case)[0].to(dev())
    corr = torch.zeros(B, N, N, device=dev())
    pair, hyper = blk.interaction, blk.interaction_hyper[0]
    with torch.no_grad():                   # weight images are packed once, outside the count
        blk.eval()(x, n_agents=ops.agent_subset(mask, device=dev()))
    g = GraphedMultiScale(blk, B, N, ragged="subset")
    gsub = ops.agent_subset(mask.to(dev()))                             # (built on the device: launched here)
    torch.cuda.synchronize()
    launches = []
    real = ops.stream_handle
    monkeypatch.setattr(ops, "stream_handle", lambda: launches.append(1) or real())
    sub = ops.agent_subset(mask, device=dev())
    blk.train()
    for call in (lambda: blk(x, n_agents=gsub), lambda: pair(x, n_agents=gsub), lambda: hyper(x, corr, n_agents=gsub)):
        with pytest.raises(NotImplementedError):         # a GPU-built subset admits empty scenes: inference only
            call()
    G.set_ragged_training(False)
    with pytest.raises(NotImplementedError):             # ... and without the opt-in every subset is
        blk(x, n_agents=sub)
    G.set_ragged_training(True)
    blk.eval()
    with torch.no_grad():
        with pytest.raises(ValueError):
            hyper(x, corr, H=torch.zeros(B, N, N, device=dev()), n_agents=sub)
        with pytest.raises(ValueError):
            hyper(x, corr, masks=ops.IncidenceMasks(torch.zeros(B, N, dtype=torch.int64, device=dev()),
                                                    torch.zeros(B, N, dtype=torch.int64, device=dev())), n_agents=sub)
        hyper.listall = True
        try:
            with pytest.raises(NotImplementedError):
                hyper(x, corr, n_agents=sub)
            with pytest.raises(NotImplementedError):
                blk(x, n_agents=sub)
        finally:
            hyper.listall = False
        for call in (lambda s: blk(x, n_agents=s), lambda s: pair(x, n_agents=s), lambda s: hyper(x, corr, n_agents=s)):
            with pytest.raises(ValueError):              # a subset of other sizes
                call(ops.agent_subset(mask[:-1], device=dev()))
            with pytest.raises(ValueError):
                call(ops.agent_subset(torch.cat([mask, mask], dim=1), device=dev()))
        big = G.MS_HGNN_hyper(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=1,
                              scale=N + 1).to(dev()).eval()
        with pytest.raises(RuntimeError):
            big(x, corr, n_agents=sub)
        with pytest.raises(ValueError):                  # (before the process group is asked)
            sharding.sharded_forward(blk, x, n_agents=sub)
        with pytest.raises(ValueError):
            g(agent_mask=mask)                           # a CPU mask
    assert not launches
    assert sub._dev is None and sub._order is None       # ... and nothing was uploaded
