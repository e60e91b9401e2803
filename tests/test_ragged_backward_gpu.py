"""Training on ragged batches ("Ragged batches", Training): the count-aware node->edge backward and the
fourth zeroing kind alone through the C ABI, then whole modules and the block under autograd against the per-scene CPU
oracle (tests/ragged_backward_cases.py), then the plumbing of the opt-in.

Gates.  Kernels: `backward_kernel_refs.gate`, max(4 e32, 2^-22 scale), never above TOL_CLEAN of the scale.  Modules: the
gates of tests/test_backward_gpu.py — TOL_ANY (2e-3 of max|grad|) on any batch, TOL_CLEAN (2e-5) on the scenes without a
ReLU input inside the rounding window of zero (relu_probe, applied per scene); forward values within 1e-5."""
import pytest
import torch

import backward_kernel_refs as R
import ragged_backward_cases as RB
import ragged_cases as C
from test_backward_gpu import TOL_ANY, TOL_CLEAN, _check, _modules

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def opted_in():
    import groupnet_amd as G
    G.set_ragged_training(True)
    yield
    G.set_ragged_training(None)


def _api():
    from groupnet_amd import _lib
    return _lib, _lib.load(), dev()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 1. the count-aware pooling backward ----------------------------------------------------------------------------
def _buffers(case):
    d = {k: v.to(dev()) for k, v in RB.kernel_inputs(case).items()}
    out = {o: d[o + "0"].clone() for o in R.N2E_OUTPUTS}
    nv = torch.tensor(case.counts, dtype=torch.int32, device=dev())
    return d, out, nv


def _verdict(bad, case, d, out):
    for o in R.N2E_OUTPUTS:
        bound, e32, scale, ref = RB.kernel_gate(case, o, TOL_CLEAN)
        err = float((out[o].detach().double().cpu() - ref).abs().max())
        print(f"\nn2e_bwd_ragged {case.name} (N={case.N} counts={list(case.counts)} E={case.E} {case.kind}) {o}: measured "
              f"{err:.2e} / e32 {e32:.2e} / gate {bound:.2e} (scale {scale:.2e})", end="")
        if not err <= bound:        # (NaN fails)
            bad.append((case.name, o, err, e32, bound))
    for b, n in enumerate(case.counts):
        # padded node rows are neither read nor written; an empty slot and a scene without gradient keep every bit
        rows = slice(0, None) if n == 0 or b == case.zero_scene else slice(n, None)
        assert torch.equal(_bits(out["dxp"][b, rows]), _bits(d["dxp0"][b, rows])), (case.name, "dxp", b)
        assert torch.equal(_bits(out["dpq"][b, rows]), _bits(d["dpq0"][b, rows])), (case.name, "dpq", b)


@pytest.mark.parametrize("case", RB.KERNEL_CASES, ids=lambda c: c.name)
def test_node2edge_bwd_ragged(case):
    L, lib, _ = _api()
    d, out, nv = _buffers(case)
    H = d["H"] if case.kind in ("hyper", "one") else None
    with torch.cuda.device(dev()):
        L.check(lib.gn_node2edge_bwd_ragged_f32(L.addr(d["xp"]), L.addr(d["pq"]), L.addr(H), L.addr(d["w2"]),
                                                L.addr(d["b2"]), L.addr(d["dedges"]), L.addr(out["dxp"]),
                                                L.addr(out["dpq"]), L.addr(out["dw2"]), L.addr(out["db2"]), case.B, case.N,
                                                case.E, int(case.kind == "sym"), L.addr(nv), L.stream_handle()),
                "gn_node2edge_bwd_ragged_f32")
    torch.cuda.synchronize()
    bad = []
    _verdict(bad, case, d, out)
    assert not bad, bad


def test_node2edge_bwd_ragged_grouped():
    """sym pairwise, hyper E = N and hyper E = 1 in one launch over the counts [11, 4, 1]."""
    L, lib, _ = _api()
    bufs = [_buffers(c) for c in RB.GROUPED]
    groups = [L.N2EBwdGroup(xp=L.addr(d["xp"]), pq=L.addr(d["pq"]), H=L.addr(d["H"] if c.kind != "sym" else None),
                            w2=L.addr(d["w2"]), b2=L.addr(d["b2"]), dedges=L.addr(d["dedges"]), dxp=L.addr(o["dxp"]),
                            dpq=L.addr(o["dpq"]), dw2=L.addr(o["dw2"]), db2=L.addr(o["db2"]), E=c.E,
                            sym=int(c.kind == "sym")) for c, (d, o, _) in zip(RB.GROUPED, bufs)]
    arr = (L.N2EBwdGroup * len(groups))(*groups)
    with torch.cuda.device(dev()):
        L.check(lib.gn_node2edge_bwd_ragged_grouped_f32(arr, len(groups), 3, 11, L.addr(bufs[0][2]), L.stream_handle()),
                "gn_node2edge_bwd_ragged_grouped_f32")
    torch.cuda.synchronize()
    bad = []
    for c, (d, o, _) in zip(RB.GROUPED, bufs):
        _verdict(bad, c, d, o)
    assert not bad, bad


def test_node2edge_bwd_ragged_refuses_before_any_launch():
    """N = 141 (no per-wave ragged form), missing and misaligned counts: the error code, and no buffer is touched."""
    L, lib, _ = _api()
    N = RB.LDS_LIMIT_N + 1
    z = lambda *s: torch.randn(*s, device=dev())
    xp, pq, H, w2, b2, dedges = z(1, N, 64), z(1, N, 64), torch.ones(1, 1, N, device=dev()), z(32), z(1), z(1, 1, 64)
    outs = [z(1, N, 64), z(1, N, 64), z(32), z(1)]
    before = [o.clone() for o in outs]
    nv = torch.tensor([3, 0], dtype=torch.int32, device=dev())
    call = lambda n, counts: lib.gn_node2edge_bwd_ragged_f32(
        L.addr(xp), L.addr(pq), L.addr(H), L.addr(w2), L.addr(b2), L.addr(dedges), *[L.addr(o) for o in outs], 1, n, 1, 0,
        counts, L.stream_handle())
    grp = lambda n, counts: lib.gn_node2edge_bwd_ragged_grouped_f32(
        (L.N2EBwdGroup * 1)(L.N2EBwdGroup(xp=L.addr(xp), pq=L.addr(pq), H=L.addr(H), w2=L.addr(w2), b2=L.addr(b2),
                                          dedges=L.addr(dedges), dxp=L.addr(outs[0]), dpq=L.addr(outs[1]),
                                          dw2=L.addr(outs[2]), db2=L.addr(outs[3]), E=1, sym=0)), 1, 1, n, counts,
        L.stream_handle())
    with torch.cuda.device(dev()):
        for f in (call, grp):
            assert f(N, L.addr(nv)) == L.GN_ERR_LDS
            assert f(11, None) == L.GN_ERR_NULL
            assert f(11, L.addr(nv) + 2) == L.GN_ERR_ALIGN
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(outs, before))


# ---- 2. the fourth zeroing kind ------------------------------------------------------------------------------------
def test_zero_sym_pair_rows():
    from groupnet_amd import ops
    B, N, counts = 3, 5, [5, 2, 1]
    g = torch.Generator().manual_seed(4)
    t0 = torch.randn(B, 15, 64, generator=g)
    t = t0.to(dev())
    ops.zero_padding([(t, ops.ZERO_SYM_PAIR_ROWS)], ops.AgentCounts(tuple(counts), N, dev()))
    torch.cuda.synchronize()
    pairs = [(i, j) for i in range(N) for j in range(i, N)]
    seen = 0
    for b, n in enumerate(counts):
        for r, (i, j) in enumerate(pairs):
            if i >= n or j >= n:
                assert not bool(t[b, r].any()), (b, i, j)
                seen += 1
            else:
                assert torch.equal(_bits(t[b, r]), _bits(t0[b, r])), (b, i, j)
    assert seen == (15 - 3) + (15 - 1)
    with pytest.raises(ValueError):
        ops.zero_padding([(torch.zeros(B, 14, 64, device=dev()), ops.ZERO_SYM_PAIR_ROWS)],
                         ops.AgentCounts(tuple(counts), N, dev()))


# ---- 3. whole modules ---------------------------------------------------------------------------------------------
def _sub(case, rows):
    counts = [case["counts"][b] for b in rows]
    return dict(case, counts=counts, B=len(counts))


def _module_run(tag, module, state0, pairwise, scale, case, h, U_mod, R1, R2, nmp, rows, tol):
    """Scenes `rows` of the batch as a ragged batch of their own: oracle and HIP, forward and backward, gated at tol."""
    sub = _sub(case, rows)
    hs, Us = h[rows].contiguous(), [u[rows].contiguous() for u in U_mod]
    R1s, R2s = R1[rows].contiguous(), R2[rows].contiguous()
    ref = RB.module_oracle(state0, pairwise, scale, sub, hs, Us, R1s, R2s, nmp)
    for p in module.parameters():
        p.grad = None
    x = hs.to(dev()).requires_grad_(True)
    nz = [u.to(dev()) for u in Us]
    if pairwise:
        nf, fac = module(x, noise_u=nz, n_agents=sub["counts"])
    else:
        module.scale = scale
        corr = C.garbage_corr(sub, C.padded_corr(sub, hs)).to(dev())
        nf, fac, H = module(x, corr, noise_u=nz, n_agents=sub["counts"])
        assert torch.equal(H.cpu(), C.padded_incidence(sub, hs, scale))
    e_nf = float((nf.detach().double().cpu() - ref["node_feat"]).abs().max())
    e_fac = float((fac.detach().double().cpu() - ref["factors"]).abs().max())
    assert e_nf <= 1e-5 and e_fac <= 1e-5, (tag, e_nf, e_fac)
    for b, n in enumerate(sub["counts"]):          # padded positions of the outputs: zeros
        assert not bool(nf[b, n:].any())
        valid = torch.zeros(fac.shape[1], dtype=torch.bool)
        valid[RB.valid_factor_rows(case["N"], n, fac.shape[1], pairwise)] = True
        assert not bool(fac[b][~valid.to(dev())].any())
    # R1 / R2 are non-zero at padded positions too: the backward must drop them
    ((nf * R1s.to(dev())).sum() + (fac * R2s.to(dev())).sum()).backward()
    for b, n in enumerate(sub["counts"]):
        assert torch.equal(x.grad[b, n:], torch.zeros_like(x.grad[b, n:])), (tag, "padded rows of dL/dh", b)
    eh = float((x.grad.double().cpu() - ref["g_h"]).abs().max()) / float(ref["g_h"].abs().max())
    assert eh <= tol, (tag, "dL/dh", eh, tol)
    used = [k for k, v in ref["grads"].items() if v is not None and float(v.abs().max()) > 0]
    ew, where = _check({k: p.grad for k, p in module.named_parameters()}, ref["grads"], used, tol)
    return ref["clean"], eh, ew, where, len(used)


def _module_case(kind, N, counts, scale, nmp, min_used):
    pairwise = kind == "pair"
    case = RB.settled_case(N, counts, [] if pairwise else [scale], seed=N, nmp=nmp)
    h, U = C.inputs(case, nmp)
    h = C.with_garbage(case, h)
    assert C.min_gap(case, h) >= C.MIN_GAP
    pair, hyper = _modules(300 + N, nmp)
    module = pair if pairwise else hyper
    state0 = {k: v.detach().clone() for k, v in module.state_dict().items()}
    module.to(dev()).train()
    g = torch.Generator().manual_seed(5)
    B = case["B"]
    E = N * N if pairwise else (1 if scale == N else N)
    R1, R2 = torch.randn(B, N, 64, generator=g), torch.randn(B, E, module.edge_types, generator=g)
    U_mod = U[0] if pairwise else U[1]
    tag = f"ragged {kind} N={N} counts={list(counts)} scale={scale} nmp={nmp}"
    args = (module, state0, pairwise, scale, case, h, U_mod, R1, R2, nmp)
    clean, eh, ew, where, n_used = _module_run(tag, *args, list(range(B)), TOL_ANY)
    assert n_used >= min_used * (nmp if not pairwise else 1), n_used
    msg = f"\n{tag}: whole batch dL/dh {eh:.1e}, worst parameter {ew:.1e} ({where}); {int(clean.sum())}/{B} scenes clean"
    if bool(clean.all()):
        assert eh <= TOL_CLEAN and ew <= TOL_CLEAN, (tag, eh, ew, where)
        msg += "; all clean: gated at 2e-5"
    elif bool(clean.any()):
        rows = [b for b in range(B) if bool(clean[b])]
        _, eh2, ew2, where2, _ = _module_run(tag + " clean scenes", *args, rows, TOL_CLEAN)
        msg += f"; clean scenes {rows} alone dL/dh {eh2:.1e}, worst parameter {ew2:.1e} ({where2})"
    print(msg)


@pytest.mark.parametrize("N,counts,nmp", [(5, (5, 3, 2, 1), 1), (17, (17, 9, 1), 1), (6, (6, 4, 2, 1), 2)])
def test_pairwise_module_ragged_gradients(N, counts, nmp):
    _module_case("pair", N, counts, None, nmp, 30)


@pytest.mark.parametrize("N,counts,scale,nmp", [(7, (7, 4, 3, 2, 1), 3, 1), (7, (7, 4, 3, 2, 1), 7, 1), (17, (17, 6, 3), 5, 1),
                                                (6, (6, 4, 2, 1), 3, 2)])
def test_hyper_module_ragged_gradients(N, counts, scale, nmp):
    _module_case("hyper", N, counts, scale, nmp, 40)


# ---- 4. the block -------------------------------------------------------------------------------------------------
def test_block_ragged_gradients_and_one_sgd_step():
    case = C.BY_ID["n7"]
    B, N, counts, scales = case["B"], case["N"], case["counts"], case["scales"]
    blk, sp, shs = C.cpu_block(case)
    h, U = C.inputs(case)
    h = C.with_garbage(case, h)
    assert C.min_gap(case, h) >= C.MIN_GAP
    S = len(scales)
    g = torch.Generator().manual_seed(6)
    Rm = torch.randn(B, N, 64 * (1 + S), generator=g)           # over the module columns of `final`, padded rows included
    refs = []
    for i, (state, s) in enumerate(zip([sp, *shs], [None, *scales])):
        E = N * N if s is None else (1 if s == N else N)
        K = C.K_PAIR if s is None else C.K_HYPER
        refs.append(RB.module_oracle(state, s is None, s, case, h, U[i], Rm[..., 64 * i:64 * (i + 1)], torch.zeros(B, E, K)))
    g_f = sum(r["g_h"] for r in refs)
    clean = torch.stack([r["clean"] for r in refs]).all(dim=0)
    blk.to(dev()).train()
    x = h.to(dev()).requires_grad_(True)
    noise = [[u.to(dev()) for u in Um] for Um in U]
    final, new_H = blk(x, noise_u=noise, n_agents=counts)
    want = torch.cat([r["node_feat"] for r in refs], dim=-1)
    assert float((final[..., 64:].detach().double().cpu() - want).abs().max()) <= 1e-5
    assert torch.equal(final[..., :64], x.detach())
    (final[..., 64:] * Rm.to(dev())).sum().backward()
    for b, n in enumerate(counts):
        assert torch.equal(x.grad[b, n:], torch.zeros_like(x.grad[b, n:]))
    tol = TOL_CLEAN if bool(clean.all()) else TOL_ANY
    eh = float((x.grad.double().cpu() - g_f).abs().max()) / float(g_f.abs().max())
    assert eh <= tol, ("dL/df", eh, tol)
    worst = []
    for prefix, r in zip(["interaction."] + [f"interaction_hyper.{i}." for i in range(S)], refs):
        used = [k for k, v in r["grads"].items() if v is not None and float(v.abs().max()) > 0]
        hip = {k[len(prefix):]: p.grad for k, p in blk.named_parameters() if k.startswith(prefix)}
        worst.append(_check(hip, r["grads"], used, tol))
    print(f"\nragged block n7: dL/df {eh:.1e}, worst parameter per module {worst}; {int(clean.sum())}/{B} scenes clean, "
          f"gate {tol:g}")
    with torch.no_grad():
        _, H_inf = blk.eval()(x.detach(), noise_u=noise, n_agents=counts)
    assert torch.equal(new_H, H_inf)
    # one SGD step lowers the loss (as test_multiscale_block_trains_one_sgd_step; over the module columns — the first
    # 64 are the copy of f, whose padded rows hold the garbage and would drown the change in fp32)
    blk.train()
    target = torch.randn(B, N, blk.out_features - 64, generator=g).to(dev())
    opt = torch.optim.SGD(blk.parameters(), lr=0.05)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out, _ = blk(x.detach(), noise_u=noise, n_agents=counts)
        loss = ((out[..., 64:] - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[2] < losses[0], losses


# ---- 5. plumbing ---------------------------------------------------------------------------------------------------
def _pair_and_input(N=5, B=3, seed=11):
    pair, hyper = _modules(seed)
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(B, N, 64, generator=g)
    U = [torch.rand(B, N * N, 6, generator=g)]
    return pair.to(dev()).train(), hyper.to(dev()).train(), h, U


def test_counts_all_N_take_the_full_batch_training_path():
    pair, hyper, h, U = _pair_and_input()
    x, nz = h.to(dev()).requires_grad_(True), [U[0].to(dev())]
    a = pair(x, noise_u=nz, n_agents=[5, 5, 5])
    b = pair(x, noise_u=nz)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].requires_grad
    torch.manual_seed(3)
    a = pair(x, n_agents=torch.tensor([5, 5, 5]))
    torch.manual_seed(3)
    b = pair(x)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_without_the_opt_in_training_is_refused():
    import groupnet_amd as G
    from groupnet_amd.multiscale import MultiScaleHGNN
    pair, hyper, h, U = _pair_and_input()
    x = h.to(dev()).requires_grad_(True)
    corr = torch.zeros(3, 5, 5, device=dev())
    blk = MultiScaleHGNN([2, 5]).to(dev()).train()
    G.set_ragged_training(False)
    for call in (lambda: pair(x, n_agents=[5, 2, 1]), lambda: hyper(x, corr, n_agents=[5, 2, 1]),
                 lambda: blk(x, n_agents=[5, 2, 1])):
        with pytest.raises(NotImplementedError, match="inference-only"):
            call()
    G.set_ragged_training(True)
    # still refused with it: listall, a handed-in H, a padded size beyond the per-scene backward
    hyper.listall = True
    try:
        with pytest.raises(NotImplementedError, match="listall"):
            hyper(x, corr, n_agents=[5, 2, 1])
    finally:
        hyper.listall = False
    with pytest.raises(ValueError):
        hyper(x, corr, H=torch.zeros(3, 5, 5, device=dev()), n_agents=[5, 2, 1])
    big = torch.zeros(1, 141, 64, device=dev(), requires_grad=True)
    with pytest.raises(NotImplementedError, match="140"):
        pair(big, n_agents=[100])
    with pytest.raises(ValueError):
        pair(x, n_agents=[5, 0, 1])


def test_backward_after_an_in_place_weight_update_still_raises():
    pair, _, h, U = _pair_and_input()
    x = h.to(dev()).requires_grad_(True)
    nf, fac = pair(x, noise_u=[U[0].to(dev())], n_agents=[5, 2, 1])
    with torch.no_grad():
        next(pair.parameters()).add_(1.0)
    with pytest.raises(RuntimeError, match="modified in place"):
        (nf.sum() + fac.sum()).backward()


def test_bf16_input_trains_through_the_fp32_path():
    pair, _, h, U = _pair_and_input()
    counts = [5, 2, 1]
    x = h.to(dev()).bfloat16().requires_grad_(True)
    nf, fac = pair(x, noise_u=[U[0].to(dev())], n_agents=counts)
    assert nf.dtype == torch.bfloat16 and fac.dtype == torch.bfloat16
    (nf.float().sum() + fac.float().sum()).backward()
    assert x.grad.dtype == torch.bfloat16 and bool(torch.isfinite(x.grad.float()).all())
    for b, n in enumerate(counts):
        assert not bool(x.grad[b, n:].any()) and bool(x.grad[b, :n].any())
        assert not bool(nf[b, n:].any())
