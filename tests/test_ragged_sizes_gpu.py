"""Ragged batches (`n_agents=`) on the device at the batch sizes where the launchers pack several scenes into a
workgroup, remap workgroups over the XCDs, rank a whole scene per top-k band and stride the scatter — the shapes the
small cases of tests/test_ragged_gpu.py (B = 2 ... 6) never reach.  Cases, inputs and the float64 oracle by count class:
tests/ragged_size_cases.py; what every launch is planned as, and that the inputs can tell a workgroup's first count from
a scene's own: tests/test_ragged_sizes_cpu.py.

EVERY scene of a batch is compared (n50-b521: a sample of whole workgroups), padded positions must be exactly zero over
the whole batch (one mask comparison on the device), outputs of the single-stage entry points start from NaN, and the
library is asked for the plan of each launch with the product's own arguments.

Gates (the project's, unchanged).  fp32 storage: 1e-5 absolute against float64; affinities 2e-6; incidences bit for bit;
bf16 storage: TOL_ORACLE of tests/test_bf16_gpu.py of the module's largest |reference|, absolute on factors, against the
oracle fed the bf16-rounded features.
"""
import contextlib
import ctypes

import pytest
import torch

import ragged_cases as C
import ragged_size_cases as S
from launch_forms import CAPPED_GRID
from test_bf16_gpu import TOL_ORACLE
from test_ragged_gpu import _node_rows, precision
from test_ragged_sizes_cpu import N2E_RUNS, assert_n2e_plan

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def outputs_from_nan(monkeypatch):
    """Every floating tensor the entry points allocate for their results starts as NaN: a position the launch does not
    write shows."""
    real = torch.empty

    def empty(*a, **k):
        t = real(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t
    monkeypatch.setattr(torch, "empty", empty)
    try:
        yield
    finally:
        monkeypatch.setattr(torch, "empty", real)


def spy_plans(monkeypatch, log, stems):
    """Ask the library, at every launch of `stems` through ops._fn, for the plan of that launch with the very arguments
    the product passes (without the stream): log gets (stem, rc, plan)."""
    from groupnet_amd import _lib, ops
    real = ops._fn

    def fn(stem, dt):
        f = real(stem, dt)
        if stem not in stems:
            return f

        def call(*a):
            plan = _lib.LaunchPlan()
            log.append((stem, real(stem + "_plan", dt)(*a[:-1], ctypes.byref(plan)), plan))
            return f(*a)
        return call
    monkeypatch.setattr(ops, "_fn", fn)


def worst(got, ref, scenes=None):
    """(largest |got - ref| in float64 on the device, the scene it occurs in); NaN counts as infinite."""
    err = (got.double() - ref.to(got.device)).abs().flatten(1).amax(1)
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    if scenes is not None:
        keep = torch.zeros_like(err, dtype=torch.bool)
        keep[torch.as_tensor(list(scenes), device=err.device)] = True
        err = err.masked_fill(~keep, 0.0)
    b = int(err.argmax())
    return float(err[b]), b


def padding_is_zero(t, valid):
    """Every position of t outside `valid` (a CPU bool mask over t's leading dims) is exactly zero — on the device."""
    v = valid.to(t.device)
    v = v.reshape(v.shape + (1,) * (t.dim() - v.dim()))
    return not bool((t.masked_fill(v, 0) != 0).any())


def on_device(case, t, valid, bf16, seed=77):
    """t with garbage (N(0,1) x 100) outside `valid`, on the device in its storage type."""
    x = S.with_garbage(case, t, valid, seed).to(dev())
    return x.bfloat16() if bf16 else x


# ---------------------------------------------------------------------------------------------------------------------
# a. node -> edge
# ---------------------------------------------------------------------------------------------------------------------
def sampled_scenes(case, SG):
    """n50-b521: the first and the last workgroup and every scene of 16 seeded workgroups, 64 scenes at most."""
    B = case["B"]
    n_wg = (B + SG - 1) // SG
    gen = torch.Generator().manual_seed(50)
    wgs = {0, n_wg - 1} | set(torch.randperm(n_wg, generator=gen)[:16].tolist())
    scenes = sorted(b for w in wgs for b in range(w * SG, min(B, (w + 1) * SG)))
    assert len(scenes) <= 64
    return scenes


@pytest.mark.parametrize("case_id,groups,form,dtype", N2E_RUNS, ids=[f"{c}-{g or 'alone'}-{f}-{d}" for c, g, f, d in N2E_RUNS])
def test_node2edge_at_launch_sizes(case_id, groups, form, dtype, monkeypatch):
    """Hyper groups in one launch, banded and row form (by switch; by size at n50-b521), and the pairwise graph ordered
    and symmetric: every scene against the float64 `O.node2edge` of its count class; the plan of the very launch."""
    from groupnet_amd import ops
    base, bf16 = S.BY_ID[case_id], dtype == "bf16"
    case = S.groups_of(base, groups) if groups else base
    B, N, scales, counts = case["B"], case["N"], case["scales"], case["counts"]
    SG, last, rows = S.N2E_REACHES[(case_id, groups, form)]
    blk, sp, shs = C.cpu_block(case)
    blk = blk.to(dev()).eval()
    h, _ = S.inputs(case_id, bf16)
    x = on_device(case, h, S.valid_nodes(case), bf16)
    plans, bad = [], []
    spy_plans(monkeypatch, plans, ("gn_node2edge_ragged",))
    if S.SWITCH[form] is None:
        monkeypatch.delenv("GN_N2E_ROWS", raising=False)
    else:
        monkeypatch.setenv("GN_N2E_ROWS", S.SWITCH[form])
    scenes = sampled_scenes(case, SG) if case_id == "n50-b521" else None
    with torch.no_grad():
        if groups is not None:
            Hs = [S.padded_incidence(case, h, s) for s in scales]
            items = [_node_rows(m, x) for m in blk.interaction_hyper]
            items = [(xp, pq, H.to(dev()), w2, b2) for (xp, pq, w2, b2), H in zip(items, Hs)]
            with outputs_from_nan(monkeypatch):
                got = ops.node2edge_grouped(items, n_agents=counts)
            refs = S.hyper_n2e_oracle(case, h, shs, scenes)
            kinds = list(scales)
            same = ops.node2edge_grouped(items, n_agents=[N] * B)
            assert all(torch.equal(p, q) for p, q in zip(same, ops.node2edge_grouped(items)))
        else:
            sym = form == "pair-sym"
            xp, pq, w2, b2 = _node_rows(blk.interaction, x)
            with outputs_from_nan(monkeypatch):
                got = [ops.node2edge(xp, pq, None, w2, b2, sym=sym, n_agents=counts)]
            refs, kinds = [S.pair_n2e_oracle(case, h, sp, sym)], ["sym" if sym else "ord"]
            assert torch.equal(ops.node2edge(xp, pq, None, w2, b2, sym=sym, n_agents=[N] * B),
                               ops.node2edge(xp, pq, None, w2, b2, sym=sym))
    (_, rc, plan), = plans                             # (the calls without padded scenes take the plain entry point)
    assert rc == 0
    for kind, g, ref in zip(kinds, got, refs):
        assert g.dtype == x.dtype
        err, b = worst(g, ref, scenes)
        tol = TOL_ORACLE * float(ref.abs().max()) if bf16 else C.TOL
        print(f"\nn2e {case_id} {groups} {form} {dtype} group {kind}: {err:.2e} (gate {tol:.2e}) at scene {b}, "
              f"n = {counts[b]}")
        if not err <= tol:
            bad.append(f"group {kind}: {err:.3e} > {tol:.3e} at scene {b} (n = {counts[b]}, workgroup of {SG} from "
                       f"scene {b - b % SG}: counts {counts[b - b % SG:b - b % SG + SG]})")
        if not padding_is_zero(g, S.valid_rows(case, kind)):
            bad.append(f"group {kind}: padded rows are not zero")
    assert not bad, "\n".join(bad)
    n = len(got)
    assert_n2e_plan(plan, n, S.launch_plan(case_id, groups, form), (case_id, groups, form))
    assert list(plan.spw[:n]) == [SG] * n and plan.variant == rows and plan.xcd == 1
    assert last is None or B % SG == last


# ---------------------------------------------------------------------------------------------------------------------
# b. incidence
# ---------------------------------------------------------------------------------------------------------------------
GRAPH_CASES = ["n7-b2050", "n17-b1030"]


def graph_scales(case):
    return case["stage_scales"] or case["scales"]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case_id", GRAPH_CASES)
def test_fused_affinity_topk_at_launch_sizes(case_id, dtype, monkeypatch):
    from groupnet_amd import ops
    case, bf16 = S.BY_ID[case_id], dtype == "bf16"
    B, N, counts, scales = case["B"], case["N"], case["counts"], graph_scales(S.BY_ID[case_id])
    h, _ = S.inputs(case_id, bf16)
    x = on_device(case, h, S.valid_nodes(case), bf16)
    final = torch.full((B, N, 128), float("nan"), dtype=x.dtype, device=dev())
    plans = []
    spy_plans(monkeypatch, plans, ("gn_affinity_topk_ragged",))
    with torch.no_grad(), outputs_from_nan(monkeypatch):
        corr, Hs, H_cat = ops.affinity_topk(x, scales, want_corr=True, f_out=final[..., :64], want_H_cat=True,
                                            n_agents=torch.tensor(counts))
    (_, rc, plan), = plans
    assert rc == 0 and list(plan.grid) == [B, 1, 1]
    want_H = [S.padded_incidence(case, h, s) for s in scales]
    for s, H, W in zip(scales, Hs, want_H):
        assert H.dtype == torch.float32 and torch.equal(H, W.to(dev())), f"scale {s}"
    assert H_cat.dtype == x.dtype and torch.equal(H_cat.float(), torch.cat(want_H, dim=1).to(dev()))
    assert torch.equal(final[..., :64], x) and bool(torch.isnan(final[..., 64:]).all())
    err, b = worst(corr, S.padded_corr(case, h).double())
    print(f"\ncorr {case_id} {dtype}: {err:.2e} (gate {C.TOL_CORR:g}) at scene {b}")
    assert err <= C.TOL_CORR
    v = S.valid_nodes(case)
    assert padding_is_zero(corr, v[:, :, None] & v[:, None, :])
    with torch.no_grad():
        a = ops.affinity_topk(x, scales, want_corr=True, want_H_cat=True, n_agents=[N] * B)
        c = ops.affinity_topk(x, scales, want_corr=True, want_H_cat=True)
    assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2]) and all(torch.equal(p, q) for p, q in zip(a[1], c[1]))


@pytest.mark.parametrize("case_id", GRAPH_CASES)
def test_banded_topk_at_launch_sizes(case_id, monkeypatch):
    """The stand-alone top-k with a whole scene per band (TE = N) on a caller's corr whose padded rows and columns hold
    garbage."""
    from groupnet_amd import _lib, ops
    case = S.BY_ID[case_id]
    B, N, counts, scales = case["B"], case["N"], case["counts"], graph_scales(case)
    h, _ = S.inputs(case_id)
    v = S.valid_nodes(case)
    corr = on_device(case, S.padded_corr(case, h), v[:, :, None] & v[:, None, :], False, seed=78)
    lb, plans = _lib.load(), []
    real = lb.gn_topk_incidence_ragged_f32

    def launch(*a):
        plan = _lib.LaunchPlan()
        plans.append((lb.gn_topk_incidence_ragged_plan_f32(*a[:-1], ctypes.byref(plan)), plan))
        return real(*a)
    monkeypatch.setattr(lb, "gn_topk_incidence_ragged_f32", launch)
    with torch.no_grad():
        with outputs_from_nan(monkeypatch):
            Hs = ops.topk_incidence(corr, scales, n_agents=counts)
        (rc, plan), = plans
        assert rc == 0 and plan.TE == N and list(plan.grid) == [1, B, 1]
        for s, H in zip(scales, Hs):
            assert torch.equal(H, S.padded_incidence(case, h, s).to(dev())), f"scale {s}"
        full = ops.topk_incidence(corr, scales)
        assert all(torch.equal(p, q) for p, q in zip(ops.topk_incidence(corr, scales, n_agents=[N] * B), full))
        assert not all(torch.equal(p, q) for p, q in zip(Hs, full))


# ---------------------------------------------------------------------------------------------------------------------
# c. scatter
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("divisor", [None, 1.0], ids=["own-count", "one"])
def test_scatter_strides_over_a_ragged_batch(divisor, monkeypatch):
    """n17-b1930, one launch over the pairwise graph (sym and ordered) and the hyper scales 2 / 5 / 17: the grid is capped
    at 4096 workgroups and strides.  Against the float64 cat(H^T feat, ori) / divisor of every scene alone, by class."""
    from groupnet_amd import ops
    case = S.BY_ID["n17-b1930"]
    B, N, scales, counts = case["B"], case["N"], case["scales"], case["counts"]
    h, _ = S.inputs(case["id"])
    v = S.valid_nodes(case)
    ori = S.with_garbage(case, h, v)
    gen = torch.Generator().manual_seed(5 + case["seed"])
    kinds = ["sym", "ord"] + list(scales)
    feats = []
    for kind in kinds:              # N(0,1) where a scene reads, x 100 where it must not
        own = S.valid_rows(case, kind)
        f = torch.randn(B, own.shape[1], 64, generator=gen)
        feats.append(torch.where(own[..., None], f, f * 100.0))
    Hs = [None, None] + [S.padded_incidence(case, h, s) for s in scales]
    od = ori.to(dev())
    items = [(f.to(dev()), None if H is None else H.to(dev()), od, i == 0) for i, (f, H) in enumerate(zip(feats, Hs))]
    plans = []
    spy_plans(monkeypatch, plans, ("gn_agg_scatter_ragged",))
    with torch.no_grad(), outputs_from_nan(monkeypatch):
        outs = ops.agg_scatter_grouped(items, divisor, n_agents=counts)
    (_, rc, plan), = plans
    assert rc == 0 and plan.grid[0] == CAPPED_GRID == 4096 and B * N * 32 > CAPPED_GRID * 256
    refs = [torch.zeros(B, N, 64, dtype=torch.float64) for _ in kinds]
    for n, idx in S.classes(case):
        d = float(n) if divisor is None else divisor
        rows, _ = S.sym_rows(N, n)
        R = torch.zeros(n, n, dtype=torch.long)
        iu = torch.triu_indices(n, n)
        R[iu[0], iu[1]] = rows
        R = torch.maximum(R, R.t())                                          # the row of the unordered pair {a, j}
        for ref, kind, f, H in zip(refs, kinds, feats, Hs):
            fd = f[idx].double()
            if kind == "sym":
                agg = fd[:, R].sum(2)
            elif kind == "ord":
                e = fd.view(len(idx), N, N, 64)[:, :n, :n]
                agg = e.sum(2) + e.sum(1)
            else:
                agg = H[idx][:, :, :n].double().transpose(1, 2) @ fd
            ref[idx, :n] = agg / d
    dv = torch.tensor(counts, dtype=torch.float32) if divisor is None else torch.full((B,), float(divisor))
    want_ori = torch.where(v[..., None], ori / dv[:, None, None], torch.zeros(())).to(dev())      # true division
    bad = []
    for kind, out, ref in zip(kinds, outs, refs):
        err, b = worst(out[..., :64], ref)
        print(f"\nscatter {kind} divisor {divisor}: {err:.2e} (gate {C.TOL:g}) at scene {b}, n = {counts[b]}")
        if not err <= C.TOL:
            bad.append(f"group {kind}: {err:.3e} at scene {b} (n = {counts[b]})")
        if not torch.equal(out[..., 64:], want_ori):
            bad.append(f"group {kind}: the ori half is not ori / divisor, or its padding is not zero")
        if not padding_is_zero(out, v):
            bad.append(f"group {kind}: padded node rows are not zero")
    assert not bad, "\n".join(bad)
    if divisor is None:
        with torch.no_grad():
            assert all(torch.equal(p, q) for p, q in zip(ops.agg_scatter_grouped(items, n_agents=[N] * B),
                                                         ops.agg_scatter_grouped(items)))


# ---------------------------------------------------------------------------------------------------------------------
# d. whole block
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id,mode,dtype", S.BLOCKS, ids=[f"{c}-{p}-{d}" for c, p, d in S.BLOCKS])
def test_block_at_launch_sizes(case_id, mode, dtype, monkeypatch):
    """The multiscale block as it is built, on EVERY scene: features, every module's factors, new_H, the copy of f, one
    zeroing launch — as tests/test_ragged_gpu.py::test_block_on_a_ragged_batch checks them at B <= 6."""
    from groupnet_amd import MS_HGNN_batch as M, multiscale, ops
    case, bf16 = S.BY_ID[case_id], dtype == "bf16"
    B, N, scales, counts = case["B"], case["N"], case["scales"], case["counts"]
    ref_feats, ref_facs, scale = S.block_oracle(case_id, bf16)
    h, U = S.inputs(case_id, bf16)
    blk = C.cpu_block(case)[0].to(dev()).eval()
    zeroings, real_zero = [], ops.zero_padding
    monkeypatch.setattr(ops, "zero_padding", lambda *a, **k: zeroings.append(1) or real_zero(*a, **k))
    v = S.valid_nodes(case)
    x = on_device(case, h, v, bf16)
    nd = [[u.to(dev()) for u in us] for us in U]
    res, orig = {}, M.run_message_passing
    plans = []
    spy_plans(monkeypatch, plans, ("gn_node2edge_ragged",))

    def spy(*a, **k):
        r = orig(*a, **k)
        res.setdefault("all", []).extend(r)
        return r
    monkeypatch.setattr(multiscale, "run_message_passing", spy)
    with precision(mode), torch.no_grad():
        out, new_H = blk(x, noise_u=nd, n_agents=counts)
        assert len(res["all"]) == 1 + len(scales) and len(zeroings) == 1
        facs = [r[1] for r in res["all"]]
        same = blk(x, noise_u=nd, n_agents=[N] * B)
        full = blk(x, noise_u=nd)
    assert torch.equal(same[0], full[0]) and torch.equal(same[1], full[1])
    _, rc, plan = plans[0]
    assert rc == 0 and min(plan.spw[:1 + len(scales)]) > 1 and plan.xcd == 1          # scenes share workgroups here too
    assert out.dtype == x.dtype and torch.equal(out[..., :64], x)                      # f copied through, padding included
    assert bool(torch.isfinite(out).all())
    assert torch.equal(new_H.float(), torch.cat([S.padded_incidence(case, h, s) for s in scales], dim=1).to(dev()))
    bad = []
    if not padding_is_zero(out[..., 64:], v):
        bad.append("padded node rows are not zero")
    feat_err, fac_err = [], []
    for i, kind in enumerate(["ord"] + list(scales)):
        e, b = worst(out[..., 64 * (1 + i):64 * (2 + i)], ref_feats[..., 64 * i:64 * (1 + i)])
        g, bf = worst(facs[i], ref_facs[i])
        feat_err.append(e)
        fac_err.append(g)
        tol_feat, tol_fac = (TOL_ORACLE * scale[i], TOL_ORACLE) if bf16 else (C.TOL, C.TOL)
        if not e <= tol_feat:
            bad.append(f"module {i}: features {e:.3e} > {tol_feat:.3e} at scene {b} (n = {counts[b]})")
        if not g <= tol_fac:
            bad.append(f"module {i}: factors {g:.3e} > {tol_fac:.3e} at scene {bf} (n = {counts[bf]})")
        if not padding_is_zero(facs[i], S.valid_rows(case, kind)):
            bad.append(f"module {i}: padded factors are not zero")
    print(f"\nblock {case_id} {mode} {dtype}: features {['%.1e' % e for e in feat_err]} of "
          f"{['%.2f' % s for s in scale]}, factors {['%.1e' % e for e in fac_err]}")
    assert not bad, "\n".join(bad)
