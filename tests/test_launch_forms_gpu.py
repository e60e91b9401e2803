"""The launch-size-selected kernel forms against a float64 oracle.

The launchers pick a work shape by launch size (tests/launch_forms.py `expected_forms`): waves per row block of the
typed aggregation, scenes per workgroup of the fused closing stage, the closing MLP kernel, the node -> edge form, the
gather's scene packing.  Every case here runs the HIP path on the WHOLE batch, so that the launcher picks the form the
case names, and compares a sample of ~32-64 scenes (first, last, scenes on row-block and workgroup boundaries of the
selected form, a seeded remainder) with the float64 oracle of those scenes.

Gates, the same at every size:
  * fp32 results (f16x3, bf16x6, fp32 cores): every module's features within TOL_FEAT x max|ref| of that module on
    the sample, factors within TOL_FAC absolute; incidence H bit-identical with the fp32-affinity ranking of the oracle;
  * bf16 storage: the relative gate of tests/test_bf16_gpu.py (TOL_ORACLE of max|ref|, and absolute on the factors)
    against the oracle; H exact on rows without near-ties, which may be at most 0.5 % of the rows (as there);
  * backward (fp32): L = <out, R> with R non-zero on chosen scenes only; dL/df of those scenes and every parameter
    gradient against float64 autograd, within TOL_CLEAN on clean scenes (see the backward test for config 4), and dL/df
    of every other scene exactly zero.
"""
import pytest
import torch

from launch_forms import (BACKWARD_CASES, FORWARD_CASES, assert_plans_match, block64, case_forms, clean_scenes, describe,
                          hyper64, hyper_incidence, sample_scenes, state64)
from test_backward_gpu import TOL_ANY, TOL_CLEAN
from test_bf16_gpu import TOL_ORACLE, block_and_states, safe_rows

pytestmark = pytest.mark.gpu

TOL_FEAT = 2e-6      # of max|ref| (the bound the suite applies between paths at B = 512)
TOL_FAC = 5e-6       # absolute, factors are probabilities
MIN_CLEAN = 24
PARAMS_PER_MODULE = 30    # fewest parameter tensors with a gradient per module (each Linear on the forward: weight + bias)
MAX_NEAR_TIE = 0.005      # largest share of incidence rows a bf16 case may leave out as near-ties (as test_bf16_gpu)


def dev():
    return torch.device("cuda:0")


def _precision(mode):
    from groupnet_amd import ops
    old = ops.precision()
    ops.set_precision(mode)
    return old


def _n_sample(N):
    return 32 if N >= 50 else 48


def _check_H(Hg, h, scenes, s, twin):
    """Hg: the HIP incidence of the sampled scenes (m, E, N) as float, against the oracle's fp32 ranking: exact, or for
    bf16 storage exact on the rows whose k-th / (k+1)-th affinity gap is not a near-tie.  -> (rows left out, rows)."""
    from oracle import ms_hgnn_oracle as O
    want = hyper_incidence(h, scenes, s)
    if not twin or s == h.shape[1]:
        assert torch.equal(Hg, want), f"scale {s}: incidence differs from the oracle"
        return 0, 0
    ok = safe_rows(O.affinity(h[scenes].float()), s)
    assert torch.equal(Hg[ok], want[ok]), f"scale {s}: incidence differs on tie-free rows"
    return int((~ok).sum()), ok.numel()


PLANNED = ("gn_agg_mlp", "gn_mlp2", "gn_node2edge", "gn_agg_gather")


def _spy_plans(monkeypatch, log):
    """Ask the library, at every launch of the PLANNED stages, for the plan of that launch with the very arguments the
    product passes (without the stream): log gets (stem, rc, plan)."""
    import ctypes
    from groupnet_amd import _lib, ops
    real = ops._fn

    def fn(stem, dt):
        f = real(stem, dt)
        if stem not in PLANNED:
            return f

        def call(*a):
            plan = _lib.LaunchPlan()
            log.append((stem, real(stem + "_plan", dt)(*a[:-1], ctypes.byref(plan)), plan))
            return f(*a)
        return call
    monkeypatch.setattr(ops, "_fn", fn)


@pytest.mark.parametrize("case", FORWARD_CASES, ids=[c["id"] for c in FORWARD_CASES])
def test_forward_forms_match_the_float64_oracle(case, monkeypatch):
    from groupnet_amd import multiscale
    plans = []
    _spy_plans(monkeypatch, plans)
    B, N, scales, twin = case["B"], case["N"], case["scales"], case["dtype"] == "bf16"
    forms = case_forms(case)
    scenes = sample_scenes(B, N, forms, n=_n_sample(N), seed=B + N)
    torch.manual_seed(1000 + B + N)
    h = torch.randn(B, N, 64)
    if twin:
        h = h.bfloat16().float()            # the oracle runs on the bf16-rounded inputs
    chunk = 2 if N >= 50 else None
    old = _precision(case["precision"])
    try:
        if case["kind"] == "hyper":
            import groupnet_amd as G
            (s,) = scales
            torch.manual_seed(31)
            mod = G.MS_HGNN_hyper(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=64, batch_norm=0, nmp_layers=1,
                                  scale=s).to(dev()).eval()
            st = {k: v.detach().cpu().clone() for k, v in mod.state_dict().items()}
            from oracle import ms_hgnn_oracle as O
            U = [torch.rand(B, 1 if s == N else N, 10)]
            with torch.no_grad():
                nf, fac, H = mod(h.to(dev()), O.affinity(h).to(dev()), noise_u=[U[0].to(dev())])
            sel = scenes.to(dev())
            Hg, out_g, facs_g = H[sel].float().cpu(), nf[sel].double().cpu(), [fac[sel].double().cpu()]
            _check_H(Hg, h, scenes, s, False)
            total = 0
            ref_nf, ref_fac = hyper64(st, h, Hg, U, scenes)
            out_r, facs_r, fcols = ref_nf, [ref_fac], [(0, 64)]
            unsafe = 0
        else:
            blk, sp, shs = block_and_states(scales, seed=7 + N)
            noise = [[torch.rand(shp)] for shp in blk.noise_shapes(B, N)]
            got = {}
            orig = multiscale.run_message_passing

            def spy(*a, **k):           # the block's own grouped launch; keep its factors
                got["res"] = orig(*a, **k)
                return got["res"]
            monkeypatch.setattr(multiscale, "run_message_passing", spy)
            x = h.to(dev()).bfloat16() if twin else h.to(dev())
            with torch.no_grad():
                out, H = blk(x, noise_u=[[u[0].to(dev())] for u in noise])
            sel = scenes.to(dev())
            out_g, Hall = out[sel].double().cpu(), H[sel].float().cpu()
            facs_g = [r[1][sel].double().cpu() for r in got["res"]]
            Hs, row0, unsafe, total = [], 0, 0, 0
            for s in scales:
                E = 1 if s == N else N
                Hs.append(Hall[:, row0:row0 + E])
                u, t = _check_H(Hs[-1], h, scenes, s, twin)
                unsafe, total, row0 = unsafe + u, total + t, row0 + E
            assert torch.equal(out_g[..., :64], h[scenes].double())       # f copied through
            out_r, facs_r = block64(sp, shs, scales, h, Hs, noise[0], noise[1:], scenes, chunk=chunk)
            fcols = [(64 * (1 + i), 64 * (2 + i)) for i in range(1 + len(scales))]
    finally:
        _precision(old)
    # the forward reached the forms the case names: one launch per planned stage (nmp = 1), each as `forms` says, the
    # aggregation launch carrying the closing stage exactly when `fused_closing`
    assert all(rc == 0 for _, rc, _ in plans), [(stem, rc) for stem, rc, _ in plans]
    by_stem = {stem: [p for s_, _, p in plans if s_ == stem] for stem in PLANNED}
    assert len(by_stem["gn_agg_mlp"]) == 1 and all(len(v) <= 1 for v in by_stem.values()), {k: len(v) for k, v in by_stem.items()}
    assert_plans_match(forms, *[(by_stem[stem] or [None])[0] for stem in PLANNED], case["id"])
    errs = [float((out_g[..., a:b] - out_r[..., a:b]).abs().max()) / float(out_r[..., a:b].abs().max()) for a, b in fcols]
    ferrs = [float((fg - fr).abs().max()) for fg, fr in zip(facs_g, facs_r)]
    print(f"\n{case['id']}: {describe(forms)}\n   {len(scenes)} scenes: features rel err per module "
          f"{['%.2e' % e for e in errs]}, factors abs err {['%.2e' % e for e in ferrs]}"
          f"{', near-tie rows %d/%d' % (unsafe, total) if twin else ''}")
    if twin:
        assert unsafe <= MAX_NEAR_TIE * max(total, 1), (unsafe, total)
        assert max(errs) <= TOL_ORACLE
        assert max(ferrs) <= TOL_ORACLE
    else:
        assert max(errs) <= TOL_FEAT, (case["id"], errs)
        assert max(ferrs) <= TOL_FAC, (case["id"], ferrs)


def _backward(blk, sp, shs, scales, f, noise, loss_scenes, with_pair, with_hyper, chunk):
    """L = <out, R>, R non-zero only on `loss_scenes` and on the columns of f and of the modules selected.  The HIP
    training forward + backward on the whole batch against float64 autograd of the oracle on those scenes.
    Returns (dL/df error, worst parameter error, its name, number of parameters compared)."""
    B, N = f.shape[0], f.shape[1]
    R = torch.zeros(B, N, blk.out_features)
    R[loss_scenes] = torch.randn(len(loss_scenes), N, blk.out_features)
    if not with_pair:
        R[..., 64:128] = 0
    if not with_hyper:
        R[..., 128:] = 0
    for p in blk.parameters():
        p.grad = None
    x = f.to(dev()).requires_grad_(True)
    out, H = blk(x, noise_u=[[u[0].to(dev())] for u in noise])
    (out * R.to(dev())).sum().backward()
    gx = x.grad.cpu()
    Hc, row0, Hs = H.detach()[loss_scenes.to(dev())].float().cpu(), 0, []
    for s in scales:
        E = 1 if s == N else N
        Hs.append(Hc[:, row0:row0 + E])
        assert torch.equal(Hs[-1], hyper_incidence(f, loss_scenes, s)), f"scale {s}: incidence"
        row0 += E
    st_p, st_h = state64(sp, True), [state64(s_, True) for s_ in shs]
    hh = f[loss_scenes].double().requires_grad_(True)
    out64, _ = block64(st_p, st_h, scales, hh, Hs, [noise[0][0][loss_scenes]], [[u[0][loss_scenes]] for u in noise[1:]],
                       torch.arange(len(loss_scenes)), chunk=chunk, with_pair=with_pair, with_hyper=with_hyper)
    (out64 * R[loss_scenes].double()).sum().backward()
    others = torch.ones(B, dtype=torch.bool)
    others[loss_scenes] = False
    assert bool((gx[others] == 0).all()), "dL/df of a scene without loss is not zero: a cross-scene write"
    eh = float((gx[loss_scenes].double() - hh.grad).abs().max()) / float(hh.grad.abs().max())
    ref = {f"interaction.{k}": v.grad for k, v in st_p.items()}
    for i, st in enumerate(st_h):
        ref.update({f"interaction_hyper.{i}.{k}": v.grad for k, v in st.items()})
    hip = {n: p.grad for n, p in blk.named_parameters()}
    used = [n for n, g in ref.items() if g is not None and float(g.abs().max()) > 0]
    assert len(used) >= PARAMS_PER_MODULE * (len(scales) * with_hyper + with_pair)
    gmax = max(float(ref[n].abs().max()) for n in used)
    worst, where = 0.0, None
    for n in used:      # as test_backward_gpu._check: relative to the parameter's own scale, floored at 1 % of the largest
        assert hip[n] is not None, n
        sc = max(float(ref[n].abs().max()), 1e-2 * gmax)
        e = float((hip[n].cpu().double() - ref[n]).abs().max()) / sc
        if e > worst:
            worst, where = e, n
    for n, g in hip.items():            # parameters without oracle gradient get none (or exact zeros) from the HIP path
        if n not in used and g is not None:
            assert bool((g == 0).all()), n
    return eh, worst, where, len(used)


@pytest.mark.parametrize("case", BACKWARD_CASES, ids=[c["id"] for c in BACKWARD_CASES])
def test_backward_forms_match_float64_autograd(case):
    """Training forward + HIP backward of the block at full size against float64 autograd of the oracle.

    Gate TOL_CLEAN on clean scenes only (relu_probe.py: no oracle ReLU input within the rounding window of zero): N = 11
    takes them from a sample of 128 scenes aimed at the form boundaries (~40 % are clean).  At N = 50 (config 4) a scene
    is clean far less often — measured on this case: 37 of 1024 scenes in the hyper modules, none in the pairwise module
    (~7 M ReLU units per scene) — so:
      * the hyper modules (and f): loss on the clean scenes of the WHOLE batch, gate TOL_CLEAN;
      * the pairwise module: a second backward with the loss on its columns of 8 sampled scenes, none of them clean, gated
        at TOL_ANY — test_backward_gpu's gate for batches with a ReLU unit inside the window, the gate its own N = 50
        pairwise case gets."""
    B, N, scales = case["B"], case["N"], case["scales"]
    forms = case_forms(case)
    blk, sp, shs = block_and_states(scales, seed=50 + N)
    blk.train()
    torch.manual_seed(2000 + B)
    f = torch.randn(B, N, 64)
    noise = [[torch.rand(shp)] for shp in blk.noise_shapes(B, N)]
    small = N <= 16
    pool = sample_scenes(B, N, forms, n=128, seed=B) if small else torch.arange(B)
    Hp = [hyper_incidence(f, pool, s) for s in scales]
    keep = clean_scenes(sp, shs, scales, f, Hp, noise[0], noise[1:], pool, with_pair=small)
    clean = pool[keep][:96]
    msg = f"\n{case['id']}: {describe(forms)}\n   {int(keep.sum())}/{len(pool)} scenes clean"
    assert len(clean) >= MIN_CLEAN, (int(keep.sum()), len(pool))
    eh, worst, where, n = _backward(blk, sp, shs, scales, f, noise, clean, small, True, None)
    msg += (f"; loss on {len(clean)} clean scenes{'' if small else ' (f and hyper columns)'}: dL/df {eh:.1e}, worst "
            f"parameter {worst:.1e} ({where}), {n} parameters (gate {TOL_CLEAN:g})")
    assert eh <= TOL_CLEAN and worst <= TOL_CLEAN, (eh, worst, where)
    if not small:
        loss = sample_scenes(B, N, forms, n=8, seed=B + 1)
        eh2, worst2, where2, n2 = _backward(blk, sp, shs, scales, f, noise, loss, True, False, 2)
        msg += (f"\n   pairwise columns on {len(loss)} sampled scenes: dL/df {eh2:.1e}, worst parameter {worst2:.1e} "
                f"({where2}), {n2} parameters (gate {TOL_ANY:g})")
        assert eh2 <= TOL_ANY and worst2 <= TOL_ANY, (eh2, worst2, where2)
    print(msg)
