"""A scene's result does not depend on its batch neighbours (tests/scene_isolation_cases.py states the property, the
cases and the batches; tests/test_scene_isolation_cpu.py checks that table and that the oracle itself isolates).

A — permutation.  The eval block on (h, U) and on (h[p], U[p]), p a seeded permutation without fixed points and the
    reversal: out[p], every module's factors and every incidence are BIT-identical, and both runs took the same
    launches and plans.  A row's MFMA result does not depend on the other rows, reduction orders are fixed, the node
    form's clamp scale is a power of two (bit-identical to the max form), and nothing votes on N(0,1) data.
B — mixed batches.  One set of scenes under per-scene magnitudes (ordinary, 1e6, all-zero, 3e3, 1e12; then with
    overflowing 1e24 neighbours; then with an all-NaN and a +-inf neighbour): EVERY checked scene on its own against the
    float64 oracle of that scene alone, fed that scene's HIP incidence, every gate relative to that scene and module:
      features   ordinary / zero scenes TOL_FEAT x max(1, max|ref|); 3e3, 1e6, 1e12 scenes 2e-5 x max|ref|
                 (test_f16x3_range_vote_falls_back_to_bf16x6's); bf16 storage TOL_ORACLE x max|ref|;
      factors    finite; TOL_FAC absolute on ordinary scenes (bf16 storage: TOL_ORACLE), the prob_gate rule of
                 test_modules_under_extreme_magnitudes on large ones;
      incidence  equal to the oracle's fp32 ranking of that scene; bf16 storage: on the rows that are no near-tie, which
                 are all but MAX_NEAR_TIE of the checked rows (an all-zero scene's rows are one exact tie, lowest index
                 wins: compared in full);
      identity   where nothing votes (bf16x6, fp32 cores, bf16 storage) a checked scene's features, factors and
                 incidence are bit-identical between the all-ordinary batch, the mixed batches and both poisoned batches
                 (ordinary, all-zero and large scenes alike); f16x3: between the all-ordinary batch and batches whose
                 other scenes are all-zero.
    Large scenes on bf16 storage.  bf16 keeps 8 significant bits: a pre-softmax logit carries a few 2^-9 of the largest
    magnitude in its chain, and through exp(. / tau), tau = 0.5, a 3e3 .. 1e12 scene has edges whose sampled type the
    format does not determine (measured: 7e-2 .. 6e-1 of max|ref| from the end-to-end oracle, against 4e-3 on ordinary
    scenes).  Such a scene is gated in the parts the format does determine (scene_isolation_cases.TWIN_GAP): the edge
    head on the edges whose float64 winner leads by more than four times what a CPU restatement with bf16-rounded
    operands moves a logit (and by no less than 2^-5 of the module's max|logit + gumbel|) — there the twin puts at least
    1 - TOL_ORACLE on the same type, and at least one edge of the scene must be such an edge —, and
    everything behind the edge head — typed aggregation, scatter, closing MLP — against the float64 oracle GIVEN the
    twin's own edge features, at TOL_ORACLE of max|ref|; besides finite results, f copied through, the incidence, factor
    rows that sum to 1 within 2e-2, and the scene's bits being the same beside every set of neighbours.
    Large scenes on fp32 storage are gated against the float64 oracle on seeds that keep them well conditioned
    (scene_isolation_cases.LARGE_CONDITION, checked on the CPU).
    Nothing is asserted about a poisoned scene itself.
C — training.  The training forward and the HIP backward in a batch of magnitudes 1, 3e3, 1, 30, ...: the forward of
    the ordinary scenes at the gates of B, dL/df of every scene without loss exactly zero, dL/df and every parameter
    gradient against float64 autograd of the loss scenes alone (TOL_CLEAN on relu_probe-clean scenes, TOL_ANY
    otherwise, as test_launch_forms_gpu).
"""
import pytest
import torch

import scene_isolation_cases as C
from launch_forms import block64, hyper_incidence
from oracle import ms_hgnn_oracle as O
from test_backward_gpu import TOL_ANY, TOL_CLEAN
from test_bf16_gpu import TOL_ORACLE, safe_rows
from test_launch_forms_gpu import MAX_NEAR_TIE, TOL_FAC, TOL_FEAT, _backward, _spy_plans
from test_route_gpu import carried, check_follows, record

pytestmark = pytest.mark.gpu

TOL_LARGE = C.TOL_LARGE
TWIN_ROW_SUM = 2e-2   # K bf16 roundings of a distribution (test_bf16_modules_return_reference_shaped_tuples)
PROB_SLACK = {"f16x3": 4.0, "bf16x6": 1.0, "fp32": 1.0}      # test_modules_under_extreme_magnitudes; fp32 cores: 24-bit operands


def dev():
    return torch.device("cuda:0")


class Runner:
    """One case's block on the device, its scenes and noise, a recorder of the launches of every forward, and the
    per-scene oracle (computed once per scene, magnitude and incidence, shared by every batch that holds that scene)."""

    def __init__(self, case, monkeypatch, training=False):
        from groupnet_amd import MS_HGNN_batch as M, multiscale, ops
        self.case, self.twin = case, case["dtype"] == "bf16"
        blk, self.sp, self.shs = C.cpu_block(case)
        self.blk = blk.to(dev()).train(training)
        self.h0, self.U = C.base_inputs(case)
        self.plans, self.res, self.cache = [], {}, {}
        _spy_plans(monkeypatch, self.plans)
        self.calls = record(monkeypatch)
        orig = M.run_message_passing

        def spy(*a, **k):           # the block's own grouped launch; keep its factors
            self.res["res"] = orig(*a, **k)
            return self.res["res"]
        monkeypatch.setattr(multiscale, "run_message_passing", spy)
        monkeypatch.setattr(M, "run_message_passing", spy)
        self._old = (ops.precision(), ops._INCIDENCE_FORM)
        ops.set_precision(case["precision"])
        ops.set_incidence_form(case["incidence"])

    def close(self):
        from groupnet_amd import ops
        ops.set_precision(self._old[0])
        ops.set_incidence_form(self._old[1])

    def forward(self, h, U, grad=False):
        """-> {"out", "H", "facs" (per module), "sig" (the launches and plans of this forward)}, on the CPU in fp32
        (exact for bf16 storage)."""
        N = self.case["N"]
        x = h.to(dev()).bfloat16() if self.twin else h.to(dev())
        nd = [[u.to(dev()) for u in us] for us in U]
        n0, c0 = len(self.plans), len(self.calls)
        with torch.enable_grad() if grad else torch.no_grad():
            out, H = self.blk(x.requires_grad_(grad), noise_u=nd)
        torch.cuda.synchronize()
        sig = ([(stem, rc, bytes(p)) for stem, rc, p in self.plans[n0:]], [carried(c, N) for c in self.calls[c0:]])
        assert all(rc == 0 for _, rc, _ in sig[0]) and sig[1]
        heads = [c[3] for c in self.calls[c0:] if c[0] == "edge_mlp_gumbel_grouped"]
        return dict(out=out.detach().float().cpu(), H=H.detach().float().cpu(),
                    facs=[r[1].detach().float().cpu() for r in self.res["res"]], sig=sig, raw=self.calls[c0:],
                    efs=[r[0].detach().float().cpu() for r in heads[0]])      # the first round's fac x dist per module

    def split_H(self, H):
        """The incidence of every scale from the block's concatenation."""
        N, row0, Hs = self.case["N"], 0, []
        for s in self.case["scales"]:
            Hs.append(H[:, row0:row0 + C.n_edges(N, s)])
            row0 += Hs[-1].shape[1]
        assert row0 == H.shape[1]
        return Hs

    def oracle(self, h, b, mag, Hs, want32):
        """float64 oracle of scene b alone on its HIP incidence -> (out, factors per module, fp32 factors or None)."""
        key = (b, mag, tuple(H.numpy().tobytes() for H in Hs))
        hit = self.cache.get(key)
        if hit is None or (want32 and hit[2] is None):
            one, nmp = torch.tensor([b]), self.case["nmp"]
            with torch.no_grad():
                out, facs = block64(self.sp, self.shs, self.case["scales"], h, Hs, self.U[0], self.U[1:], one, nmp)
                f32 = C.oracle32(self.sp, self.shs, h, Hs, self.U, b, nmp)[1] if want32 else None
            hit = self.cache[key] = (out, facs, f32)
        return hit

    def gate(self, name, h, mags, got, scenes=None):
        """Every checked scene of the batch (or `scenes`) against its own oracle.  Prints every figure, then asserts."""
        case, twin, N = self.case, self.twin, self.case["N"]
        bad, unsafe, total = [], 0, 0
        Hall = self.split_H(got["H"])
        for b in (C.checked(mags) if scenes is None else scenes):
            m = mags[b]
            ordinary = C.is_ordinary(m)
            Hs = [H[b:b + 1] for H in Hall]
            for s, Hg in zip(case["scales"], Hs):
                want = hyper_incidence(h, torch.tensor([b]), s)
                if twin and m != 0.0 and s != N:
                    ok = safe_rows(O.affinity(h[b:b + 1]), s)
                    unsafe, total = unsafe + int((~ok).sum()), total + ok.numel()
                    same = torch.equal(Hg[ok], want[ok])
                else:
                    total += Hg.shape[1]
                    same = torch.equal(Hg, want)
                if not same:
                    bad.append(f"{name} scene {b} (x{m:g}) scale {s}: incidence differs from the oracle's")
            if not torch.equal(got["out"][b, :, :64], h[b]):
                bad.append(f"{name} scene {b} (x{m:g}): f is not copied through")
            out64, fac64, fac32 = self.oracle(h, b, m, Hs, want32=not ordinary and not twin)
            line, n_det = f"   {name:>10} scene {b} x{m:<6g}", 0
            for i in range(1 + len(case["scales"])):
                cols = slice(64 * (1 + i), 64 * (2 + i))
                ref, x = out64[0, :, cols], got["out"][b, :, cols].double()
                scale = float(ref.abs().max())
                err = float((x - ref).abs().max())
                tol = TOL_ORACLE * scale if twin else TOL_FEAT * max(1.0, scale) if ordinary else TOL_LARGE * scale
                fg = got["facs"][i][b:b + 1]
                ferr = float((fg.double() - fac64[i]).abs().max())
                if twin and not ordinary:       # scene_isolation_cases.TWIN_GAP: the parts the format determines
                    ef = got["efs"][i][b:b + 1]
                    y, ref = C.head_and_tail64((self.sp, *self.shs)[i], h, None if i == 0 else Hs[i - 1], self.U[i],
                                               C.ordered_edge_feat(ef, N) if i == 0 else ef, b)
                    ref = ref[0]
                    scale, err = float(ref.abs().max()), float((x - ref).abs().max())
                    tol = TOL_ORACLE * scale
                    Hi = None if i == 0 else Hs[i - 1]
                    det, winner, e_emu = C.determined_edges(y, C.head_y16((self.sp, *self.shs)[i], h, Hi, self.U[i], b))
                    won = fg.double().gather(-1, winner)[..., 0][det]
                    ferr = float((1.0 - won).max()) if det.any() else 0.0
                    n_det += int(det.sum())
                    line += f" | {int(det.sum())}/{det.numel()} edges determined (e_emu {e_emu:.1e} of {float(y.abs().max()):.1e})"
                    fok = ferr <= TOL_ORACLE and float((fg.sum(-1) - 1).abs().max()) <= TWIN_ROW_SUM
                elif twin or ordinary:
                    fok = ferr <= (TOL_ORACLE if twin else TOL_FAC)
                else:
                    fok = C.prob_gate(fg, fac32[i], fac64[i], PROB_SLACK[case["precision"]])
                line += f" | {err / max(scale, 1e-300):.1e} of {scale:.1e}, fac {ferr:.1e}"
                if not (bool(torch.isfinite(x).all()) and err <= tol):
                    bad.append(f"{name} scene {b} (x{m:g}) module {i}: features {err:.3e} > {tol:.3e} (max|ref| {scale:.3e})")
                if not (bool(torch.isfinite(fg).all()) and fok):
                    bad.append(f"{name} scene {b} (x{m:g}) module {i}: factors {ferr:.3e}")
            print(line)
            if twin and not ordinary and n_det == 0:
                bad.append(f"{name} scene {b} (x{m:g}): no edge of any module is determined: the edge head is unchecked")
        if twin:
            print(f"   {name:>10} near-tie rows {unsafe}/{total}")
        if unsafe > MAX_NEAR_TIE * total:
            bad.append(f"{name}: {unsafe} of {total} incidence rows left out as near-ties")
        return bad


@pytest.fixture
def runner(monkeypatch):
    made = []

    def make(case, training=False):
        made.append(Runner(case, monkeypatch, training))
        return made[-1]
    yield make
    for r in made:
        r.close()


def _same_scene(a, ia, b, ib):
    """Scene ia of run a and scene ib of run b: features, every module's factors, every incidence, bit for bit."""
    return (torch.equal(a["out"][ia], b["out"][ib]) and torch.equal(a["H"][ia], b["H"][ib])
            and all(torch.equal(x[ia], y[ib]) for x, y in zip(a["facs"], b["facs"])))


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_permuting_the_scenes_permutes_the_results_bit_for_bit(case, runner):
    """Test A.  Every output is bit-equivariant: no output of any case needed a tolerance."""
    run = runner(case)
    B = case["B"]
    base = run.forward(run.h0, run.U)
    assert len(base["facs"]) == 1 + len(case["scales"]) and bool(torch.isfinite(base["out"]).all())
    # the forward took the route the case's id names (the CPU file holds `case_route` against the table)
    check_follows(base["raw"], C.case_route(case), ["pair"] + [C.n_edges(case["N"], s) for s in case["scales"]], case["N"],
                  nmp=case["nmp"])
    for what, p in (("derangement", C.derangement(B, case["seed"])), ("reversal", torch.arange(B - 1, -1, -1))):
        perm = run.forward(run.h0[p].contiguous(), C.take(run.U, p))
        assert perm["sig"] == base["sig"], f"{what}: the same B took other launches or plans"
        for i, b in enumerate(p.tolist()):
            assert torch.equal(perm["out"][i], base["out"][b]), f"{what}: features of scene {b} at position {i}"
            assert torch.equal(perm["H"][i], base["H"][b]), f"{what}: incidence of scene {b} at position {i}"
            for k, (x, y) in enumerate(zip(perm["facs"], base["facs"])):
                assert torch.equal(x[i], y[b]), f"{what}: factors of module {k}, scene {b} at position {i}"


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_every_scene_of_a_mixed_batch_matches_its_own_oracle(case, runner):
    """Test B."""
    run = runner(case)
    B = case["B"]
    votes = not run.twin and case["precision"] == "f16x3"
    many = dict(C.batches(B))
    if votes:
        many.update(C.zero_neighbour_batches(B))
    print(f"\n{case['id']}: per scene and module, features err / max|ref| of max|ref|, factors abs err")
    got, bad = {}, []
    for name, mags in many.items():
        h = C.scaled(case, run.h0, mags)
        got[name] = run.forward(h, run.U)
        assert got[name]["sig"] == got["ordinary"]["sig"], f"{name}: the same B took other launches or plans"
        bad += run.gate(name, h, mags, got[name])
    # cross-batch identity wherever no workgroup votes: of every checked scene, the large ones included (f16x3: the
    # batches hold ordinary and all-zero scenes only)
    free = list(many) if not votes else ["ordinary", *C.zero_neighbour_batches(B)]
    first, pairs = {}, 0
    for name in free:
        for b in C.checked(many[name]):
            m = many[name][b]
            if (b, m) not in first:
                first[(b, m)] = name
            elif not _same_scene(got[first[(b, m)]], b, got[name], b):
                bad.append(f"scene {b} (x{m:g}) differs between the batches {first[(b, m)]} and {name}")
            else:
                pairs += 1
    print(f"   {pairs} scene pairs bit-identical across {len(free)} batches")
    assert pairs >= B - 2
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", C.TRAIN_CASES, ids=[c["id"] for c in C.TRAIN_CASES])
def test_training_in_a_mixed_batch_keeps_scenes_apart(case, runner):
    """Test C.  N = 11: loss on the clean ordinary scenes at TOL_CLEAN, then on every ordinary scene at TOL_ANY.
    N = 50: the f and hyper columns of the hyper-clean ordinary scenes at TOL_CLEAN, the pairwise columns of every
    ordinary scene at TOL_ANY (a pairwise module of N = 50 is never clean)."""
    run = runner(case, training=True)
    B, N, scales = case["B"], case["N"], case["scales"]
    mags = C.train_mags(B)
    f = C.scaled(case, run.h0, mags)
    ordinary = torch.tensor([b for b, m in enumerate(mags) if m == 1.0])
    clean = C.train_clean_scenes(case)
    assert len(clean) >= case["min_clean"], clean
    print(f"\n{case['id']}: magnitudes {mags}, clean ordinary scenes {clean.tolist()}")
    got = run.forward(f, run.U, grad=True)
    bad = run.gate("train", f, mags, got, scenes=ordinary.tolist())
    assert not bad, "\n".join(bad)
    small = N <= 16
    # (_backward asserts dL/df of every scene without loss exactly zero and the loss scenes' incidence)
    eh, worst, where, n = _backward(run.blk, run.sp, run.shs, scales, f, run.U, clean, small, True, None)
    print(f"   loss on the clean scenes{'' if small else ' (f and hyper columns)'}: dL/df {eh:.1e}, worst parameter "
          f"{worst:.1e} ({where}), {n} parameters (gate {TOL_CLEAN:g})")
    assert eh <= TOL_CLEAN and worst <= TOL_CLEAN, (eh, worst, where)
    eh2, worst2, where2, n2 = _backward(run.blk, run.sp, run.shs, scales, f, run.U, ordinary, True, small, None if small else 2)
    print(f"   loss on every ordinary scene{'' if small else ' (pairwise columns)'}: dL/df {eh2:.1e}, worst parameter "
          f"{worst2:.1e} ({where2}), {n2} parameters (gate {TOL_ANY:g})")
    assert eh2 <= TOL_ANY and worst2 <= TOL_ANY, (eh2, worst2, where2)
