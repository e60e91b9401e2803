"""Test helper: the cases, references and per-scene oracle of the ragged-training tests (tests/test_ragged_backward_cpu.py
pins them, tests/test_ragged_backward_gpu.py runs them).  Pure torch on the CPU; the library is never loaded.

Kernel reference (gn_node2edge_bwd_ragged[_grouped]_f32).  Scene b of a padded batch holds n_b agents; its pooling is the
full-batch pooling of the scene ALONE at size n_b: the softmax of a hyperedge runs over n_b nodes.  So the expected
buffers are `backward_kernel_refs.n2e_grads` on the scene's slice — x', pq and H cut to n_b node rows / columns, the
pairwise incidence of n_b nodes with dedges gathered at the PADDED rows of the valid pairs — scene by scene, in float64
(the reference) and in float32 (the yardstick of `backward_kernel_refs.gate`).  Inputs follow that helper's rules: pq on
the dyadic grid k/64 in [-2, 2], H in {0, 1, 2, 0.5}, so no ReLU decision depends on rounding.  Padded rows of x', pq
carry finite garbage (N(0,1) x 100, pq on its grid x 64) that nothing may read into a valid value.

The seeded flaws are evaluated by a second, independent statement of the counted softmax (`node2edge_counted`'s: the
non-member term (n_b - members) exp(0 - max), the 0 in the maximum iff a non-member exists), on the padded scene:
  * "N_for_nb": N - members non-members;
  * "zero_in_max": the 0 enters the maximum also where no non-member exists.  The softmax is shift-invariant, so this is
    a flaw of fp32 ARITHMETIC only — exp(z - 0) underflows where every logit of a full row lies far below zero — and is
    evaluated in float32: the "one" case has its logits at -256 (exactly: w2 on the grid k/16, b2 = -256), where the
    flawed kernel divides 0 by 0;
  * "invalid_pair": every pair of the padded pairwise graph is walked.

Module oracle.  Per scene, the CPU oracle on h[b:b+1, :n_b] under torch autograd, the scene's noise gathered at the
padded indices; loss = <node_feat, R1> + <factors, R2> over valid positions, R1 / R2 drawn over the whole padded tensors;
parameter gradients summed over the scenes, the gradient of h zero at padded rows by construction."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

import backward_kernel_refs as R
import ragged_cases as C
from launch_forms import state64
from oracle import ms_hgnn_oracle as O
from ragged_size_cases import node2edge_counted      # noqa: F401  (the counted softmax this helper restates; pinned in the CPU test)
from relu_probe import relu_probe

F64, F32 = R.F64, R.F32
FLAWS = ("N_for_nb", "zero_in_max", "invalid_pair")
FLAW_FACTOR = 100.0


@dataclass(frozen=True)
class Case:
    name: str
    N: int
    counts: Tuple[int, ...]
    E: int
    kind: str                   # "hyper" | "one" | "ordered" | "sym"
    zero_scene: int = -1        # this scene's dedges are 0
    w2_scale: float = 0.25
    seed: int = 0

    @property
    def B(self) -> int:
        return len(self.counts)


KERNEL_CASES = [
    Case("hyper_e11", 11, (11, 5, 1, 0), 11, "hyper", zero_scene=0, seed=1),
    Case("one_allones", 11, (11, 5, 1, 0), 1, "one", seed=2),
    Case("ordered", 5, (5, 2, 1), 25, "ordered", seed=3),
    Case("sym", 5, (5, 2, 1), 15, "sym", seed=4),
    Case("big_lds", 140, (140, 3), 20, "hyper", w2_scale=1 / 16, seed=5),
]
GROUPED = [
    Case("grp_sym", 11, (11, 4, 1), 66, "sym", seed=11),
    Case("grp_hyper", 11, (11, 4, 1), 11, "hyper", seed=12),
    Case("grp_one", 11, (11, 4, 1), 1, "one", seed=13),
]
LDS_LIMIT_N = 140       # route.N2E_BWD_SCENE_MAX_N; N = 141 is refused


def scene_lds(N: int) -> int:
    return (4 * N * 64 + 64 + 16 * N) * 4


def pair_rows(N: int, n: int, sym: bool) -> torch.Tensor:
    """The padded rows of the valid pairs (i, j < n) of a scene, in the order `R.pair_incidence(n, sym)` lists them."""
    if not sym:
        return C.pair_index(N, n)
    return torch.tensor([i * N - (i * (i - 1)) // 2 + (j - i) for i in range(n) for j in range(i, n)], dtype=torch.long)


def _hyper_H(case: Case, g: torch.Generator) -> torch.Tensor:
    """Rows e < n_b over the columns < n_b: row 0 with exactly n_b members (no non-member), row 1 (where it exists) with
    one member, the others with 2 .. n_b - 1 members (at most 16), weights in {1, 2, 0.5}; rows e >= n_b and columns
    n >= n_b zero.  E != N (big_lds): every row is valid, as the single row of a scale-N module is."""
    B, N, E = case.B, case.N, case.E
    H = torch.zeros(B, E, N)
    wts = torch.tensor([1.0, 2.0, 0.5])
    for b, n in enumerate(case.counts):
        for e in range(E if E != N else n):
            cnt = n if e == 0 else 1 if e == 1 else int(torch.randint(2, max(3, min(n, 17)), (1,), generator=g))
            cnt = min(cnt, n)
            idx = torch.randperm(n, generator=g)[:cnt]
            H[b, e, idx] = wts[torch.randint(0, 3, (cnt,), generator=g)]
    return H


@functools.lru_cache(maxsize=None)
def kernel_inputs(case: Case) -> Dict[str, torch.Tensor]:
    """fp32 CPU tensors of a case at its PADDED shapes (H is the explicit incidence of the valid part also where the
    kernel gets H == NULL: (B, E, N) with E the padded row count, invalid pair rows zero)."""
    g = torch.Generator().manual_seed(7000 + case.seed)
    B, N, E = case.B, case.N, case.E
    Rn = lambda *s: torch.randn(*s, generator=g)
    if case.kind == "hyper":
        H = _hyper_H(case, g)
    elif case.kind == "one":
        H = torch.zeros(B, 1, N)
        for b, n in enumerate(case.counts):
            H[b, 0, :n] = 1.0
    else:
        sym = case.kind == "sym"
        H = torch.zeros(B, E, N)
        for b, n in enumerate(case.counts):
            if n:
                H[b, pair_rows(N, n, sym), :n] = R.pair_incidence(n, sym)
    assert tuple(H.shape) == (B, E, N)
    pq = torch.randint(-128, 129, (B, N, 64), generator=g).float() / 64
    xp = Rn(B, N, 64)
    for b, n in enumerate(case.counts):         # finite garbage in the padded node rows
        xp[b, n:] *= 100.0
        pq[b, n:] *= 64.0
    dedges = Rn(B, E, 64)                       # non-zero at invalid rows too: nothing may read them
    if case.zero_scene >= 0:
        dedges[case.zero_scene] = 0
    if case.kind == "one":      # exact logits far below zero: w2 on the grid k/16, b2 = -256 (module docstring)
        w2, b2 = torch.randint(-4, 5, (32,), generator=g).float() / 16, torch.tensor([-256.0])
    else:
        w2, b2 = Rn(32) * case.w2_scale, Rn(1)
    return dict(xp=xp, pq=pq, H=H, w2=w2, b2=b2, dedges=dedges, dxp0=Rn(B, N, 64), dpq0=Rn(B, N, 64), dw20=Rn(32),
                db20=Rn(1))


def scene_slice(case: Case, inp: Dict[str, torch.Tensor], b: int) -> Dict[str, torch.Tensor]:
    """Scene b alone at its own size n_b, as `R.n2e_grads` takes it (the sums dw2 / db2 start from zero)."""
    N, n = case.N, case.counts[b]
    if case.kind in ("ordered", "sym"):
        sym = case.kind == "sym"
        rows = pair_rows(N, n, sym)
        H = R.pair_incidence(n, sym)[None]
        dedges = inp["dedges"][b:b + 1, rows]
    else:
        keep = torch.arange(case.E) if case.E != N else torch.arange(n)
        H, dedges = inp["H"][b:b + 1, keep, :n], inp["dedges"][b:b + 1, keep]
    return dict(xp=inp["xp"][b:b + 1, :n], pq=inp["pq"][b:b + 1, :n], H=H, w2=inp["w2"], b2=inp["b2"], dedges=dedges,
                dxp0=inp["dxp0"][b:b + 1, :n], dpq0=inp["dpq0"][b:b + 1, :n], dw20=torch.zeros(32), db20=torch.zeros(1))


def _abs_terms(sl: Dict[str, torch.Tensor], dtype) -> torch.Tensor:
    """(32,) sum of |datt * act| of a scene slice: what `R.n2e_grads` folds into its scalar dw2_scale, per element."""
    c = lambda k: sl[k].to(dtype)
    H = c("H")
    b2 = c("b2").reshape(1, 1, 1).expand(*H.shape).clone().requires_grad_(True)
    keep: dict = {}
    edges = R.n2e_ref(c("xp"), c("pq"), H, c("w2"), b2, None, keep)
    datt, = torch.autograd.grad((edges * c("dedges")).sum(), (b2,))
    return (datt[..., None] * keep["act"]).abs().sum(dim=(0, 1, 2))


def kernel_grads(case: Case, dtype, inp: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """Expected contents of the four in-out buffers after the ragged launch, evaluated in `dtype`, with the scales of the
    two sums as `R.n2e_grads` defines them (absolute-term sums over EVERY scene, the start value one more term).
    ``inp``: other tensors than the case's own (the CPU pin substitutes pq)."""
    inp = kernel_inputs(case) if inp is None else inp
    c = lambda k: inp[k].to(dtype)
    out = dict(dxp=c("dxp0").clone(), dpq=c("dpq0").clone(), dw2=c("dw20").clone(), db2=c("db20").clone())
    dw2_abs, db2_abs = c("dw20").abs(), float(c("db20").abs().sum())
    for b, n in enumerate(case.counts):
        if n == 0:
            continue
        sl = scene_slice(case, inp, b)
        r = R.n2e_grads(sl, dtype)
        out["dxp"][b, :n], out["dpq"][b, :n] = r["dxp"][0], r["dpq"][0]
        out["dw2"] += r["dw2"]
        out["db2"] += r["db2"]
        dw2_abs = dw2_abs + _abs_terms(sl, dtype)
        db2_abs += r["db2_scale"]
    out["dw2_scale"], out["db2_scale"] = float(dw2_abs.max()), db2_abs
    return out


@functools.lru_cache(maxsize=None)
def kernel_expected(case: Case):
    return kernel_grads(case, F64), kernel_grads(case, F32)


def kernel_gate(case: Case, out: str, ceiling: float):
    """(bound, e32, scale, ref64) of one output: `R.gate`, capped at `ceiling` of the scale (TOL_CLEAN)."""
    r64, r32 = kernel_expected(case)
    scale = R.n2e_scale(r64, out)
    bound, e32 = R.gate(r64[out], r32[out], scale)
    return min(bound, ceiling * scale), e32, scale, r64[out]


# ---------------------------------------------------------------------------------------------------------------------
# the second statement of the counted softmax, with the flaws
# ---------------------------------------------------------------------------------------------------------------------
def counted_pool(xp, pq, H, w2, b2, n: int, flaw: Optional[str] = None, keep: Optional[dict] = None):
    """Pooled edges (E, 64) of ONE padded scene: x', pq (N, 64), H (E, N) with members only at columns < n (rows without
    members pool nothing), the softmax over n nodes.  b2: scalar or (E, N)."""
    N = xp.shape[0]
    P, Qn = pq[:, :32], pq[:, 32:]
    pre = P[None, :, :] + (H @ Qn)[:, None, :]
    act = torch.relu(pre)
    att = act @ w2 + b2
    if keep is not None:
        keep["act"] = act.detach()
    member = H != 0
    cnt = member.sum(-1)
    others = ((N if flaw == "N_for_nb" else n) - cnt).clamp(min=0).to(xp.dtype)
    v = (att * H).masked_fill(~member, float("-inf"))
    mx = v.amax(dim=-1)
    zero_in = (others > 0) | (cnt == 0) if flaw != "zero_in_max" else torch.ones_like(cnt, dtype=torch.bool)
    mx = torch.where(zero_in, mx.clamp(min=0), mx)
    ex = torch.exp(v - mx[:, None])
    total = ex.sum(-1) + others * torch.exp(-mx)
    total = torch.where(cnt == 0, torch.ones_like(total), total)      # (an empty row: ex is all zero)
    return (ex / total[:, None] * H) @ xp


def counted_grads(case: Case, dtype, flaw: Optional[str] = None) -> Dict[str, torch.Tensor]:
    """The four buffers by `counted_pool`, scene by scene on the PADDED tensors."""
    inp = kernel_inputs(case)
    c = lambda k: inp[k].to(dtype)
    out = dict(dxp=c("dxp0").clone(), dpq=c("dpq0").clone(), dw2=c("dw20").clone(), db2=c("db20").clone())
    N = case.N
    for b, n in enumerate(case.counts):
        if n == 0:
            continue
        H = c("H")[b]
        if flaw == "invalid_pair" and case.kind in ("ordered", "sym"):
            H = R.pair_incidence(N, case.kind == "sym", dtype=dtype)
        xp, pq = c("xp")[b].clone().requires_grad_(True), c("pq")[b].clone().requires_grad_(True)
        b2 = c("b2").reshape(1, 1).expand(*H.shape).clone().requires_grad_(True)
        keep: dict = {}
        edges = counted_pool(xp, pq, H, c("w2"), b2, n, flaw, keep)
        dxp, dpq, datt = torch.autograd.grad((edges * c("dedges")[b]).sum(), (xp, pq, b2))
        out["dxp"][b] += dxp
        out["dpq"][b] += dpq
        out["dw2"] += (datt[..., None] * keep["act"]).sum(dim=(0, 1))
        out["db2"] += datt.sum().reshape(1)
    return out


def flaw_moves(case: Case, flaw: str, ceiling: float) -> Dict[str, float]:
    """Per output, |flawed - ref64| in units of the output's gate (inf where the flawed value is not finite).  The
    arithmetic flaw is evaluated in float32, the others in float64."""
    bad = counted_grads(case, F32 if flaw == "zero_in_max" else F64, flaw)
    moves = {}
    for o in R.N2E_OUTPUTS:
        bound, _, _, ref = kernel_gate(case, o, ceiling)
        d = (bad[o].double() - ref).abs()
        moves[o] = float("inf") if not bool(torch.isfinite(d).all()) else float(d.max()) / bound
    return moves


# ---------------------------------------------------------------------------------------------------------------------
# the module oracle
# ---------------------------------------------------------------------------------------------------------------------
def module_case(N: int, counts, scales=(), seed: int = 0, redraw: int = 0) -> Dict:
    """A `ragged_cases`-style case for whole modules (its `inputs`, `with_garbage`, `min_gap` take it)."""
    return dict(id=f"n{N}_{'_'.join(map(str, counts))}", N=N, counts=list(counts), B=len(counts), scales=list(scales),
                seed=seed + 1000 * redraw, what="ragged training")


def settled_case(N: int, counts, scales=(), seed: int = 0, nmp: int = 1) -> Dict:
    """`module_case`, redrawn (deterministically) until every top-k gap of a valid row is at least `C.MIN_GAP`."""
    for redraw in range(64):
        case = module_case(N, counts, scales, seed, redraw)
        if C.min_gap(case, C.inputs(case, nmp)[0]) >= C.MIN_GAP:
            return case
    raise AssertionError("no draw with the affinity gaps the cases need")


def valid_factor_rows(N: int, n: int, E: int, pairwise: bool) -> torch.Tensor:
    """The rows of a module's padded `factors` that are valid for a scene of n agents."""
    if pairwise:
        return C.pair_index(N, n)
    return torch.arange(1 if E == 1 else n)


def scene_module_grads(state, pairwise: bool, scale: Optional[int], N: int, n: int, hb: torch.Tensor, noise,
                       R1b: torch.Tensor, R2b: torch.Tensor, nmp: int = 1):
    """One module on ONE scene alone (hb (1, n, 64), its noise at the valid edges) in float64 under autograd, loss
    <node_feat, R1b[:n]> + <factors, R2b[valid rows]> -> (node_feat (n, .), factors, d hb (n, 64), parameter gradients by
    name (None: unused), clean: no ReLU input within the rounding window of zero, H or None)."""
    st = state64(state, requires_grad=True)
    x = hb.double().clone().requires_grad_(True)
    nz = [u.double() for u in noise]
    with relu_probe(1) as probe:
        if pairwise:
            H = None
            nf, fac = O.ms_hgnn_pairwise_forward(st, x, nz, nmp, decomposed=True)
        else:
            H = C.scene_incidence(C.scene_corr(hb.float(), 0, n), scale, N)
            nf, fac = O._message_passing(st, x, H.double(), nz, nmp, True, None)
    rows = valid_factor_rows(N, n, fac.shape[1], pairwise)
    ((nf[0] * R1b[:n].double()).sum() + (fac[0] * R2b[rows].double()).sum()).backward()
    return nf[0].detach(), fac[0].detach(), x.grad[0], {k: v.grad for k, v in st.items()}, bool(probe.clean()[0]), H


def module_oracle(state, pairwise: bool, scale: Optional[int], case: Dict, h: torch.Tensor, U_mod: List[torch.Tensor],
                  R1: torch.Tensor, R2: torch.Tensor, nmp: int = 1, scenes=None):
    """The per-scene oracle of one module over (a subset of) a ragged batch -> dict(node_feat (B,N,.) and factors at
    their padded shapes, zeros at padded positions; g_h (B,N,64), zero at padded rows by construction; grads by name,
    summed over the scenes; clean (B,) bool)."""
    N = case["N"]
    scenes = list(range(case["B"])) if scenes is None else list(scenes)
    nf_all = torch.zeros(case["B"], N, R1.shape[-1], dtype=F64)
    fac_all = torch.zeros(*R2.shape, dtype=F64)
    g_h = torch.zeros(case["B"], N, 64, dtype=F64)
    grads: Dict[str, Optional[torch.Tensor]] = {}
    clean = torch.zeros(case["B"], dtype=torch.bool)
    for b in scenes:
        n = case["counts"][b]
        noise = C.scene_noise(U_mod, b, N, n, pairwise)
        nf, fac, gx, gp, ok, _ = scene_module_grads(state, pairwise, scale, N, n, h[b:b + 1, :n], noise, R1[b], R2[b], nmp)
        nf_all[b, :n], g_h[b, :n], clean[b] = nf, gx, ok
        fac_all[b, valid_factor_rows(N, n, fac_all.shape[1], pairwise)] = fac
        for k, v in gp.items():
            if v is not None:
                grads[k] = v.clone() if grads.get(k) is None else grads[k] + v
            else:
                grads.setdefault(k, None)
    return dict(node_feat=nf_all, factors=fac_all, g_h=g_h, grads=grads, clean=clean)
