"""Test helper: the bottleneck width — the output width `dout` of the closing MLP nmp_mlp_end (128 -> 128 -> bottleneck_dim)
— as a dimension of the hot path (no GPU needed to import).

The reference's default is 1024 and INTEGRATION.md calls the width free; the launchers branch on it: the 16-bit-core image
exists up to 64 (weights.closing_mlp) and the plain fp32-core kernel runs beyond it, the bf16-core kernels are
instantiated with one 32-wide output tile up to 32 and with two above, the closing stage fused into the aggregation
launch exists for 33..64 only, every store has a vector and an element branch by `(dout | ldy) & 3`, bf16 storage ends at
64, and the backward's GEMMs take dout as their K or N.  This module holds what the tests of the width share:

  * the width tables;
  * inputs drawn on the CPU from seeds of their own and plain-torch references that take `dtype`:
    y = W1 relu(W0 x + b0) + b1 with x given or x = cat(H^T feat, ori) / N, and whole modules on oracle.ms_hgnn_oracle;
  * the choice of every case's inputs ON THE REFERENCES ALONE: the first of 16 seeded draws on which the fp32 CPU reference
    stays within a third of the fp32 gate (bf16 storage: on which four times the bf16 restatement's error stays within the
    cap) — tests/test_bottleneck_cpu.py runs every search without a GPU;
  * the gates (module docstring of tests/test_bottleneck_gpu.py).
"""
from __future__ import annotations

import contextlib
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from edge_type_cases import abs_err, cast, dead_parameters, engine_inputs, engine_ref, pair_index, rel_err, state_of
from launch_forms import IMAGE_MAX_DOUT, ONE_TILE_MAX_DOUT, expected_forms, mlp2_form, pair_count, sample_scenes
from oracle import ms_hgnn_oracle as O

D_ALL = tuple(range(1, 65))
# the tile edge (32 | 33), the vector / element store edge (multiples of 4 and not), the image edge (64 | 65) and ragged
# widths on both sides of each
D_EDGES = (1, 3, 4, 31, 32, 33, 36, 40, 63, 64, 65, 68, 96, 100, 129)
D_WIDE = tuple(d for d in D_EDGES if d > IMAGE_MAX_DOUT)
D_IMAGE = tuple(d for d in D_EDGES if d <= IMAGE_MAX_DOUT)
ROWS = 69                               # two full 32-row blocks and a ragged one
PATHS = ("f16x3", "bf16x6", "fp32")     # the matrix paths of the fp32 entry points

TOL_FEAT = 2e-6          # of max|ref64|: tests/test_launch_forms_gpu.py TOL_FEAT, the typed-stage gate of the edge-type tests
TOL_FAC = 5e-6           # absolute (factors are probabilities): ... TOL_FAC
BF16_MARGIN = 4.0        # bf16 storage: max|hip - ref64| <= 4 e_emu, the project's margin over a reference's own error
BF16_CAP = 1.5e-2        # ... and 4 e_emu within this share of max|ref64| (the bar of the twins)
DRAWS = 16
WIDTH_CLASSES = ("<=32", "33..64", ">64")


def _gen(*key: int) -> torch.Generator:
    """A generator seeded by the key (a polynomial in 1009, modulo 2^61 - 1: a key of any length stays a valid seed)."""
    seed = 0
    for k in key:
        seed = (seed * 1009 + int(k)) % ((1 << 61) - 1)
    return torch.Generator().manual_seed(seed)


def width_class(d: int) -> str:
    return WIDTH_CLASSES[0] if d <= ONE_TILE_MAX_DOUT else (WIDTH_CLASSES[1] if d <= IMAGE_MAX_DOUT else WIDTH_CLASSES[2])


def bf16r(t: torch.Tensor) -> torch.Tensor:
    """t rounded to bf16, in t's dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the closing MLP alone
# ---------------------------------------------------------------------------------------------------------------------
# input forms, (kind, B, N, scale): "x": a tensor of ROWS rows (N: its width din); "sym": ScatterSpec over the unordered
# pairs of the pairwise graph; "hyper": ScatterSpec with a top-k H of `scale` members (E = N, or 1 at scale = N — and
# E = 20 > 16, which only mlp2_x_kernel takes); "nodeagg": NodeAggSpec
Form = Tuple[str, int, int, int]
X_FORM: Form = ("x", 0, 128, 0)
INPUT_FORMS: Tuple[Form, ...] = (("sym", 3, 5, 0), ("sym", 3, 11, 0), ("hyper", 3, 11, 3), ("hyper", 3, 11, 11),
                                 ("hyper", 3, 20, 5), ("nodeagg", 3, 11, 0))
TWO_GROUPS: Tuple[Form, Form] = (("sym", 3, 11, 0), ("hyper", 3, 11, 3))      # two groups in one launch (they share B, N)
PLACEMENT_D = (1, 3, 4, 33, 36, 40, 64)
OTHER_WIDTHS = ((64, 128), (64, 256), (128, 256))       # (din, dh): the other instantiations of the C ABI
OTHER_D = (7, 32, 40, 64)
FLAWS = ("bias2", "noN", "swap", "untransposed")


def form_id(form: Form) -> str:
    kind, B, N, s = form
    return f"x{N}" if kind == "x" else f"{kind}-N{N}" + (f"-s{s}" if s else "")


def form_rows(form: Form) -> int:
    return ROWS if form[0] == "x" else form[1] * form[2]


def form_edges(form: Form) -> int:
    """Edge rows per scene of a fused-scatter form (0: none)."""
    kind, _, N, s = form
    return pair_count(N) if kind == "sym" else ((1 if s == N else N) if kind == "hyper" else 0)


def closing_mlp(dout: int, din: int = 128, dh: int = 128, which: int = 0):
    """The MLP din -> dh -> dout on the CPU, default nn.Linear init from a seed of its widths."""
    import groupnet_amd as G
    torch.manual_seed(((7 * 1009 + din) * 1009 + dh) * 1009 + dout + 100003 * which)
    return G.MLP(din, dout, hidden_size=(dh,))


def pair_rows_incidence(N: int, dtype=torch.float64) -> torch.Tensor:
    """(N (N + 1) / 2, N): weight 1 on both nodes of an unordered pair row and on a self-loop's node (what the scatter of
    the unordered pairs forms: the pair row already holds both ordered edges)."""
    ii, jj, _ = pair_index(N)
    H = torch.zeros(ii.numel(), N, dtype=dtype)
    H[torch.arange(ii.numel()), ii] = 1
    H[torch.arange(ii.numel()), jj] = 1
    return H


def draw_source(form: Form, dout: int, draw: int, bf16: bool = False, which: int = 0) -> Dict[str, torch.Tensor]:
    """The inputs of one group: {"x"} or {"ori", "feat" | "agg"[, "H"]} (bf16-representable where asked)."""
    kind, B, N, s = form
    g = _gen(11, ("x", "sym", "hyper", "nodeagg").index(kind), B, N, s, dout, draw, which)
    rnd = lambda *shape: bf16r(torch.randn(*shape, generator=g)) if bf16 else torch.randn(*shape, generator=g)
    if kind == "x":
        return dict(x=rnd(ROWS, N))
    src = dict(ori=rnd(B, N, 64))
    if kind == "nodeagg":
        src["agg"] = rnd(B, N, 64)
        return src
    if kind == "hyper":
        src["H"] = O.topk_incidence_ranked(O.affinity(src["ori"]), s)
    src["feat"] = rnd(B, form_edges(form), 64)
    return src


def closing_input(form: Form, src: Dict[str, torch.Tensor], dtype=torch.float64, flaw: Optional[str] = None) -> torch.Tensor:
    """The MLP's input rows (rows, din): x, or cat(H^T feat, ori) / N.  flaw (tests/test_bottleneck_cpu.py): "noN" leaves
    the division out, "swap" puts ori first, "untransposed" applies H instead of H^T (where it is square)."""
    kind, B, N, _ = form
    if kind == "x":
        return src["x"].to(dtype)
    ori = src["ori"].to(dtype)
    if kind == "nodeagg":
        agg = src["agg"].to(dtype)
    else:
        H = pair_rows_incidence(N, dtype)[None].expand(B, -1, -1) if kind == "sym" else src["H"].to(dtype)
        if flaw == "untransposed" and H.shape[1] == H.shape[2]:
            agg = torch.matmul(H, src["feat"].to(dtype))
        else:
            agg = torch.matmul(H.transpose(1, 2), src["feat"].to(dtype))
    cat = torch.cat((ori, agg) if flaw == "swap" else (agg, ori), dim=-1)
    return (cat if flaw == "noN" else cat / N).reshape(B * N, 128)


def closing_ref(state: Dict[str, torch.Tensor], x: torch.Tensor, dtype=torch.float64, emulate_bf16: bool = False,
                flaw: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(y, hid) of y = W1 relu(W0 x + b0) + b1 in `dtype`, written out as products and sums.  emulate_bf16: the
    restatement of the bf16 twins — operands (x, W0, W1), the hidden activations and the result rounded to bf16, sums
    in `dtype`.  flaw "bias2": the bias of the second 32-wide output tile dropped."""
    W0, b0, W1, b1 = (state[k].to(dtype) for k in ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias"))
    x = x.to(dtype)
    if emulate_bf16:
        x, W0, W1 = bf16r(x), bf16r(W0), bf16r(W1)
    if flaw == "bias2":
        b1 = torch.cat((b1[:32], torch.zeros_like(b1[32:])))
    hid = torch.relu((x[:, None, :] * W0[None, :, :]).sum(-1) + b0)
    if emulate_bf16:
        hid = bf16r(hid)
    y = (hid[:, None, :] * W1[None, :, :]).sum(-1) + b1
    return (bf16r(y) if emulate_bf16 else y), hid


@functools.lru_cache(maxsize=None)
def closing_case(forms: Tuple[Form, ...], dout: int, bf16: bool = False, din: int = 128, dh: int = 128) -> Dict:
    """One launch of len(forms) groups at width dout -> {"mlps" (on the CPU), "states", "srcs", "x64", "hid64", "y64" (per
    group, float64), "err_ref" (the reference's own error: fp32 CPU against float64 of max|ref64| — bf16: e_emu, absolute),
    "gate" (per group, absolute, on y), "draw"}.  The inputs are the first of DRAWS seeded draws on which every group's
    reference error is within its bound: a third of TOL_FEAT (y, and the kept x and hid) on fp32 storage, 4 e_emu within
    BF16_CAP of max|ref64| on bf16 storage.  Nothing of the code under test enters the choice."""
    mlps = [closing_mlp(dout, din, dh, which=i) for i in range(len(forms))]
    states = [state_of(m) for m in mlps]
    last = None
    for draw in range(DRAWS):
        srcs = [draw_source(f if f[0] != "x" else ("x", 0, din, 0), dout, draw, bf16, which=i) for i, f in enumerate(forms)]
        x64 = [closing_input(f, s) for f, s in zip(forms, srcs)]
        out64 = [closing_ref(st, x) for st, x in zip(states, x64)]
        ok, errs, gates = True, [], []
        for f, s, st, x, (y, hid) in zip(forms, srcs, states, x64, out64):
            top = float(y.abs().max())
            if bf16:
                e = abs_err(closing_ref(st, x, emulate_bf16=True)[0], y)
                ok = ok and BF16_MARGIN * e <= BF16_CAP * top
                gates.append(BF16_MARGIN * e)
            else:
                x32 = closing_input(f, s, torch.float32)
                y32, hid32 = closing_ref(st, x32, torch.float32)
                e = rel_err(y32, y)
                ok = ok and max(e, rel_err(x32, x), rel_err(hid32, hid)) <= TOL_FEAT / 3
                gates.append(TOL_FEAT * top)
            errs.append(e)
        last = dict(mlps=mlps, states=states, srcs=srcs, x64=x64, hid64=[o[1] for o in out64], y64=[o[0] for o in out64],
                    err_ref=errs, gate=gates, draw=draw)
        if ok:
            return last
    raise AssertionError(f"no draw of {forms} dout={dout} bf16={bf16} keeps the reference's own error within its bound: {last['err_ref']}")


def closing_launch_form(forms: Sequence[Form], dout: int, precision: str, dtype: str = "fp32", xs: Optional[str] = None,
                        keep: bool = False, dh: int = 128):
    """`launch_forms.mlp2_form` of the launch of these groups: (kernel, tiles[2]) or None (refused)."""
    fused = keep or any(f[0] != "x" for f in forms)
    wide = any(f[0] == "hyper" and form_edges(f) > 16 for f in forms)
    return mlp2_form(dout, form_rows(forms[0]), len(forms), precision, dtype, fused_input=fused, wide_hyper=wide,
                     xs=None if xs is None else xs != "0", dh=dh)


# ---------------------------------------------------------------------------------------------------------------------
# 2. / 3. whole modules
# ---------------------------------------------------------------------------------------------------------------------
def pair_module(d: int, seed: int, nmp: int = 1):
    import groupnet_amd as G
    torch.manual_seed(seed)
    return G.MS_HGNN_oridinary(embedding_dim=16, h_dim=64, mlp_dim=64, bottleneck_dim=d, batch_norm=0, nmp_layers=nmp)


def hyper_module(d: int, scale: int, seed: int, nmp: int = 1):
    import groupnet_amd as G
    torch.manual_seed(seed)
    return G.MS_HGNN_hyper(embedding_dim=64, h_dim=64, mlp_dim=64, bottleneck_dim=d, batch_norm=0, nmp_layers=nmp, scale=scale)


@contextlib.contextmanager
def bf16_mlps():
    """The oracle with every MLP restated as the bf16 twins store it: inputs, weights, hidden activations and results
    rounded to bf16 (sums, softmax and the graph sums in the dtype of the call; `module_case` rounds the factors, which
    the twins store in bf16 too)."""
    real = O.mlp

    def mlp(state, prefix, x):
        n = 0
        while f"{prefix}.layers.{n}.weight" in state:
            n += 1
        x = bf16r(x)
        for i in range(n):
            x = F.linear(x, bf16r(state[f"{prefix}.layers.{i}.weight"]), state[f"{prefix}.layers.{i}.bias"])
            x = bf16r(torch.relu(x) if i != n - 1 else x)
        return x
    O.mlp = mlp
    try:
        yield
    finally:
        O.mlp = real


def _mcase(tag: str, d: int, B: int, N: int, scales: Sequence[Optional[int]], nmp: int = 1, dtype: str = "fp32") -> Tuple:
    return (tag, d, B, N, tuple(scales), nmp, dtype)


def module_case_id(case: Tuple) -> str:
    tag, d, B, N, scales, nmp, dtype = case
    return f"{tag}-d{d}-B{B}-N{N}" + (f"-nmp{nmp}" if nmp > 1 else "") + ("-bf16" if dtype == "bf16" else "")


# the latency form (fuse_closing=True) of [pairwise, hyper scale 3, hyper scale N] at N = 11: B = 7 (every hyper group below
# 128 row blocks: 4 waves per row block) and B = 400 (the scale-3 group: 138 row blocks, 2 waves; packed scenes)
FUSED_D = (16, 32, 33, 40, 63, 64, 96)
FUSED_CASES = [_mcase("latency", d, B, 11, (None, 3, 11)) for B in (7, 400) for d in FUSED_D]
# one module through its own forward: N = 5 and 11 (fused gather / scatter), N = 20 (the stand-alone scatter)
MODULE_N = (5, 11, 20)
NMP2_D = (3, 40, 100)       # two rounds: only the last closing MLP has the bottleneck width (one per width class)


def module_cases(kind: str, N: int, dtype: str = "fp32", nmp: int = 1) -> List[Tuple]:
    widths = (D_EDGES if nmp == 1 else NMP2_D) if dtype == "fp32" else (D_IMAGE if nmp == 1 else ())
    scale = None if kind == "pair" else 3
    return [_mcase(kind, d, 3, N, (scale,), nmp, dtype) for d in widths]


MODULE_KINDS = ("pair", "hyper")
ALL_MODULE_CASES = (FUSED_CASES + [c for k in MODULE_KINDS for N in MODULE_N for dt in ("fp32", "bf16") for c in module_cases(k, N, dt)]
                    + [c for k in MODULE_KINDS for c in module_cases(k, 11, nmp=2)])


def module_forms(case: Tuple) -> Dict:
    tag, d, B, N, scales, nmp, dtype = case
    return expected_forms(B, N, [s for s in scales if s is not None], "f16x3", dtype, block=tag == "latency",
                          with_pair=scales[0] is None, bottleneck=d)


@functools.lru_cache(maxsize=None)
def module_case(case: Tuple) -> Dict:
    """-> {"mods" (on the CPU), "states", "h", "Hs", "U", "scenes", "ref" ([(node_feat, factors)] per module, float64, on
    the scenes), "err_ref" ((features of max|ref64|, factors absolute) of the fp32 oracle — bf16: e_emu of both, absolute),
    "gate" ((features, factors) per module, absolute), "draw"}: the first of DRAWS seeded draws of the inputs on which the
    reference's own error is within its bound, as `closing_case`."""
    tag, d, B, N, scales, nmp, dtype = case
    twin = dtype == "bf16"
    types = tuple(6 if s is None else 10 for s in scales)
    base = 9000 + 37 * d + N + (500 if tag == "latency" else 0) + 7 * nmp
    mods = [pair_module(d, base + 31 * i, nmp) if s is None else hyper_module(d, s, base + 31 * i, nmp) for i, s in enumerate(scales)]
    states = [state_of(m) for m in mods]
    scenes = torch.arange(B) if B <= 48 else sample_scenes(B, N, module_forms(case), n=48, seed=B + N)
    last = None
    for draw in range(DRAWS):
        h, Hs, U = engine_inputs(B, N, scales, types, base + 1000 * (draw + 1), nmp, bf16=twin)
        with torch.no_grad():
            ref = engine_ref(states, h, Hs, U, scenes, nmp)
            if twin:
                with bf16_mlps():
                    other = [O._message_passing(cast(st, torch.float64), h[scenes].double(),
                                                (O.pairwise_incidence(N, len(scenes), torch.float64) if H is None else H[scenes].double()),
                                                [u[scenes].double() for u in us], nmp, False, None)
                             for st, H, us in zip(states, Hs, U)]
                other = [(nf, bf16r(fac)) for nf, fac in other]      # (the twins store the factors in bf16 as well)
            else:
                other = engine_ref(states, h, Hs, U, scenes, nmp, dtype=torch.float32)
        ok, errs, gates = True, [], []
        for (f64, c64), (fo, co) in zip(ref, other):
            top = float(f64.abs().max())
            if twin:
                ef, ec = abs_err(fo, f64), abs_err(co, c64)
                ok = ok and BF16_MARGIN * ef <= BF16_CAP * top and BF16_MARGIN * ec <= BF16_CAP
                gates.append((BF16_MARGIN * ef, BF16_MARGIN * ec))
            else:
                ef, ec = rel_err(fo, f64), abs_err(co, c64)
                ok = ok and ef <= TOL_FEAT / 3 and ec <= TOL_FAC / 3
                gates.append((TOL_FEAT * top, TOL_FAC))
            errs.append((ef, ec))
        last = dict(mods=mods, states=states, h=h, Hs=Hs, U=U, scenes=scenes, ref=ref, err_ref=errs, gate=gates, draw=draw)
        if ok:
            return last
    raise AssertionError(f"no draw of {module_case_id(case)} keeps the reference's own error within its bound: {last['err_ref']}")


# ---------------------------------------------------------------------------------------------------------------------
# 4. training
# ---------------------------------------------------------------------------------------------------------------------
BACKWARD_D = (1, 3, 32, 33, 40, 100)      # K = 1 (lda = 1) and 3 of the closing GEMMs, the tile edge, a ragged tile, no image
BACKWARD_KINDS = ("pair", "hyper3")
BACKWARD_SIZE = (4, 7)
RELU_MARGIN = 1e-7                          # as tests/edge_type_cases.py


def backward_oracle(kind: str, state, h: torch.Tensor, U: torch.Tensor, H: Optional[torch.Tensor]):
    if kind == "pair":
        return O.ms_hgnn_pairwise_forward(state, h, [U], 1, decomposed=True)
    return O._message_passing(state, h, H, [U], 1, True, None)


@functools.lru_cache(maxsize=None)
def backward_case(kind: str, d: int) -> Dict:
    """As edge_type_cases.backward_case, at bottleneck width d and the reference's edge types: a module (heads and
    attention scaled away from their flat start) and the inputs of L = <node_feat, R1> + <factors, R2> — the first of
    DRAWS seeded draws on which the float64 ORACLE has no ReLU input within RELU_MARGIN of zero and at least one clean
    scene."""
    from relu_probe import relu_probe
    B, N = BACKWARD_SIZE
    scale = None if kind == "pair" else 3
    K = 6 if kind == "pair" else 10
    mod = pair_module(d, 700 + d) if kind == "pair" else hyper_module(d, scale, 800 + d)
    with torch.no_grad():
        for name, p in mod.named_parameters():
            if "attention_mlp" in name or "MLP_distribution" in name or "MLP_factor" in name:
                p.mul_(4.0)
    state = state_of(mod)
    E = N * N if kind == "pair" else N
    for shift in range(DRAWS):
        g = _gen(12, BACKWARD_KINDS.index(kind), d, shift)
        h, U = torch.randn(B, N, 64, generator=g), torch.rand(B, E, K, generator=g)
        R1, R2 = torch.randn(B, N, d, generator=g), torch.randn(B, E, K, generator=g)
        H = None if kind == "pair" else O.topk_incidence_ranked(O.affinity(h), scale)
        with torch.no_grad(), relu_probe(B) as probe:
            backward_oracle(kind, cast(state, torch.float64), h.double(), U.double(), None if H is None else H.double())
        if float(probe.near.min()) > RELU_MARGIN and bool(probe.clean().any()):
            c = dict(mod=mod, state=state, scale=scale, h=h, U=U, R1=R1, R2=R2, shift=shift, K=K)
            c["dead"] = dead_parameters(kind, c)
            return c
    raise AssertionError(f"no draw of {kind} d={d} keeps the oracle's ReLU inputs away from zero")
