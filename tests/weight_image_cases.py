"""Test helper: the range flag behind the two-part fp16 weight images, at every kernel that reads it (no GPU needed to
import).

The f16x3 path walks a two-part fp16 image of each weight set; one flag word sits behind every image.  The split
(gn_split_bf16_f32, parts = 2) raises it when a weight is not |w| <= 65000, every kernel reads it through
`image_flag(image, substeps)` — the word's offset is recomputed at each call site from that kernel's own count of
sub-steps — and a flagged workgroup repeats its rows on the bf16x6 path.  A wrong offset fails silently either way: read
past the image an out-of-range weight is missed (inf / NaN), read inside it the launch always falls back (right, slow).
This module holds what tests/test_weight_images_cpu.py and tests/test_weight_images_gpu.py share:

  * `CALL_SITES`: the `image_flag(` call sites of gn_mlp_bf16.hpp by their argument text;
  * `SITES`: one entry per image and kernel form that reads a flag — packer, image name, the nn.Linear weights that feed
    the image, the stand-alone `ops` call that runs exactly that kernel, the switches that force the form;
  * per site the modules, the inputs (seeded draws on the CPU) and the references (oracle.ms_hgnn_oracle or the plain
    torch restatements of bottleneck_cases, in the dtype asked for);
  * `case(site, pos, value)`: one weight of one source matrix of the image set to `value` — the first of DRAWS seeded
    draws on which the fp32 CPU reference stays within a third of the gate against float64 (nothing of the code under
    test enters the choice; the CPU file runs every search).

Magnitudes: the operand the large weight multiplies is scaled by 1 / |w| — the input column for a first-layer weight
(the producing layer's output unit where the kernel forms its input rows itself), the hidden unit (row and bias of the
first layer) for a second-layer weight — so the product is O(1), everything downstream is ordinary and the gates mean
something.  Every weight but the one stays in range.  (65000.0 exactly does NOT flag and runs on the fp16 path, where an
operand of 1.5e-5 is an fp16 subnormal with an absolute error of 2^-25 (gn_mlp_bf16.hpp, header): times 65000 that is
2e-3 of an O(1) result.  That case is therefore held to the flag, to finiteness and to having run the fp16 path; its
distance from float64 is printed, not gated.)
"""
from __future__ import annotations

import functools
import math
import zlib
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

import bottleneck_cases as BC
import edge_type_cases as EC
from edge_type_cases import abs_err, cast, pair_index, rel_err, state_of
from launch_forms import pair_count
from oracle import ms_hgnn_oracle as O

FLAG_LIMIT = 65000.0          # gn_mlp_mfma.hip split_bf16_image: `if (!(fabsf(x) <= 65000.f))`
# (the value written, whether the split must raise the flag): 65001 flags although fp16 holds it; NaN flags too (LIFE_VALUES)
WEIGHT_VALUES: Tuple[Tuple[float, bool], ...] = ((7.0e4, True), (-7.0e4, True), (math.inf, True), (65000.0, False), (65001.0, True))
LIFE_VALUES: Tuple[Tuple[float, bool], ...] = ((7.0e4, True), (math.nan, True))
TOL_FEAT = BC.TOL_FEAT        # of max|ref64|, no floor
PROB_FLOOR = 1e-4             # scene_isolation_cases.prob_gate: slack x max(1e-4, 3 x the fp32 oracle's own distance)
DRAWS = BC.DRAWS
B = 3
PROB_OUTPUTS = ("ef", "dist")           # outputs gated as probabilities; every other output is a feature

# `image_flag(` call sites of groupnet_amd/csrc/gn_mlp_bf16.hpp: argument text -> the name SITES uses
CALL_SITES: Dict[str, str] = {
    "img, 72": "node-chain",
    "imgA, OTA * 4": "node-W1cat",
    "img, 80": "edge",
    "image, 48": "closing-stream",
    "img, pair_form ? K * 16 : K * 32": "typed-agg",
    "img, kSub": "mlp2_x",
    "image, HT * (NA + NB)": "mlp2_xs",
}
W1CAT_K = (1, 4, 5, 12)                  # the node form ends at K = 12
AGG_K = (1, 4, 5, 8, 13, 16)
AGG_FORMS = {"eo": ("eo", B, 0, 23), "gather": ("gather", B, 11, 3), "pair": ("pair", B, 11, 0), "pair-node": ("pair-node", B, 11, 0)}
FUSED_D = (33, 64)
MLP2_D = (4, 32, 33, 64)
MLP2_OTHER_D = (7, 40)                   # one and two output tiles at the other (din, dh)
MLP2_FORMS: Tuple[BC.Form, ...] = (BC.X_FORM, ("sym", B, 11, 0), ("hyper", B, 11, 3))
MLP2_KERNELS = {"0": "mlp2_x_kernel", "1": "mlp2_xs_kernel"}       # GN_MLP2_XS -> kernel


class Site(NamedTuple):
    id: str
    call_site: str                   # a value of CALL_SITES
    packer: str                      # the layout of groupnet_amd.weights that builds the image
    image: str                       # its name in XImages.src
    feeds: Tuple[str, ...]           # the nn.Linear weights that feed the image, in image order
    ops_call: str                    # the stand-alone ops call that runs exactly that kernel
    switches: Tuple[Tuple[str, str], ...]      # environment switches that force the form
    kind: str
    p: Tuple[Tuple[str, object], ...]          # the kind's parameters

    def __getitem__(self, k):        # site["K"]
        return dict(self.p)[k] if isinstance(k, str) else tuple.__getitem__(self, k)

    def substeps(self) -> int:
        """Sub-steps of the image = where its kernel looks for the flag word (the `Depends on` column of the issue)."""
        q = dict(self.p)
        if self.image == "chain":
            return 72
        if self.image == "edge":
            return 80
        if self.image == "W1cat":
            return 4 * q["K"] * 4
        if self.image == "W2t":
            return q["K"] * 16
        if self.image == "W12":
            return q["K"] * 32
        din, dh, dout = q.get("din", 128), q.get("dh", 128), q["dout"]
        return (dh // 32) * (2 * (din // 32) + 2 * ((dout + 31) // 32))


def _site(id, call_site, packer, image, feeds, ops_call, kind, switches=(), **p) -> Site:
    return Site(id, call_site, packer, image, tuple(feeds), ops_call, tuple(switches), kind, tuple(sorted(p.items())))


_CHAIN = ("node2edge_start_mlp.0.layers.0", "node2edge_start_mlp.0.layers.1", "attention_mlp.0.layers.0")
_EDGE = ("init_MLP.layers.0", "init_MLP.layers.1", "MLP_distribution.layers.0", "MLP_factor.layers.0",
         "MLP_distribution.layers.1", "MLP_factor.layers.1")
_MLP2 = ("layers.0", "layers.1")


def _sites() -> List[Site]:
    s = []
    for m, N in (("pair", 5), ("hyper", 11)):
        s.append(_site(f"node-{m}", "node-chain", "node_chain", "chain", _CHAIN, "node_stage_grouped", "node", module=m, N=N))
    for K in W1CAT_K:
        s.append(_site(f"w1cat-K{K}", "node-W1cat", "typed_agg", "W1cat", ("agg_mlp.k.layers.0",), "node_stage_grouped(a_specs)",
                       "w1cat", K=K, N=11))
    s.append(_site("edge-rows", "edge", "edge_mlp", "edge", _EDGE, "edge_mlp_gumbel_grouped(edges)", "edge", form="rows",
                   module="hyper", N=11))
    s.append(_site("edge-pairpool", "edge", "edge_mlp", "edge", _EDGE, "edge_mlp_gumbel_grouped(PoolSpec, sym)", "edge",
                   form="pairpool", module="pair", N=5))
    s.append(_site("edge-hyperpool", "edge", "edge_mlp", "edge", _EDGE, "edge_mlp_gumbel_grouped(PoolSpec(H))", "edge",
                   (("GN_POOL_STAGE", "1"),), form="hyperpool", module="hyper", N=11))
    for K in AGG_K:
        for form in ("eo", "gather"):
            s.append(_site(f"agg-{form}-K{K}", "typed-agg", "typed_agg", "W12", ("agg_mlp.k.layers.0", "agg_mlp.k.layers.1"),
                           "agg_mlp_grouped(%s)" % ("eo" if form == "eo" else "GatherSpec"), "agg", form=form, K=K))
        s.append(_site(f"agg-pair-K{K}", "typed-agg", "typed_agg", "W2t", ("agg_mlp.k.layers.1",), "agg_mlp_grouped(PairSpec)",
                       "agg", form="pair", K=K))
        if K <= EC.NODE_FORM_MAX_K:
            s.append(_site(f"agg-node-K{K}", "typed-agg", "typed_agg", "W2t", ("agg_mlp.k.layers.1",),
                           "agg_mlp_grouped(PairSpec(node=True))", "agg", (("GN_NODE_FORM", "1"),), form="pair-node", K=K))
    for d in FUSED_D:
        for group in ("pair", "hyper"):
            s.append(_site(f"fused-d{d}-{group}-closing", "closing-stream", "closing_mlp", "mlp2", _MLP2, "agg_mlp_closing",
                           "fused", (("GN_FUSE_CLOSING", "1"),), dout=d, group=group, which="closing", N=11))
            s.append(_site(f"fused-d{d}-{group}-agg", "typed-agg", "typed_agg", "W2t" if group == "pair" else "W12",
                           ("agg_mlp.k.layers.1",) if group == "pair" else ("agg_mlp.k.layers.0", "agg_mlp.k.layers.1"),
                           "agg_mlp_closing", "fused", (("GN_FUSE_CLOSING", "1"),), dout=d, group=group, which="agg", N=11, K=6 if group == "pair" else 10))
    for xs, kernel in MLP2_KERNELS.items():
        for d in MLP2_D:
            for form in MLP2_FORMS:
                s.append(_site(f"{kernel[:-7]}-d{d}-{BC.form_id(form)}", kernel[:-7], "closing_mlp", "mlp2", _MLP2,
                               "mlp2_grouped(%s)" % ("x" if form[0] == "x" else "ScatterSpec"), "mlp2", (("GN_MLP2_XS", xs),),
                               xs=xs, din=128, dh=128, dout=d, form=form))
        for din, dh in BC.OTHER_WIDTHS:
            for d in MLP2_OTHER_D:
                s.append(_site(f"{kernel[:-7]}-{din}-{dh}-d{d}", kernel[:-7], "closing_mlp", "mlp2", _MLP2, "mlp2_grouped(x)", "mlp2",
                               (("GN_MLP2_XS", xs),), xs=xs, din=din, dh=dh, dout=d, form=("x", 0, din, 0)))
    return s


SITES: List[Site] = _sites()
SITE = {s.id: s for s in SITES}
KEEP_SITES = ("node-pair", "node-hyper", "edge-rows") + tuple(s.id for s in SITES if s.kind == "mlp2" and s["form"][0] == "x")


def flag_expected(value: float) -> bool:
    """The split's predicate, `!(fabsf(x) <= 65000.f)`: NaN flags."""
    return not abs(value) <= FLAG_LIMIT


def _gen(site: Site, draw: int) -> torch.Generator:
    return BC._gen(41, zlib.crc32(site.id.encode()), draw)


# ---------------------------------------------------------------------------------------------------------------------
# modules, positions, inputs
# ---------------------------------------------------------------------------------------------------------------------
class Pos(NamedTuple):
    label: str                  # "first" | "last" | "lasttype"
    lin: object                 # the nn.Linear that holds the weight
    r: int
    c: int
    layer: int                  # 1: a first-layer weight, 2: a second-layer weight (what the typed images take differs)
    tame: Callable[[float], None]      # scales by s the operand the weight multiplies


def _unit(lin, u: int) -> Callable[[float], None]:
    """Output unit u of a layer (its weight row and bias)."""
    def f(s):
        with torch.no_grad():
            lin.weight[u] *= s
            lin.bias[u] *= s
    return f


def _col(inp: Dict[str, torch.Tensor], name: str, j: int) -> Callable[[float], None]:
    def f(s):
        inp[name][..., j] *= s
    return f


def modules(site: Site) -> Dict[str, object]:
    """The site's modules on the CPU, from seeds of their own (fresh objects: a case writes into them)."""
    k = site.kind
    if k in ("node", "edge"):
        return dict(mod=EC.pair_module(6, 4100) if site["module"] == "pair" else EC.hyper_module(10, 3, 4200))
    if k == "w1cat":
        return dict(mod=EC.pair_module(site["K"], 4300 + site["K"]))
    if k == "agg":
        return dict(agg=EC.agg_module(site["K"]))
    if k == "fused":
        d = site["dout"]
        return dict(pair=BC.pair_module(d, 4500 + d), hyper=BC.hyper_module(d, 3, 4600 + d))
    return dict(mlp=BC.closing_mlp(site["dout"], site["din"], site["dh"]), other=BC.closing_mlp(site["dout"], site["din"], site["dh"], which=1))


def sources(site: Site, mods: Dict[str, object]) -> List[object]:
    """The nn.Linear layers that feed the site's image, in image order (`Site.feeds` names them)."""
    k = site.kind
    if k == "node":
        m = mods["mod"]
        return [*m.node2edge_start_mlp[0].layers, m.attention_mlp[0].layers[0]]
    if k == "edge":
        h = mods["mod"].nmp_mlp_start
        return [*h.init_MLP.layers, h.MLP_distribution.layers[0], h.MLP_factor.layers[0], h.MLP_distribution.layers[1],
                h.MLP_factor.layers[1]]
    if k in ("w1cat", "agg") or (k == "fused" and site["which"] == "agg"):
        a = (mods["agg"] if k == "agg" else mods["mod" if k == "w1cat" else site["group"]].edge_aggregation_list[0]).agg_mlp
        if site.image == "W1cat":
            return [m.layers[0] for m in a]
        if site.image == "W2t":
            return [m.layers[1] for m in a]
        return [l for m in a for l in m.layers]
    if k == "fused":
        return list(mods[site["group"]].nmp_mlp_end.layers)
    return list(mods["mlp"].layers)


def inputs(site: Site, draw: int) -> Dict[str, torch.Tensor]:
    k, g = site.kind, _gen(site, draw)
    rnd = lambda *s: torch.randn(*s, generator=g)
    if k in ("node", "w1cat"):
        return dict(x=rnd(B, site["N"], 64))
    if k == "edge":
        K = 6 if site["module"] == "pair" else 10
        if site["form"] == "rows":
            return dict(edges=rnd(B, 23, 64), U=torch.rand(B, 23, K, generator=g))
        x, N = rnd(B, site["N"], 64), site["N"]
        if site["form"] == "pairpool":
            return dict(x=x, U=torch.rand(B, N * N, K, generator=g))
        H = O.topk_incidence_ranked(O.affinity(x), 3)
        return dict(x=x, H=H, U=torch.rand(B, H.shape[1], K, generator=g))
    if k == "agg":
        form, _, N, x = AGG_FORMS[site["form"]]
        if form == "eo":
            return dict(eo=rnd(B, x, 64), ef=torch.rand(B, x, site["K"], generator=g))
        out = dict(ori=rnd(B, N, 64))
        E = pair_count(N)
        if form == "gather":
            out["H"] = O.topk_incidence_ranked(O.affinity(out["ori"]), x)
            E = out["H"].shape[1]
        out["ef"] = torch.rand(B, E, site["K"], generator=g)
        return out
    if k == "fused":
        N = site["N"]
        ori = rnd(B, N, 64)
        H = O.topk_incidence_ranked(O.affinity(ori), 3)
        return dict(ori=ori, H=H, ef_pair=torch.rand(B, pair_count(N), 6, generator=g), ef_hyper=torch.rand(B, H.shape[1], 10, generator=g))
    return BC.draw_source(site["form"], site["dout"], draw)


def positions(site: Site, mods: Dict[str, object], inp: Dict[str, torch.Tensor]) -> List[Pos]:
    """Where a case puts its weight: the first element of the image's first matrix, the last element of its last matrix
    (the last tile of the image), and for a W12 image of K > 1 types the first element of the last type's first matrix."""
    k, src = site.kind, sources(site, mods)
    if k == "node":
        s0, s1, a0 = src
        return [Pos("first", s0, 0, 0, 1, _col(inp, "x", 0)), Pos("last", a0, a0.out_features - 1, a0.in_features - 1, 1, _unit(s1, 63))]
    if k == "w1cat":
        return [Pos("first", src[0], 0, 0, 1, _col(inp, "x", 0)), Pos("last", src[-1], 127, 63, 1, _col(inp, "x", 63))]
    if k == "edge":
        i0, f0, f1 = src[0], src[3], src[5]
        first = _col(inp, "edges", 0) if site["form"] == "rows" else _unit(mods["mod"].node2edge_start_mlp[0].layers[1], 0)
        return [Pos("first", i0, 0, 0, 1, first), Pos("last", f1, 0, f1.in_features - 1, 2, _unit(f0, f0.out_features - 1))]
    if k == "agg" or (k == "fused" and site["which"] == "agg"):
        mlps = (mods["agg"] if k == "agg" else mods[site["group"]].edge_aggregation_list[0]).agg_mlp
        l0, l1 = [m.layers[0] for m in mlps], [m.layers[1] for m in mlps]
        col = _col(inp, "eo" if "eo" in inp else "ori", 0)
        last = Pos("last", l1[-1], 63, 127, 2, _unit(l0[-1], 127))
        if site.image == "W2t":
            return [last] if k == "fused" else [Pos("first", l1[0], 0, 0, 2, _unit(l0[0], 0)), last]
        first = Pos("first", l0[0], 0, 0, 1, col)
        if k == "fused":
            return [first]
        return [first, last] + ([Pos("lasttype", l0[-1], 0, 0, 1, col)] if len(l0) > 1 else [])
    w0, w1 = src
    last = Pos("last", w1, w1.out_features - 1, w1.in_features - 1, 2, _unit(w0, w0.out_features - 1))
    if k == "fused":
        return [last]
    name = "x" if site["form"][0] == "x" else "feat"       # (column 0 of cat(H^T feat, ori) / N is column 0 of feat)
    return [Pos("first", w0, 0, 0, 1, _col(inp, name, 0)), last]


def images_flagged(site: Site, pos: Pos) -> Tuple[str, ...]:
    """The images of the site's packer that a weight at `pos` must flag: layer 1 of a typed MLP feeds W1cat and W12,
    layer 2 feeds W2t and W12; every other packer has one image."""
    if site.packer != "typed_agg":
        return (site.image,)
    return ("W1cat", "W12") if pos.layer == 1 else ("W2t", "W12")


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------
def reference(site: Site, mods: Dict[str, object], inp: Dict[str, torch.Tensor], dtype=torch.float64) -> Dict[str, torch.Tensor]:
    """The outputs of the site's launch in `dtype` from the modules' current weights."""
    k = site.kind
    t = lambda name: inp[name].to(dtype)
    with torch.no_grad():
        if k == "node":
            st = cast(state_of(mods["mod"]), dtype)
            xp = O.mlp(st, "node2edge_start_mlp.0", t("x"))
            W, b = st["attention_mlp.0.layers.0.weight"], st["attention_mlp.0.layers.0.bias"]
            return dict(xp=xp, pq=torch.cat((F.linear(xp, W[:, :64], b), F.linear(xp, W[:, 64:])), -1))
        if k == "w1cat":
            st = cast(state_of(mods["mod"].edge_aggregation_list[0]), dtype)
            return dict(A=torch.cat([F.linear(t("x"), st[f"agg_mlp.{q}.layers.0.weight"], st[f"agg_mlp.{q}.layers.0.bias"] / 2)
                                     for q in range(site["K"])], -1))
        if k == "edge":
            if site["form"] == "rows":
                ef, dist = O.edge_mlp_gumbel(cast(state_of(mods["mod"].nmp_mlp_start, "head"), dtype), "head", t("edges"), t("U"))
                return dict(ef=ef, dist=dist)
            st = cast(state_of(mods["mod"]), dtype)
            if site["form"] == "hyperpool":
                ef, dist = O.edge_mlp_gumbel(st, "nmp_mlp_start", O.node2edge(st, t("x"), t("H"), 0, True)[0], t("U"))
                return dict(ef=ef, dist=dist)
            N = site["N"]
            fd, dist = O.edge_mlp_gumbel(st, "nmp_mlp_start", O.node2edge(st, t("x"), O.pairwise_incidence(N, B, dtype), 0, True)[0], t("U"))
            ii, jj, _ = pair_index(N)
            return dict(ef=fd[:, ii * N + jj] + fd[:, jj * N + ii], dist=dist)
        if k == "agg":
            return dict(feat=EC.agg_ref(state_of(mods["agg"], "agg"), AGG_FORMS[site["form"]], inp, dtype))
        if k == "fused":
            N, ori = site["N"], t("ori")
            out = {}
            for group, case, ef in (("pair", ("pair-node", B, N, 0), "ef_pair"), ("hyper", ("gather", B, N, 3), "ef_hyper")):
                m = mods[group]
                feat = EC.agg_ref(state_of(m.edge_aggregation_list[0], "agg"), case, dict(ori=inp["ori"], H=inp["H"], ef=inp[ef]), dtype)
                agg = feat if group == "pair" else torch.matmul(t("H").transpose(1, 2), feat)
                x = (torch.cat((agg, ori), -1) / N).reshape(B * N, 128)
                out["y_" + group] = BC.closing_ref(state_of(m.nmp_mlp_end), x, dtype)[0].reshape(B, N, -1)
            return out
        x = BC.closing_input(site["form"], inp, dtype)
        y, hid = BC.closing_ref(state_of(mods["mlp"]), x, dtype)
        return dict(y=y, keep_x=x, keep_hid=hid)


def gated(site: Site) -> Tuple[str, ...]:
    """The outputs of `reference` that the flagged image decides (a fused launch: the flagged group's rows)."""
    return ("y_" + site["group"],) if site.kind == "fused" else {"node": ("xp", "pq"), "w1cat": ("A",), "edge": PROB_OUTPUTS,
                                                               "agg": ("feat",), "mlp2": ("y",)}[site.kind]


def own_error(name: str, ref32: torch.Tensor, ref64: torch.Tensor) -> Tuple[float, float]:
    """(the fp32 reference's own error, a third of the gate) of one output: features as a share of max|ref64| against
    TOL_FEAT, probabilities absolute against prob_gate's floor."""
    if name in PROB_OUTPUTS:
        return abs_err(ref32, ref64), PROB_FLOOR / 3
    return rel_err(ref32, ref64), TOL_FEAT / 3


def _case(site: Site, pos: Optional[str], value: Optional[float]) -> Dict:
    last = None
    for draw in range(DRAWS):
        mods, inp = modules(site), inputs(site, draw)
        p = None
        if pos is not None:
            (p,) = [q for q in positions(site, mods, inp) if q.label == pos]
            with torch.no_grad():
                p.lin.weight[p.r, p.c] = value
            if math.isfinite(value):
                p.tame(1.0 / abs(value))
        c = dict(site=site, mods=mods, inp=inp, pos=p, value=value, draw=draw, ref64=None, ref32=None, own={})
        if value is None or math.isfinite(value):
            c["ref64"], c["ref32"] = reference(site, mods, inp), reference(site, mods, inp, torch.float32)
            c["own"] = {n: own_error(n, c["ref32"][n], c["ref64"][n]) for n in gated(site)}
        last = c
        if all(e <= third for e, third in c["own"].values()):
            return c
    raise AssertionError(f"no draw of {site.id} {pos} {value} keeps the fp32 reference within a third of the gate: {last['own']}")


def case(site: Site, pos: Optional[str] = None, value: Optional[float] = None) -> Dict:
    """-> {"site", "mods" (on the CPU), "inp", "pos" (the `Pos` written, None: every weight as drawn), "value", "draw",
    "ref64", "ref32" (`reference`; None for an infinite weight), "own" ({output: (fp32 reference's error, a third of its
    gate)})}: the first of DRAWS seeded draws of the inputs on which every gated output's fp32 reference is within a third
    of its gate.  Fresh objects on every call (the GPU tests move the modules)."""
    return _case(site, pos, value)


def cases_of(site: Site) -> List[Tuple[str, float, bool]]:
    """(position, value, flags) of the site's damaged cases: every value of WEIGHT_VALUES at the first position, 7e4 at the
    others."""
    labels = [p.label for p in positions(site, modules(site), inputs(site, 0))]
    out = [(labels[0], v, f) for v, f in WEIGHT_VALUES]
    return out + [(l, WEIGHT_VALUES[0][0], True) for l in labels[1:]]


# ---------------------------------------------------------------------------------------------------------------------
# the flag over a parameter's life
# ---------------------------------------------------------------------------------------------------------------------
LIFE_B, LIFE_N, LIFE_SCALE = 3, 11, 5
LIFE_ROUTES = ("inplace", "data", "load_state_dict")


def life_module(kind: str):
    """The pairwise module (K = 6) or the hyper module (K = 10, scale 5) of the life tests, on the CPU."""
    return EC.pair_module(6, 4700) if kind == "pair" else EC.hyper_module(10, LIFE_SCALE, 4800)
