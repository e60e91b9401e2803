"""The range flag behind the two-part fp16 weight images, at every kernel that reads it, and over a parameter's life.
Needs an MI355X: `pytest -m gpu`.

Every kernel of the f16x3 path finds its image's flag word at an offset it recomputes from its own count of sub-steps
(tests/weight_image_cases.py lists the seven call sites and one site per image and kernel form).  A wrong offset fails
silently: read past the image an out-of-range weight is missed, read inside it every launch falls back to bf16x6 —
right results, the fp16 speed gone.  Per site, stand-alone so that the stage's bits can be compared:

  (a) in range, the fast path really runs: the f16x3 launch differs in some bit from the same launch in the bf16x6 mode
      and agrees with it to 2e-6 max(1, max|bf16x6|) (the idiom of test_f16x3_fallback_is_the_bf16x6_path);
  (b) one weight of one source matrix out of range (first element, last element of the last matrix, the last type's
      matrix; 7e4, -7e4, +inf, 65001 — and 65000, which must NOT flag): the flag words of the packer's images are
      exactly the expected ones, the f16x3 launch is finite and bit-identical to the bf16x6-mode launch, a sibling stage
      of another image still passes (a), and the activations a training forward keeps (`keep=`) are bit-identical too;
  (c) flagged, the result is right: against float64 at TOL_FEAT of max|ref64| (features) and scene_isolation_cases'
      prob_gate (probabilities), no floor of 1.0 in either.

Part 3, the flag over a parameter's life: the word follows the weights of the LAST split — set by an excursion (7e4,
NaN) through each write route, clear again once the weight is back, the stage's bits then those of a twin that never
left range; through `weights.repack_scope` (the batched split) and replays of a `GraphedTrainStep`.
"""
import copy
import math

import pytest
import torch

import weight_image_cases as W
from bottleneck_cases import TOL_FEAT
from edge_type_cases import abs_err
from scene_isolation_cases import prob_gate
from test_bottleneck_gpu import _spec
from test_edge_types_gpu import _agg_source
from test_parity_gpu import _with_precision

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    """Bit-identical (NaN payloads included: an infinite weight makes NaNs, which torch.equal calls unequal)."""
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def flag_word(pk, name, refresh=True) -> int:
    """The flag word behind image `name` of a packed set: the int32 at src.numel() // 1024 * 2048 int16 elements of a
    buffer that long plus 8.  refresh=False reads the buffer as it stands (no split is launched)."""
    xi = pk["xi"]
    n = xi.src[name].numel() // 1024 * 2048
    buf = xi.get(name, 2) if refresh else xi.img[(name, 2)][0]
    assert buf.numel() == n + 8 and buf.dtype == torch.int16
    return int(buf[n:].view(torch.int32)[0])


@pytest.fixture(autouse=True)
def _f16x3_is_the_path():
    """Every test here starts on the f16x3 path, whatever GN_PRECISION says, and leaves the path as it found it."""
    from groupnet_amd import ops
    old = ops.precision()
    ops.set_precision("f16x3")
    yield
    ops.set_precision(old)


@pytest.fixture(scope="module")
def holder():
    """A module whose `_packed_mlp2` packs any two-layer MLP and whose node stage forms any typed MLP's layer 1."""
    from edge_type_cases import pair_module
    return pair_module(6, 1).to(dev()).eval()


# ---------------------------------------------------------------------------------------------------------------------
# the stand-alone launch of every kind of site
# ---------------------------------------------------------------------------------------------------------------------
def _to_dev(c):
    for m in c["mods"].values():
        m.to(dev()).eval()
    c["dinp"] = {k: v.to(dev()) for k, v in c["inp"].items()}
    return c


def packed(site, c, holder) -> dict:
    """The packed set that holds the site's image (a call refreshes it after a write)."""
    k, mods = site.kind, c["mods"]
    if k == "node":
        return mods["mod"]._packed_n2e(0)
    if k == "edge":
        return mods["mod"].nmp_mlp_start._packed()
    if k == "w1cat":
        return mods["mod"].edge_aggregation_list[0]._packed()
    if k == "agg":
        return mods["agg"]._packed()
    if k == "fused":
        m = mods[site["group"]]
        return m._packed_mlp2(m.nmp_mlp_end) if site["which"] == "closing" else m.edge_aggregation_list[0]._packed()
    return holder._packed_mlp2(mods["mlp"])


def launch(site, c, holder, monkeypatch, keep=False):
    """The site's one launch on the current matrix path -> {output name: tensor} (keep=True: the activations a training
    forward keeps as well, "keep_*")."""
    from groupnet_amd import ops
    for name, val in site.switches:
        monkeypatch.setenv(name, val)
    k, mods, x = site.kind, c["mods"], c["dinp"]
    kept = [] if keep else None
    with torch.no_grad():
        if k == "node":
            ((xp, pq),), _ = ops.node_stage_grouped([(x["x"], mods["mod"]._packed_n2e(0))], kept)
            out = dict(xp=xp, pq=pq)
        elif k == "w1cat":
            m = mods["mod"]
            ((xp, pq),), (A,) = ops.node_stage_grouped([(x["x"], m._packed_n2e(0))], None,
                                                       [(m.edge_aggregation_list[0]._packed(), site["K"])])
            out = dict(A=A, sib_xp=xp, sib_pq=pq)
        elif k == "edge":
            m = mods["mod"]
            pk, K = m.nmp_mlp_start._packed(), m.edge_types
            if site["form"] == "rows":
                item = (x["edges"], x["U"], pk, K, 0, True)
            else:
                if "xp" not in c:      # the node stage once, on one path: both edge launches pool the same rows
                    n2e = m._packed_n2e(0)
                    c["xp"], c["pq"] = _with_precision("bf16x6", lambda: ops.node_mlp(x["x"], n2e))
                    c["w2"], c["b2"] = n2e["w2"], n2e["b2"]
                sym = site["form"] == "pairpool"
                item = (ops.PoolSpec(c["xp"], c["pq"], x.get("H"), c["w2"], c["b2"], sym), x["U"], pk, K, site["N"] if sym else 0, True)
            ((ef, dist),) = ops.edge_mlp_gumbel_grouped([item], 0.5, kept)
            out = dict(ef=ef, dist=dist)
        elif k == "agg":
            pk = mods["agg"]._packed()
            (feat,) = ops.agg_mlp_grouped([(_agg_source(W.AGG_FORMS[site["form"]], c["inp"], site["K"], pk, torch.float32),
                                            x["ef"], pk, site["K"])])
            out = dict(feat=feat)
        elif k == "fused":
            p, h = mods["pair"], mods["hyper"]
            ap, ah = p.edge_aggregation_list[0]._packed(), h.edge_aggregation_list[0]._packed()
            A = ops.node_linear(x["ori"], ap["W1cat"], ap["b1half"], 6 * 128)
            ys = ops.agg_mlp_closing([(ops.PairSpec(A, node=True), x["ef_pair"], ap, 6), (ops.GatherSpec(x["ori"], x["H"]), x["ef_hyper"], ah, 10)],
                                     [(p._packed_mlp2(p.nmp_mlp_end), None, x["ori"]), (h._packed_mlp2(h.nmp_mlp_end), None, x["ori"])])
            assert ys is not None, "the aggregation launch declined the closing stage"
            out = dict(y_pair=ys[0], y_hyper=ys[1])
        else:
            (y,) = ops.mlp2_grouped([(_spec(site["form"], c["inp"], torch.float32), holder._packed_mlp2(mods["mlp"]), None)], kept)
            out = dict(y=y)
    if keep:
        out.update({"keep_" + n: t for n, t in kept[0].items()})
    torch.cuda.synchronize()
    return {n: t.clone() for n, t in out.items()}


def sibling(site, c, holder, monkeypatch):
    """A launch that walks ANOTHER image (or another group's images) beside the damaged one -> {name: tensor}."""
    from groupnet_amd import ops
    k, mods, x = site.kind, c["mods"], c["dinp"]
    with torch.no_grad():
        if k == "node":        # the edge kernel of the same module, on rows of its own
            m = mods["mod"]
            e = torch.randn(W.B, 23, 64, generator=torch.Generator().manual_seed(7)).to(dev())
            U = torch.rand(W.B, 23, m.edge_types, generator=torch.Generator().manual_seed(8)).to(dev())
            out = dict(zip(("ef", "dist"), ops.edge_mlp_gumbel(e, U, m.nmp_mlp_start._packed(), m.edge_types)))
        elif k == "edge":      # the node stage of the same module
            xin = x["x"] if "x" in x else torch.randn(W.B, 11, 64, generator=torch.Generator().manual_seed(9)).to(dev())
            out = dict(zip(("xp", "pq"), ops.node_mlp(xin, mods["mod"]._packed_n2e(0))))
        elif k == "w1cat":     # the chain image of the same launch and the pair form (W2t) of the same packer
            out = {n: t for n, t in launch(site, c, holder, monkeypatch).items() if n.startswith("sib_")}
            pk = mods["mod"].edge_aggregation_list[0]._packed()
            A = ops.node_linear(x["x"], pk["W1cat"], pk["b1half"], site["K"] * 128)
            ef = torch.rand(W.B, W.pair_count(site["N"]), site["K"], generator=torch.Generator().manual_seed(10)).to(dev())
            (out["pair_feat"],) = ops.agg_mlp_grouped([(ops.PairSpec(A), ef, pk, site["K"])])
        elif k == "agg":
            pk, K = mods["agg"]._packed(), site["K"]
            ori = torch.randn(W.B, 11, 64, generator=torch.Generator().manual_seed(11)).to(dev())
            if c["pos"].layer == 1:       # layer 1 flags W1cat and W12: the pair form's W2t stays on the fp16 path
                ori[..., c["pos"].c] /= abs(c["value"])       # (the column the large weight multiplies, as the case's own)
                A = ops.node_linear(ori, pk["W1cat"], pk["b1half"], K * 128)
                ef = torch.rand(W.B, W.pair_count(11), K, generator=torch.Generator().manual_seed(12)).to(dev())
                out = dict(pair_feat=ops.agg_mlp_grouped([(ops.PairSpec(A), ef, pk, K)])[0])
            elif K <= 12:                 # layer 2 flags W2t and W12: the node stage's W1cat stays on the fp16 path
                _, (A,) = ops.node_stage_grouped([(ori, holder._packed_n2e(0))], None, [(pk, K)])
                out = dict(A=A)
            else:
                out = {}
        elif k == "fused":     # the other group of the same launch
            out = {n: t for n, t in launch(site, c, holder, monkeypatch).items() if n != "y_" + site["group"]}
        else:                  # another closing MLP through the same kernel
            for name, val in site.switches:
                monkeypatch.setenv(name, val)
            out = dict(y=ops.mlp2(_spec(site["form"], c["inp"], torch.float32), holder._packed_mlp2(mods["other"])))
    torch.cuda.synchronize()
    return {n: t.clone() for n, t in out.items()}


def both(fn):
    """fn() on the f16x3 path and in the bf16x6 mode."""
    return _with_precision("f16x3", fn), _with_precision("bf16x6", fn)


def _units(names):
    """The outputs by the workgroups that write them: a fused launch's groups and the node stage's chain beside its
    layer-1 workgroups vote on their own images, every other launch's outputs come from the same workgroups."""
    names = list(names)
    if any(n.startswith(("y_", "sib_")) for n in names):
        return [[n] for n in names if n.startswith("y_")] + [[n for n in names if n.startswith("sib_")], [n for n in names if n[:2] not in ("y_", "si")]]
    return [names]


def assert_fast_path(fast, slow, what):
    """(a): every output within 2e-6 max(1, max|bf16x6|) of the bf16x6 mode's, and every unit of outputs (`_units`)
    differs from it in some bit."""
    assert fast.keys() == slow.keys() and fast, what
    for n in fast:
        err, top = float((fast[n] - slow[n]).abs().max()), max(1.0, float(slow[n].abs().max()))
        assert bool(torch.isfinite(fast[n]).all()) and err <= 2e-6 * top, (what, n, err, top)
    for unit in _units(fast):
        assert not unit or any(not same_bits(fast[n], slow[n]) for n in unit), (what, unit, "the f16x3 launch IS the bf16x6 launch: it always falls back")


def assert_fallback(fast, slow, what, finite=True):
    """(b): every output bit-identical to the bf16x6 mode's."""
    assert fast.keys() == slow.keys() and fast, what
    for n in fast:
        assert same_bits(fast[n], slow[n]), (what, n, "differs from the bf16x6 launch")
        assert not finite or bool(torch.isfinite(fast[n]).all()), (what, n)


def assert_right(site, c, got, what):
    """(c): the gated outputs against float64 — features at TOL_FEAT of max|ref64|, probabilities at prob_gate."""
    line = []
    for n in W.gated(site):
        ref = c["ref64"][n]
        err = abs_err(got[n].reshape(ref.shape), ref)
        if n in W.PROB_OUTPUTS:
            assert prob_gate(got[n].reshape(ref.shape), c["ref32"][n], ref, 1.0), (what, n, err)
        else:
            top = float(ref.abs().max())
            assert err <= TOL_FEAT * top, (what, n, err / top)
            err /= top
        line.append(f"{n} {err:.1e}")
    return " ".join(line)


# ---------------------------------------------------------------------------------------------------------------------
# 2. per site: (a), (b), (c)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site", W.SITES, ids=[s.id for s in W.SITES])
def test_in_range_the_fast_path_runs(site, holder, monkeypatch):
    """(a) with every weight as drawn: no flag word of the packer is set, the launch is not the bf16x6 launch."""
    c = _to_dev(W.case(site))
    pk = packed(site, c, holder)
    assert all(flag_word(pk, name) == 0 for name in pk["xi"].src)
    fast, slow = both(lambda: launch(site, c, holder, monkeypatch))
    assert_fast_path(fast, slow, site.id)
    print(f"\n{site.id} in range: " + assert_right(site, c, fast, site.id), end="")


@pytest.mark.parametrize("site", W.SITES, ids=[s.id for s in W.SITES])
def test_flagged_image_is_the_bf16x6_launch_and_right(site, holder, monkeypatch):
    """(b) and (c) for every position and value of the site (weight_image_cases.cases_of)."""
    lines = []
    for pos, value, flags in W.cases_of(site):
        c = _to_dev(W.case(site, pos, value))
        what = f"{site.id} {pos} {value:g}"
        pk = packed(site, c, holder)
        words = {name: flag_word(pk, name) != 0 for name in pk["xi"].src}
        want = set(W.images_flagged(site, c["pos"])) if flags else set()
        assert {n for n, w in words.items() if w} == want, (what, words)
        fast, slow = both(lambda: launch(site, c, holder, monkeypatch))
        if not flags:       # 65000.0 exactly: the fp16 path, finite (its accuracy: module docstring of the cases)
            assert all(bool(torch.isfinite(t).all()) for t in fast.values()), what
            assert any(not same_bits(fast[n], slow[n]) for n in fast), (what, "fell back without a flag")
            err = {n: abs_err(fast[n].reshape(c["ref64"][n].shape), c["ref64"][n]) for n in W.gated(site)}
            lines.append(f"{pos} {value:g} not flagged, |f16x3 - float64| " + " ".join(f"{n} {e:.1e}" for n, e in err.items()))
            continue
        flagged = {n: t for n, t in fast.items() if not n.startswith("sib_") and (site.kind != "fused" or n == "y_" + site["group"])}
        assert_fallback(flagged, {n: slow[n] for n in flagged}, what, finite=math.isfinite(value))
        if math.isfinite(value):
            lines.append(f"{pos} {value:g}: " + assert_right(site, c, fast, what))
            # every other image stays in range: a sibling stage is still on the fp16 path
            sfast, sslow = both(lambda: sibling(site, c, holder, monkeypatch))
            if sfast:
                assert_fast_path(sfast, sslow, what + " sibling")
    print(f"\n{site.id}: " + "; ".join(lines), end="")


@pytest.mark.parametrize("site", [W.SITE[i] for i in W.KEEP_SITES], ids=list(W.KEEP_SITES))
def test_flagged_training_forward_keeps_the_bf16x6_activations(site, holder, monkeypatch):
    """The activations a training forward keeps for the backward (`keep=`: hid / z1, z, dh1, lgf / the input rows and
    hid) are those the second pass stored: bit-identical to the bf16x6 mode's, at every position."""
    for pos, value, _ in [x for x in W.cases_of(site) if x[1] == W.WEIGHT_VALUES[0][0]]:
        c = _to_dev(W.case(site, pos, value))
        assert flag_word(packed(site, c, holder), site.image) != 0
        fast, slow = both(lambda: launch(site, c, holder, monkeypatch, keep=True))
        assert any(n.startswith("keep_") for n in fast), site.id
        assert_fallback(fast, slow, f"{site.id} {pos} keep")
    c = _to_dev(W.case(site))
    fast, slow = both(lambda: launch(site, c, holder, monkeypatch, keep=True))
    assert_fast_path(fast, slow, site.id + " keep, in range")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the flag over a parameter's life
# ---------------------------------------------------------------------------------------------------------------------
def _life_stages(kind, mod):
    """(image name, the packed set's getter, the parameter an excursion writes, (r, c), the stage's stand-alone launch)
    of a module's four packers; inputs from seeds of their own."""
    from groupnet_amd import ops
    g = torch.Generator().manual_seed(4900 + len(kind))
    B, N, K = W.LIFE_B, W.LIFE_N, mod.edge_types
    x = torch.randn(B, N, 64, generator=g).to(dev())
    edges, U = torch.randn(B, 23, 64, generator=g).to(dev()), torch.rand(B, 23, K, generator=g).to(dev())
    ef, y = torch.rand(B, 23, K, generator=g).to(dev()), torch.randn(W.BC.ROWS, 128, generator=g).to(dev())
    agg, head, end = mod.edge_aggregation_list[0], mod.nmp_mlp_start, mod.nmp_mlp_end
    return [
        ("chain", lambda: mod._packed_n2e(0), mod.node2edge_start_mlp[0].layers[1].weight, (63, 255),
         lambda: torch.cat(ops.node_mlp(x, mod._packed_n2e(0)), -1)),
        ("edge", head._packed, head.MLP_distribution.layers[0].weight, (5, 9),
         lambda: torch.cat(ops.edge_mlp_gumbel(edges, U, head._packed(), K), -1)),
        ("W12", agg._packed, agg.agg_mlp[K - 1].layers[1].weight, (63, 127), lambda: ops.agg_mlp(edges, ef, agg._packed(), K)),
        ("mlp2", lambda: mod._packed_mlp2(end), end.layers[0].weight, (0, 0), lambda: ops.mlp2(y, mod._packed_mlp2(end))),
    ]


def _write(route, mod, param, rc, value):
    from groupnet_amd.MS_HGNN_batch import invalidate_weight_caches
    with torch.no_grad():
        if route == "inplace":                  # an in-place op: the version counter moves
            param[rc] = value
        elif route == "data":                   # behind autograd's back
            param.data[rc] = value
            invalidate_weight_caches(mod)
        else:
            sd = {k: v.detach().clone() for k, v in mod.state_dict().items()}
            (name,) = [k for k, p in mod.named_parameters() if p is param]
            sd[name][rc] = value
            mod.load_state_dict(sd)


@pytest.mark.parametrize("value", [v for v, _ in W.LIFE_VALUES], ids=["7e4", "nan"])
@pytest.mark.parametrize("route", W.LIFE_ROUTES)
@pytest.mark.parametrize("kind", ["pair", "hyper"])
def test_flag_follows_the_weight_through_every_write_route(kind, route, value):
    """0 at the start; nonzero after an excursion of one weight and a refresh; 0 again after the old value is back — and
    the stage's f16x3 bits are then exactly those of a twin that never left range (a sticky word keeps the image on the
    bf16x6 path for the life of the module: right results, the fp16 path gone)."""
    mod = W.life_module(kind).to(dev()).eval()
    twin = copy.deepcopy(mod)
    for (name, pk, param, rc, run), (_, _, _, _, run_twin) in zip(_life_stages(kind, mod), _life_stages(kind, twin)):
        what = (kind, route, value, name)
        assert flag_word(pk(), name) == 0, what
        old = float(param.detach()[rc])
        _write(route, mod, param, rc, value)
        assert flag_word(pk(), name) != 0, what
        others = [n for n in pk()["xi"].src if n != name and not (name == "W12" and n == "W2t")]
        assert all(flag_word(pk(), n) == 0 for n in others), what
        fast, slow = both(lambda: run().clone())
        assert same_bits(fast, slow), what
        _write(route, mod, param, rc, old)
        assert float(param.detach()[rc]) == old
        assert flag_word(pk(), name) == 0, (what, "the flag word outlived the weight that raised it")
        fast, slow = both(lambda: run().clone())
        ref = _with_precision("f16x3", lambda: run_twin().clone())
        assert same_bits(fast, ref), (what, "not the bits of the twin that never left range")
        assert not same_bits(fast, slow), (what, "still on the bf16x6 path")


def _f16_flags(batch):
    """{address of the packed source: flag word} of the two-part images of a RepackBatch, read as they stand."""
    return {a.data_ptr(): int(out[a.numel() // 1024 * 2048:].view(torch.int32)[0]) for a, out, parts in batch.splits if parts == 2}


def _chain_src(blk):
    """The source address of the pairwise module's chain image (its cache as it stands: no refresh, no split)."""
    from groupnet_amd import weights
    return weights.cache(blk.interaction, ("n2e", 0)).pk["xi"].src["chain"].data_ptr()


LIFE_COL = 3        # the input column the excursion's weight multiplies, scaled by 1 / 7e4: the step stays ordinary


def _life_block_inputs(seed):
    from groupnet_amd.multiscale import MultiScaleHGNN
    torch.manual_seed(seed)
    blk = MultiScaleHGNN([W.LIFE_SCALE]).to(dev()).train()
    f = torch.randn(W.LIFE_B, W.LIFE_N, 64, device=dev())
    f[..., LIFE_COL] /= 7.0e4
    tgt = torch.randn(W.LIFE_B, W.LIFE_N, blk.out_features, device=dev())
    return blk, f, tgt


def test_repack_scope_rebuilds_the_flag_with_the_image():
    """Three SGD steps of a block (pairwise K = 6, hyper K = 10 at scale 5) inside `weights.repack_scope` and of its twin
    outside: step 1 records; before step 2 a weight of the pairwise node stage goes out of range through `.data`, after
    it the batch's chain image is flagged and no other image of the batch is (the batch kernel's per-job n_tiles, images
    of different sizes in one launch); the weight is back before step 3, after which every flag is clear — and losses
    and parameters equal the twin's, bit for bit."""
    import contextlib
    from groupnet_amd import weights
    a, f, tgt = _life_block_inputs(41)
    b = copy.deepcopy(a)
    U = [[torch.rand(s, device=dev())] for s in a.noise_shapes(W.LIFE_B, W.LIFE_N)]
    holder, losses = {}, {"a": [], "b": []}
    rc = (0, LIFE_COL)
    old = {}
    for step in range(3):
        for name, blk in (("a", a), ("b", b)):
            w = blk.interaction.node2edge_start_mlp[0].layers[0].weight
            if step == 1:
                old[name] = float(w.detach()[rc])
                w.data[rc] = 7.0e4
            if step == 2:
                w.data[rc] = old[name]
            with (weights.repack_scope(holder) if name == "a" else contextlib.nullcontext()):
                out, _ = blk(f, noise_u=U)
                loss = ((out - tgt) ** 2).mean()
                blk.zero_grad(set_to_none=True)
                loss.backward()
            with torch.no_grad():
                for p in blk.parameters():
                    if p.grad is not None:
                        p.data.add_(p.grad, alpha=-0.05)
            losses[name].append(float(loss.detach()))
        if step == 0:
            continue
        flags = _f16_flags(holder["batch"])
        chain = _chain_src(a)
        assert chain in flags and len(flags) > 4, len(flags)
        assert (flags[chain] != 0) == (step == 1), (step, "the batched split left the chain image's flag word", flags[chain])
        assert all(v == 0 for k, v in flags.items() if k != chain), (step, "another image of the batch is flagged")
    print(f"\nrepack_scope with an excursion: {len(flags)} two-part images per step, losses {losses['a']}", end="")
    assert all(math.isfinite(l) for l in losses["a"]) and losses["a"] == losses["b"]
    for pa, pb in zip(a.parameters(), b.parameters()):
        assert torch.equal(pa, pb)


def test_graphed_train_step_flag_follows_the_weight_between_replays():
    """One capture, three replays; between the first and the second a weight goes out of range through `.data`, between
    the second and the third it comes back.  The chain image's flag word — rebuilt inside the graph — follows it, no other
    image is flagged, losses and gradients stay finite, and the third replay's loss equals, bit for bit, that of a twin
    whose weights never left range (lr = 0: the parameters of both are those of the start at every replay)."""
    from groupnet_amd.graphs import GraphedTrainStep
    blk, f, tgt = _life_block_inputs(43)
    twin = copy.deepcopy(blk)
    loss_fn = lambda out, H, t: ((out - t) ** 2).mean()
    steps = [GraphedTrainStep(m, torch.optim.SGD(m.parameters(), lr=0.0), loss_fn, W.LIFE_B, W.LIFE_N,
                              target_shapes=[tuple(tgt.shape)], seed=13, warmup=2) for m in (blk, twin)]
    for s in steps:
        s.counter.zero_()
    w, rc = blk.interaction.node2edge_start_mlp[0].layers[0].weight, (0, LIFE_COL)
    old = float(w.detach()[rc])
    chain = _chain_src(blk)
    losses = []
    for replay in range(3):
        if replay == 1:
            w.data[rc] = 7.0e4
        if replay == 2:
            w.data[rc] = old
        la, lb = (float(s(f, tgt)) for s in steps)
        torch.cuda.synchronize()
        flags = _f16_flags(steps[0]._repack["batch"])
        assert (flags[chain] != 0) == (replay == 1), (replay, flags[chain])
        assert all(v == 0 for k, v in flags.items() if k != chain) and not any(_f16_flags(steps[1]._repack["batch"]).values())
        assert math.isfinite(la) and all(bool(torch.isfinite(p.grad).all()) for p in blk.parameters() if p.grad is not None)
        losses.append((la, lb))
    print(f"\ngraphed step with an excursion: losses (block, twin) {losses}", end="")
    assert losses[0][0] == losses[0][1] and losses[2][0] == losses[2][1], losses
    for (n, pa), (_, pb) in zip(blk.named_parameters(), twin.named_parameters()):
        assert torch.equal(pa, pb), n      # (gradients are not compared: the backward's split-K sums are atomic)
