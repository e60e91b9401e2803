"""The conditions on the references of tests/test_bf16_twins_gpu.py, held without a GPU (tests/bf16_twin_cases.py).

A. the element-wise rule on random data, for every case the GPU file runs:
   * the float64 emulation without roundings is the existing oracle function, to 1e-12;
   * the closing MLP's emulation is `bottleneck_cases.closing_ref(emulate_bf16=True)` bit for bit, and the oracle under
     `bottleneck_cases.bf16_mlps` (another summation order of the same restatement) satisfies the rule;
   * (a) the same chain in float32 torch satisfies the rule on every element; (b) the allowance s + ulp_bf16(pre) is at or
     below the old gate 8e-3 max|ref64| on every element; (c) every edge's sampled type is determined under the slack;
   * every named flaw breaks the rule on some element of every case that exercises it — with the record of which of them
     the old whole-tensor gate would have passed.
B. the exact-arithmetic probes: nothing rounds, every partial sum fits 24 bits, about half the ReLUs are active, every hidden
   unit and input column reaches some output, no two output columns are the same function, the values fac * dist takes
   are 0, 1/2 and 1, and every routing flaw changes the result.
"""
import pytest
import torch
import torch.nn.functional as F

import bf16_twin_cases as T
from bottleneck_cases import bf16_mlps, closing_input, closing_ref
from edge_type_cases import agg_ref, cast, edge_ref
from oracle import ms_hgnn_oracle as O

IDS = [T.case_id(c) for c in T.CASES]
FLAW_LOG = {}      # (flaw, stage) -> [cases, caught by the rule, passed by the old gate]


@pytest.fixture(scope="module", autouse=True)
def _flaw_table():
    yield
    if FLAW_LOG:
        print("\nnamed flaws: flaw, stage: cases / caught by the element-wise rule / passed by the old 8e-3 gate\n" + "\n".join(
            f"  {f:<13} {st:<8} {n:>3} / {c:>3} / {o:>3}" for (f, st), (n, c, o) in sorted(FLAW_LOG.items())))


def test_helpers_round_truncate_and_space_as_bf16():
    t = torch.tensor([1.0, 1.00390625, 1.005859375, -1.005859375, 3.1415926, 0.0, 2.0 ** -20, 255.5, 257.0], dtype=torch.float64)
    assert torch.equal(T.bf16r(t), t.float().bfloat16().double())
    assert T.bf16_trunc(t).tolist() == [1.0, 1.0, 1.0, -1.0, 3.140625, 0.0, 2.0 ** -20, 255.0, 256.0]
    assert T.ulp_bf16(t).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 0.0, 2.0 ** -27, 1.0, 2.0]
    x = torch.randn(4096, generator=torch.Generator().manual_seed(5)).double()      # (fp32 values: one rounding to bf16)
    up = T.bf16r(x)
    assert bool(((up - x).abs() <= T.ulp_bf16(x) / 2).all()) and bool((T.bf16_trunc(x).abs() <= x.abs()).all())


def _oracle(case):
    c = T.case_inputs(case)
    st = cast(c["state"], torch.float64)
    if case[0] == "node":
        x = c["x"].double()
        xp = O.mlp(st, "node2edge_start_mlp.0", x)
        W, b = st["attention_mlp.0.layers.0.weight"], st["attention_mlp.0.layers.0.bias"]
        return dict(xp=xp, pq=torch.cat((F.linear(xp, W[:, :64], b), F.linear(xp, W[:, 64:])), dim=-1))
    if case[0] == "edge":
        fd, dist = edge_ref(c["state"], c["edges"], c["U"], c["sym_N"])
        return dict(fd=fd, dist=dist)
    if case[0] == "agg":
        return dict(feat=agg_ref(c["state"], case[3:], c["inp"]))
    x = closing_input(c["form"], c["src"])
    return dict(y=O.mlp({"m." + k: v for k, v in st.items()}, "m", x))


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_emulation_without_roundings_is_the_oracle(case):
    with torch.no_grad():
        want = _oracle(case)
    got = T.ref64(case)
    assert set(got) == set(want)
    for k in want:
        w = want[k].reshape(got[k].shape)
        assert float((got[k] - w).abs().max()) <= 1e-12 * max(1.0, float(w.abs().max())), (T.case_id(case), k)
    # ... and so is the written-out evaluation that carries the slack
    slow = T.emulate(case, T.Arith(rounding=False))
    for k in want:
        assert float((slow[k].pre - got[k]).abs().max()) <= 1e-12 * max(1.0, float(got[k].abs().max()))


@pytest.mark.parametrize("case", T.CLOSING_CASES, ids=[T.case_id(c) for c in T.CLOSING_CASES])
def test_closing_emulation_is_the_existing_restatement(case):
    c = T.case_inputs(case)
    ref = T.reference(case)["y"]
    x = closing_input(c["form"], c["src"])
    with torch.no_grad():
        y, _ = closing_ref(c["state"], x, emulate_bf16=True)
        with bf16_mlps():
            other = O.mlp({"m." + k: v.double() for k, v in c["state"].items()}, "m", x)
    assert torch.equal(y, ref.val)
    assert T.rule_failures(other, ref) == 0


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_conditions_on_the_reference(case):
    """(a), (b), (c), and the emulation's own values inside the rule."""
    ref, r64, cond = T.reference(case), T.ref64(case), T.case_inputs(case)["cond"]
    f32 = T.emulate(case, T.Arith(torch.float32))
    lines = []
    for k, o in ref.items():
        assert bool(torch.isfinite(o.pre).all()) and bool((o.s >= 0).all()) and bool(torch.isfinite(o.s).all())
        assert T.rule_failures(o.val, o) == 0, (T.case_id(case), k, "the emulation itself")
        bad = T.rule_failures(f32[k].val, o)
        assert bad == 0, (T.case_id(case), k, f"(a): {bad} of {o.pre.numel()} elements of the fp32 chain break the rule")
        share = T.allowance_share(o, r64[k])
        lo, hi = T.bounds(o)
        lines.append(f"{k}: allowance median {float(share.median()):.2f} max {float(share.max()):.2f} of the old gate, "
                     f"{float((lo != hi).double().mean()):.1%} of elements have two admissible values, "
                     f"fp32 chain differs on {float((f32[k].val.double() != o.val).double().mean()):.2%}")
    print(f"\n{T.case_id(case)} (draw {T.case_inputs(case)['draw']}): " + "; ".join(lines)
          + (f"; (c) margin - 2 slack >= {cond['c']:.2e}, slack / tau <= {cond['first']:.2e}" if "c" in cond else ""), end="")
    assert T.conditions_hold(case, cond), (T.case_id(case), cond)
    assert cond["b"] <= 1.0, (T.case_id(case), f"(b): allowance {cond['b']:.2f} of the old gate")
    if case[0] == "edge":
        assert cond["c"] > 0 and cond["first"] <= T.FIRST_ORDER_MAX
        if case[1] == 1:
            assert bool((ref["dist"].val == 1).all()) and float(ref["dist"].s.max()) <= 1e-5


@pytest.mark.parametrize("case", T.CASES, ids=IDS)
def test_every_named_flaw_breaks_the_rule(case):
    """Each flaw a case exercises breaks the rule on some element, with the record of whether the old gate would have
    passed it."""
    ref, r64 = T.reference(case), T.ref64(case)
    clean = T.emulate(case, T.Arith(slack=False))
    assert all(T.rule_failures(clean[k].val, ref[k]) == 0 for k in ref)       # (the matmul order alone breaks nothing)
    lines = []
    for flaw in T.case_flaws(case):
        bad = T.emulate(case, T.Arith(flaw=flaw, slack=False))
        fails = sum(T.rule_failures(bad[k].val, ref[k]) for k in ref)
        n = sum(o.pre.numel() for o in ref.values())
        old = all(T.old_gate_passes(bad[k].val, r64[k]) for k in ref)
        log = FLAW_LOG.setdefault((flaw, T.stage_of(case)), [0, 0, 0])
        log[0], log[1], log[2] = log[0] + 1, log[1] + int(fails > 0), log[2] + int(old)
        lines.append(f"{flaw} {fails}/{n}{' (old gate passes)' if old else ''}")
        assert fails > 0, (T.case_id(case), flaw, "passes the element-wise rule")
    print(f"\n{T.case_id(case)}: " + ", ".join(lines), end="")


# ---- B. the exact-arithmetic probes --------------------------------------------------------------------------------------
PROBE_IDS = [T.probe_id(c) for c in T.PROBES]
PROBE_MLPS = dict(node=("node2edge_start_mlp.0",), edge=("head.init_MLP", "head.MLP_distribution", "head.MLP_factor"), closing=("",))


def _two_layer_weights(case, state):
    if case[0] == "agg":
        return [(state[f"agg.agg_mlp.{k}.layers.0.weight"], state[f"agg.agg_mlp.{k}.layers.1.weight"]) for k in range(case[1])]
    return [(state[f"{p}{'.' if p else ''}layers.0.weight"], state[f"{p}{'.' if p else ''}layers.1.weight"]) for p in PROBE_MLPS[case[0]]]


@pytest.mark.parametrize("case", T.PROBES, ids=PROBE_IDS)
def test_probe_is_exact_in_every_arithmetic(case):
    """On the float64 reference: every value a twin stores equals its own bf16 rounding, every partial sum fits 24 bits (all
    terms are multiples of PROBE_QUANTUM and sum|terms| stays below 2^24 of them), about half the ReLUs are active, every
    hidden unit and every input column reaches some output, no two output columns are the same function — and so the
    result is the same bit for bit written out or through matmul, in float64 or float32, with the bf16 roundings of the
    twins in place or not, in the order of operations of either aggregation kernel."""
    A = T.Exact()
    got, ref = T.probe_eval(case, A), T.probe_reference(case)
    variants = [got, T.probe_eval(case, T.Arith(torch.float32, rounding=False)), T.probe_eval(case, T.Arith(torch.float32)),
                T.probe_eval(case, T.Arith(slack=False))]
    if case[0] == "agg" and case[2] not in ("scene", "pair-node"):
        variants += [T.probe_eval(case, T.Arith(torch.float32), "rb2"), T.probe_eval(case, T.Arith(slack=False), "rb2")]
    for v in variants:
        for k in ref:
            assert torch.equal(v[k].double(), ref[k]), (T.probe_id(case), k)
    for t in A.stored:
        assert torch.equal(T.bf16r(t), t), (T.probe_id(case), "a stored value rounds")
    for k, v in ref.items():
        assert torch.equal(T.f32r(v) if k == "fd" else T.bf16r(v), v), (T.probe_id(case), k, "the result rounds")
    assert all(gran for _, gran in A.sums) and max(m for m, _ in A.sums) < 2.0 ** T.PROBE_BITS * T.PROBE_QUANTUM
    st = T.probe_inputs(case)["state"]
    scene = case[0] == "agg" and case[2] in ("scene", "pair-node")
    # (scene form: the ReLUs are those of A'_n + A'_j over the pairs that carry weight; `hiddens` holds the type sums S)
    on = torch.cat([(h > 0).double().reshape(-1) for h in (A.relus if scene else A.hiddens)]).mean()
    assert 0.3 <= float(on) <= 0.7, (T.probe_id(case), float(on))
    for W0, W1 in _two_layer_weights(case, st):
        assert bool((W1 != 0).any(0).all()), (T.probe_id(case), "a hidden unit reaches no output")
        assert bool(((W1.abs() @ W0.abs()) > 0).any(0).all()), (T.probe_id(case), "an input column reaches no output")
        nz = torch.cat((W0, W1.t()), dim=1)
        assert bool((nz[nz != 0].abs().log2() == nz[nz != 0].abs().log2().round()).all()), "a weight that is no power of two"
    if case[0] == "node":
        Wa = st["attention_mlp.0.layers.0.weight"]
        assert bool((Wa[:, :64] != 0).any(0).all()) and bool((Wa[:, 64:] != 0).any(0).all())
    for k, v in ref.items():
        cols = v.reshape(-1, v.shape[-1])
        if k in ("feat", "y", "xp", "pq"):
            assert len({tuple(c.tolist()) for c in cols.t()}) == cols.shape[1], (T.probe_id(case), k, "two equal output columns")


@pytest.mark.parametrize("case", T.PROBE_EDGE, ids=[T.probe_id(c) for c in T.PROBE_EDGE])
def test_edge_probe_is_one_hot_and_saturated(case):
    """Logits separated by >= 128 (the Gumbel softmax is exactly one-hot in fp32 and float64), the factor exactly 0, 1/2 or
    1, every one of them taken, and the sampled type moving over the types with the input."""
    c = T.probe_inputs(case)
    K = c["K"]
    with torch.no_grad():
        e = T.edge_emul(c["state"], c["edges"], c["U"], c["sym_N"], T.Arith(rounding=False, slack=False))
    dist, fd = e["dist"].pre, e["fd"].pre
    assert bool(((dist == 0) | (dist == 1)).all()) and bool((dist.sum(-1) == 1).all())
    if K > 1:
        assert float(e["margin"].min()) >= 128
        assert len(set(dist.argmax(-1).reshape(-1).tolist())) >= min(K, 5)
    per_row = fd.sum(-1) / (2 if c["sym_N"] else 1)          # (sym: both ordered edges, or twice the self-loop)
    assert set(per_row.reshape(-1).tolist()) == {0.0, 0.5, 1.0}


@pytest.mark.parametrize("case", T.PROBES, ids=PROBE_IDS)
def test_routing_flaws_change_the_probe(case):
    """Every named routing flaw a probe's stage has changes its float64 result (a second tile's bias needs a second tile, a
    neighbouring edge or scene needs one, and a type weight that differs from its neighbour's more than one type)."""
    ref = T.probe_reference(case)
    stage = "scene" if case[0] == "agg" and case[2] in ("scene", "pair-node") else case[0]
    for flaw in T.STAGE_FLAWS[stage]:
        if flaw not in T.ROUTING_FLAWS:
            continue
        if flaw == "tile_bias" and case[0] == "closing" and case[1] <= 32:
            continue
        if flaw == "ef_neighbour" and (case[1] == 1 or (stage == "scene" and case[4] == 1)):      # (one type: every weight is 1)
            continue
        bad = T.probe_eval(case, T.Arith(rounding=False, slack=False, flaw=flaw))
        assert any(not torch.equal(bad[k], ref[k]) for k in ref), (T.probe_id(case), flaw, "leaves the probe unchanged")
