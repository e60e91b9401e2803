"""Test helper: where the edge kernels' in-kernel Philox draws can go wrong, as a table (no GPU needed).

Contract: element (row, k) of a (B, E, K) draw is element  host offset + device counter + row*K + k  of the
Philox4x32-10 stream `seed`, the sum taken modulo 2^64.  `fetch_uniforms` (gn_mlp_common.hpp) reaches a row's K words by
one of three routes, chosen from K and the row's first position; `draw_route` restates that choice so that the table
below can be checked for completeness on the CPU (tests/test_device_noise_cpu.py) before tests/test_device_noise_gpu.py
runs it on every edge kernel.
"""
from collections import Counter, namedtuple

M64 = (1 << 64) - 1
ROUTES = ("swap", "runs", "runs_cross")


def draw_route(K, pos_row):
    """Route of `fetch_uniforms` for a row of K uniforms whose first stream position is `pos_row`:
      "swap"        K <= 8 and o + K <= 8 (o = pos_row & 3): the row's two lanes evaluate one block each and exchange;
      "runs"        runs of four positions (lane h, run g: features 8g + 4h ..), every run inside one block;
      "runs_cross"  at least one run crosses into the next block (the shift network selects word o + j)."""
    o = pos_row & 3
    if K <= 8 and o + K <= 8:
        return "swap"
    cross = False
    for g in range(2):
        for h in range(2):
            f0 = 8 * g + 4 * h
            if f0 < K and (pos_row + f0) % 4 + min(K - f0, 4) > 4:
                cross = True
    return "runs_cross" if cross else "runs"


def reachable():
    """{(K <= 8, route, residue of the row's first position)} over every K the ABI admits."""
    return {(K <= 8, draw_route(K, o), o) for K in range(1, 16) for o in range(4)}


# ---- the five kernels -----------------------------------------------------------------------------------------------
# name: the kernel as a trace shows it; dtype of the activations; how Python selects it (`precision` through
# ops.set_precision on fp32 tensors, `rb2` through GN_EDGE_RB2 on bf16 tensors); what the launcher's plan must then say
# (gn_kernel_name(plan.kernel), plan.precision); `pool`: the kernel can form its rows itself (ops.PoolSpec).
Kernel = namedtuple("Kernel", "id name dtype precision rb2 plan_kernel plan_precision pool")
KERNELS = [
    Kernel("fp32", "edge_mlp_gumbel_kernel", "float32", "fp32", None, "edge_mlp_gumbel_kernel", 0, False),
    Kernel("bf16x6", "edge_x_kernel<3,float>", "float32", "bf16x6", None, "edge_x_kernel", 3, True),
    Kernel("f16x3", "edge_x_kernel<2,float>", "float32", "f16x3", None, "edge_x_kernel", 2, True),
    Kernel("bf16-rb1", "edge_x_kernel<1,__bf16>", "bfloat16", None, "0", "edge_x_kernel", 1, True),
    Kernel("bf16-rb2", "edge_rb2_kernel<__bf16>", "bfloat16", None, "1", "edge_rb2_kernel", 1, True),
]


def select_kernel(kernel, monkeypatch):
    """Make the launcher pick `kernel` for tensors of the returned dtype; monkeypatch restores every setting."""
    import torch
    from groupnet_amd import ops
    monkeypatch.setattr(ops, "BF16X6", ops.BF16X6)
    monkeypatch.setattr(ops, "F16X3", ops.F16X3)
    if kernel.precision is not None:
        ops.set_precision(kernel.precision)
    if kernel.rb2 is not None:
        monkeypatch.setenv("GN_EDGE_RB2", kernel.rb2)
    return getattr(torch, kernel.dtype)


# ---- the cases --------------------------------------------------------------------------------------------------------
# One stand-alone edge MLP each: `E` rows of edges per scene (sym_N > 0: the N(N+1)/2 unordered pairs of N nodes, drawing
# for the N*N ordered edges), uniforms at host offset `offset` + device counter `counter` (None: no counter tensor).
Case = namedtuple("Case", "id K B E sym_N want_dist seed offset counter")

SEED_LO = 77
SEED_HI = (1 << 40) + 17                  # non-zero high key word
SEED_TOP = (1 << 63) + 0x1234567          # bit 63 set
SEED_ALL = 0xDEADBEEF9E3779B9             # both words busy, bit 63 set
STEP = 17_408_000                         # about one forward's draws at B = 1024, N = 50, four scales


def _pairs(N):
    return N * (N + 1) // 2


def _table():
    t = []

    def add(tag, K, B, E, seed, offset, counter=None, sym_N=0, want_dist=True):
        t.append(Case(f"{tag}-K{K}-{B}x{E}-o{offset & 3}" + (f"-sym{sym_N}{'' if want_dist else '-nodist'}" if sym_N else ""),
                      K, B, E, sym_N, want_dist, seed, offset, counter))

    # every K at 3 x 5 = 15 rows (ragged against 32).  Odd K: the rows walk through all four residues by themselves;
    # K = 6, 10: through two, so one even and one odd offset; K = 8, 12: every row has the offset's residue, so all four.
    seeds = [SEED_LO, SEED_HI, SEED_TOP, SEED_ALL]
    for n, (K, off) in enumerate([(1, 0), (3, 1), (5, 2), (7, 3), (9, 4), (15, 5)]):
        add("odd", K, 3, 5, seeds[n % 4], off, counter=1000 if n % 2 else None)
    for n, (K, off) in enumerate([(6, 0), (6, 17), (10, 2), (10, 1123)]):
        add("even", K, 3, 5, seeds[n % 4], off, counter=None if n % 2 else 2000)
    for n, (K, off) in enumerate([(8, 0), (8, 1), (8, 2), (8, 3), (12, 4), (12, 5), (12, 6), (12, 7)]):
        add("fixed", K, 3, 5, seeds[n % 4], off, counter=3000 if n < 4 else None)
    # 37 x 11 = 407 rows: ragged against 32, 128 and 256, and more than 256 (a two-row-block workgroup with both blocks
    # live, then one with a dead tail)
    add("rows", 10, 37, 11, SEED_LO, 123, counter=1000)
    add("rows", 7, 37, 11, SEED_TOP, 6)
    add("rows", 6, 37, 11, SEED_HI, 17)
    # a single row
    add("one", 7, 1, 1, SEED_ALL, 2)               # o + K > 8
    add("one", 5, 1, 1, SEED_LO, 3)                # swap at the last residue it admits
    add("one", 10, 1, 1, SEED_HI, 4)               # runs, nothing crossing
    add("one", 15, 1, 1, SEED_TOP, 1)
    # symmetric pairwise form: two ordered rows per pair row
    for N, B in ((1, 3), (2, 3), (5, 3), (11, 5)):
        add("sym", 6, B, _pairs(N), SEED_LO + N, 17, sym_N=N, want_dist=True)               # odd offset: o = 1 and 3
        add("sym", 6, B, _pairs(N), SEED_HI + N, 4 * N + 2, sym_N=N, want_dist=False, counter=40)
    add("sym", 7, 3, _pairs(5), SEED_TOP, 0, sym_N=5, want_dist=True)
    add("sym", 8, 3, _pairs(5), SEED_ALL, 3, sym_N=5, want_dist=False)
    add("sym", 8, 3, _pairs(2), SEED_LO, 1, sym_N=2, want_dist=True)
    add("sym", 10, 3, _pairs(5), SEED_LO, 9, sym_N=5, want_dist=True)
    add("sym", 15, 2, _pairs(11), SEED_HI, 2, sym_N=11, want_dist=False)
    # positions: a row's span straddles 2^32 (the low counter word of the POSITION carries) ...
    add("p32", 10, 3, 11, SEED_LO, (1 << 32) - 13)
    add("p32", 5, 3, 5, SEED_TOP, (1 << 32) - 33)
    add("p32", 7, 3, 5, SEED_HI, (1 << 31) + 5, counter=(1 << 31) - 30)
    # ... and 2^34 (block index 2^32: the second counter word becomes 1) by the host offset alone ...
    add("p34", 10, 3, 11, SEED_ALL, (1 << 34) - 27)
    add("p34", 5, 3, 5, SEED_LO, (1 << 34) - 33)
    add("p34", 6, 3, _pairs(5), SEED_HI, (1 << 34) - 75, sym_N=5)
    # ... and as host offset + device counter, each below it
    add("p34c", 7, 3, 5, SEED_TOP, (1 << 33) + 5, counter=(1 << 33) - 30)
    add("p34c", 12, 3, 5, SEED_LO, (1 << 33) - 61, counter=(1 << 33) + 2)
    # the graphs' convention: the counter starts one step back (int64 -d, i.e. 2^64 - d), host offset d + 3
    add("neg", 10, 3, 11, SEED_HI, STEP + 3, counter=-STEP)
    add("neg", 6, 3, 5, SEED_ALL, STEP + 3, counter=-STEP)
    return t


KERNEL_CASES = _table()
POSITION_CASES = [c for c in KERNEL_CASES if c.id.split("-")[0] in ("p32", "p34", "p34c", "neg")]


def kernel_cases(kernel):
    """The cases `kernel` runs: every one (a stand-alone edge MLP reads `edges`, which every kernel accepts)."""
    return list(KERNEL_CASES)


def effective_base(case):
    """First stream position of the draw: the unsigned 64-bit sum the kernel forms."""
    return (case.offset + (case.counter or 0)) & M64


def ordered_edges(case):
    """Ordered edges per scene: the E of the (B, E, K) noise / dist layout."""
    return case.sym_N * case.sym_N if case.sym_N else case.E


def row_positions(case):
    """First stream position of every ordered row, modulo 2^64."""
    base, K = effective_base(case), case.K
    return [(base + r * K) & M64 for r in range(case.B * ordered_edges(case))]


def route_counts(case):
    return Counter(draw_route(case.K, p) for p in row_positions(case))


def straddles(case, boundary):
    """Does one row's span [pos, pos + K) hold positions on both sides of `boundary`?"""
    return any(p < boundary < p + case.K for p in row_positions(case))


def describe(kernel, case):
    rc = route_counts(case)
    return (f"{kernel.name}: {case.id}, {case.B * case.E} rows ({case.B * ordered_edges(case)} ordered), base "
            f"{effective_base(case):#x}, routes " + ", ".join(f"{r} {rc[r]}" for r in ROUTES if rc[r]))
