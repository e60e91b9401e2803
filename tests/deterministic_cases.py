"""Test helper of the deterministic-mode tests (tests/test_deterministic_cpu.py, tests/test_deterministic_gpu.py): the
cases of the ordered split-K GEMM, the split rule include/groupnet_hip.h states for it, the K slices that rebuild an
accumulate problem's partial sums one by one, and the gates the module tests apply — restated from the files that own
them, which the CPU test pins.  Pure torch; the library is loaded by the tests, never here.

The order checks rest on one property of the split rule: a K slice [s kchunk, (s+1) kchunk) of an accumulate problem, run
as a problem of its own, has ONE split and the staging kernel of the whole (K a multiple of 32, operands that stay 16-byte
aligned at every slice) — so its result is the partial tile of split s, bit for bit, and
C_old + partial[0] + partial[1] + ... in ascending order with elementwise fp32 adds is what the ordered form must return.
"""
from __future__ import annotations

from typing import List, Tuple

import torch

import backward_kernel_refs as R

# the gates of the module tests, restated (tests/test_deterministic_cpu.py compares them with their owners)
TOL_CLEAN = 2e-5        # tests/test_backward_gpu.py:12 — of max|grad| on scenes without a ReLU input in the rounding window
TOL_ANY = 2e-3          # tests/test_backward_gpu.py:13 — any batch
FORWARD_ABS = 1e-5      # tests/test_backward_gpu.py:86, tests/test_ragged_backward_gpu.py:174 — forward values
N2E_MAX_N = 140         # route.N2E_BWD_SCENE_MAX_N, ragged_backward_cases.LDS_LIMIT_N

BM, BN, BK = 128, 64, 32


def split_rule(M: int, N: int, K: int, accum: bool) -> Tuple[int, int]:
    """(splits, kchunk) as include/groupnet_hip.h states them for gn_gemm_grouped_det_f32."""
    s0 = 1
    if accum:
        s0 = min(R.cdiv(512, R.cdiv(M, BM) * R.cdiv(N, BN)), R.cdiv(K, 256))
    kchunk = R.cdiv(R.cdiv(K, s0), BK) * BK
    return R.cdiv(K, kchunk), kchunk


# Accumulate problems on the vector path whose slices stay on it: one tile and K = 8224 (33 splits: 32 of 256 and one of
# 32) with rs and colsum; a plain-A problem over two tiles (3 splits of 256); the production dW2_k shape written transposed
# (9 splits: 8 of 256 and one of 32).
ORDER_CASES = [
    R.GemmCase("order_dW_colsum_rs_K8224", 96, 64, 8224, tA=True, accum=True, rs=3, colsum=True, seed=90),
    R.GemmCase("order_deo_rs_plain_A", 198, 64, 768, accum=True, rs=1, seed=91),
    R.GemmCase("order_dW2k_tC", 128, 64, 2080, tA=True, accum=True, tC=True, rs=12, seed=92),
]
# the second problem of a chain on ORDER_CASES[0]'s destination: other operands, another K
CHAIN_SECOND = R.GemmCase("order_chain_second_K544", 96, 64, 544, tA=True, accum=True, rs=1, colsum=True, seed=93)


def operands(c: R.GemmCase, dev=None):
    """The views of one case as `backward.GemmBatch.add` takes them: dict(A, B, C, Cbuf, mask, rs, colsum, bias)."""
    d = {k: (v if dev is None else v.to(dev)) for k, v in R.gemm_inputs(c).items()}
    Cbuf = d["C0"].clone()
    return dict(A=R.view2d(d["A"], *c.a_shape, c.lda, c.offA), B=R.view2d(d["B"], *c.b_shape, c.ldb), Cbuf=Cbuf,
                C=R.view2d(Cbuf, *c.c_shape, c.ldc_, c.offC),
                mask=R.view2d(d["mask"], c.M, c.N, c.N + 4) if c.mask else None,
                rs=d["rs"].as_strided((c.a_shape[0],), (c.rs,), 1 if c.rs > 1 else 0) if c.rs else None,
                colsum=d["colsum0"].clone() if c.colsum else None, bias=d.get("bias"))


def add(gb, c: R.GemmCase, o: dict, C=None, colsum=None) -> None:
    """Case c on the operands `o` (C / colsum: another destination than its own)."""
    gb.add(o["A"], o["B"], o["C"] if C is None else C, c.tA, c.tB, o["bias"], o["mask"], c.relu, c.alpha, c.beta, rs=o["rs"],
           colsum=o["colsum"] if colsum is None else colsum, accum=c.accum, tC=c.tC)


def k_slices(c: R.GemmCase, o: dict) -> List[dict]:
    """The operands of every K slice of the split rule, in ascending order: dict(A, B, rs, K)."""
    splits, kchunk = split_rule(c.M, c.N, c.K, c.accum)
    out = []
    for s in range(splits):
        k0, k1 = s * kchunk, min(c.K, (s + 1) * kchunk)
        A = o["A"][k0:k1] if c.tA else o["A"][:, k0:k1]
        Bm = o["B"][:, k0:k1] if c.tB else o["B"][k0:k1]
        rs = o["rs"] if o["rs"] is None or not c.tA else o["rs"][k0:k1]       # rs scales A's STORED rows
        out.append(dict(A=A, B=Bm, rs=rs, K=k1 - k0))
    return out
