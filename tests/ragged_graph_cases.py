"""Test helper of the ragged-capture tests (tests/test_ragged_graph_cpu.py, tests/test_ragged_graph_gpu.py): the rule of
the counts kernel stated in NumPy, the masks it is tried on, and the stream offsets of a block's device-noise draws.
Pure NumPy / Python; the library is never loaded."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

NOT_PREFIX, EMPTY = 1, 2        # GN_COUNTS_NOT_PREFIX, GN_COUNTS_EMPTY (include/groupnet_hip.h)
MASK_NS = [1, 63, 64, 65, 113]  # one agent; a wave less one, a wave, a wave and one; two chunks with a short tail
MASK_ROWS = ("all valid", "all invalid", "a proper prefix", "a hole", "only the last slot")


def mask_rule(valid: np.ndarray) -> Tuple[np.ndarray, int]:
    """(B,N) bytes -> (counts (B,) int32, status): count = the length of the leading run of non-zero bytes; status ORs
    NOT_PREFIX where a non-zero byte follows a zero byte and EMPTY where the count is 0."""
    v = np.asarray(valid) != 0
    B, N = v.shape
    counts = np.where(v.all(axis=1), N, np.argmin(v, axis=1)).astype(np.int32)
    status = 0
    if (v.sum(axis=1) > counts).any():
        status |= NOT_PREFIX
    if (counts == 0).any():
        status |= EMPTY
    return counts, status


def mask_rows(N: int) -> np.ndarray:
    """The five rows of MASK_ROWS at N agents, as uint8 (valid bytes are 1, or any other non-zero value)."""
    m = np.zeros((len(MASK_ROWS), N), dtype=np.uint8)
    m[0] = 1
    m[2, :max(N // 2, 1) if N > 1 else 0] = 7       # (N = 1 has no proper prefix but the empty one)
    if N > 2:
        m[3, :N // 3 + 1] = 1
        m[3, -1] = 255                              # valid after invalid
    m[4, -1] = 1                                    # N = 1: a full row; else a hole right at the start
    return m


def prefix_mask(counts: Sequence[int], N: int) -> np.ndarray:
    return (np.arange(N)[None, :] < np.asarray(counts)[:, None])


def draw_offsets(shapes: Sequence[Tuple[int, int, int]], nmp: int) -> Tuple[List[List[int]], int]:
    """Where each (module, round) draw of a block begins in the device stream — module-major, round by round inside a
    module, pairwise first, spans back to back — and the draws of one forward."""
    offs, cur = [], 0
    for (b, e, k) in shapes:
        per = []
        for _ in range(nmp):
            per.append(cur)
            cur += b * e * k
        offs.append(per)
    return offs, cur
