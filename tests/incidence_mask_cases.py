"""Shared by tests/test_incidence_masks_{cpu,gpu}.py: the numpy statement of the bit-mask form of a hyperedge incidence
(include/groupnet_hip.h, "Bit-mask form") and the incidences the tests feed."""
import numpy as np
import torch


def np_masks(H):
    """H (B,E,N) array, E, N <= 64 -> (rowmask (B,E), colmask (B,N)) as int64: bit n of rowmask[b,e] and bit e of
    colmask[b,n] are set iff H[b,e,n] != 0."""
    H = np.asarray(H)
    B, E, N = H.shape
    assert E <= 64 and N <= 64
    nz = (H != 0).astype(np.uint64)
    wn = np.uint64(1) << np.arange(N, dtype=np.uint64)
    we = np.uint64(1) << np.arange(E, dtype=np.uint64)
    row = (nz * wn[None, None, :]).sum(axis=2, dtype=np.uint64)
    col = (nz * we[None, :, None]).sum(axis=1, dtype=np.uint64)
    return row.view(np.int64), col.view(np.int64)


def np_dense_from_rows(row, N):
    """rowmask (B,E) int64 -> the 0/1 incidence (B,E,N) float32."""
    bits = (np.asarray(row).view(np.uint64)[..., None] >> np.arange(N, dtype=np.uint64)) & np.uint64(1)
    return bits.astype(np.float32)


def np_dense_from_cols(col, E):
    """colmask (B,N) int64 -> the 0/1 incidence (B,E,N) float32."""
    bits = (np.asarray(col).view(np.uint64)[..., None] >> np.arange(E, dtype=np.uint64)) & np.uint64(1)
    return np.ascontiguousarray(bits.astype(np.float32).transpose(0, 2, 1))


def random_incidence(B, E, N, seed):
    """Random 0/1 H (B,E,N) float32 whose member counts vary per row: every row draws its own density in [0, 1]; scene 0
    has an empty first row and an empty last column, scene 1 a full last row (E = 1: the row of scene 0 is empty, the row
    of scene 1 full)."""
    g = torch.Generator().manual_seed(seed)
    p = torch.rand(B, E, 1, generator=g)
    H = (torch.rand(B, E, N, generator=g) < p).float()
    H[0, 0, :] = 0
    H[0, :, N - 1] = 0
    if B > 1:
        H[1, E - 1, :] = 1
    return H
