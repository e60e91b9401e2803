"""The table of tests/device_noise_cases.py is complete, and the numpy oracle of the Philox stream is right where the
table goes: checked here without a GPU, so that tests/test_device_noise_gpu.py cannot silently miss a route of
`fetch_uniforms` or compare the kernels with a wrong stream."""
import numpy as np

from device_noise_cases import (KERNEL_CASES, KERNELS, M64, POSITION_CASES, ROUTES, draw_route, effective_base, kernel_cases,
                                ordered_edges, reachable, route_counts, row_positions, straddles)
from oracle import ms_hgnn_oracle as O


def test_reachable_routes_are_what_the_branch_conditions_admit():
    """K <= 8: the swap at every residue, and o + K > 8 (residues 1..3) only with a crossing run (the first run holds four
    words and starts off a block boundary).  K > 8: no swap; nothing crosses exactly when the row starts a block."""
    want = {(True, "swap", o) for o in range(4)} | {(True, "runs_cross", o) for o in (1, 2, 3)}
    want |= {(False, "runs", 0)} | {(False, "runs_cross", o) for o in (1, 2, 3)}
    assert reachable() == want
    for K in range(1, 16):
        for pos in range(64):
            r = draw_route(K, pos)
            assert r in ROUTES and r == draw_route(K, pos + (1 << 34)) == draw_route(K, pos & 3)
            assert (r == "swap") == (K <= 8 and (pos & 3) + K <= 8)


def _seen(cases):
    return {(c.K <= 8, draw_route(c.K, p), p & 3) for c in cases for p in row_positions(c)}


def test_table_reaches_every_route_at_every_residue():
    assert _seen(KERNEL_CASES) == reachable()
    # the K <= 8 rows that leave the swap, for ordered rows of their own and for the two ordered rows of a pair row
    for sym in (False, True):
        got = {(draw_route(c.K, p), p & 3) for c in KERNEL_CASES if c.K <= 8 and bool(c.sym_N) == sym
               for p in row_positions(c) if (p & 3) + c.K > 8}
        assert got == {("runs_cross", 1), ("runs_cross", 2), ("runs_cross", 3)}, (sym, got)


def test_every_kernel_meets_every_route():
    assert len(KERNELS) == 5 and len({k.name for k in KERNELS}) == 5
    for k in KERNELS:
        assert _seen(kernel_cases(k)) == reachable(), k.id


def test_table_holds_what_the_issue_lists():
    cs = KERNEL_CASES
    assert len({c.id for c in cs}) == len(cs)
    assert {c.K for c in cs} == {1, 3, 5, 6, 7, 8, 9, 10, 12, 15}
    assert {c.offset & 3 for c in cs} == {0, 1, 2, 3}
    rows = {c.B * c.E for c in cs}
    assert 1 in rows and 15 in rows and 407 in rows and max(rows) > 256
    assert all(any(r % m for r in rows if r > m) for m in (32, 128, 256))          # ragged last block / workgroup
    for N in (1, 2, 5, 11):
        assert {c.want_dist for c in cs if c.sym_N == N} == {True, False}, N
    assert all(c.E == c.sym_N * (c.sym_N + 1) // 2 for c in cs if c.sym_N)
    assert any((c.seed >> 32) and not c.seed >> 63 for c in cs) and any(c.seed >> 63 for c in cs)
    assert all(0 <= c.seed <= M64 and 1 <= c.K <= 15 for c in cs)
    # both carries inside one row's span; 2^34 by the host offset alone and as offset + counter with each part below it
    assert any(straddles(c, 1 << 32) for c in cs)
    assert any(straddles(c, 1 << 34) and c.counter is None for c in cs)
    assert any(straddles(c, 1 << 34) and c.counter is not None and 0 < c.counter < 1 << 34 and c.offset < 1 << 34 for c in cs)
    # ... through the swap (blocks 2^32 - 1 and 2^32 in the two lanes of one row) and through a crossing run
    for route in ("swap", "runs_cross"):
        assert any(p < 1 << 34 < p + c.K and draw_route(c.K, p) == route for c in cs for p in row_positions(c)), route
    neg = [c for c in cs if c.counter is not None and c.counter < 0]
    assert neg and all(c.offset == -c.counter + 3 and effective_base(c) == 3 for c in neg)
    assert all(c.sym_N == 0 or c.id.startswith(("sym", "p34")) for c in cs)
    assert all(sum(route_counts(c).values()) == c.B * ordered_edges(c) for c in cs)


# ---- the oracle against a scalar Philox4x32-10 ---------------------------------------------------------------------
def _philox_scalar(pos, seed):
    """Uniform `pos` of stream `seed`, word by word as Salmon et al. state the generator: counter (blk lo, blk hi, 0, 0),
    key (seed lo, seed hi), ten rounds, the key bumped by the Weyl constants between rounds."""
    m32 = 0xFFFFFFFF
    blk = (pos & M64) >> 2
    c = [blk & m32, blk >> 32, 0, 0]
    k0, k1 = seed & m32, (seed >> 32) & m32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & m32, (p0 >> 32) ^ c[3] ^ k1, p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
    return np.float32(c[pos & 3] >> 8) * np.float32(2.0 ** -24)


def test_scalar_philox_reproduces_the_published_vectors():
    """Random123 kat_vectors, philox4x32-10 (the scalar form above is then an independent statement of the stream)."""
    def words(ctr, key):
        m32 = 0xFFFFFFFF
        c, (k0, k1) = list(ctr), key
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k0, p1 & m32, (p0 >> 32) ^ c[3] ^ k1, p0 & m32]
            k0, k1 = (k0 + 0x9E3779B9) & m32, (k1 + 0xBB67AE85) & m32
        return c
    assert words((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert words((0xffffffff,) * 4, (0xffffffff,) * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert words((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # the uniform of a position is word (pos & 3) of block pos >> 2 under key = seed
    assert _philox_scalar(2, 0) == np.float32(0xbc57ac4c >> 8) * np.float32(2.0 ** -24)


def test_oracle_equals_scalar_philox_at_the_tables_positions():
    """Whole draws of the small cases, and of the large ones the rows around the carries plus both ends."""
    checked = 0
    for c in KERNEL_CASES:
        n, base = c.B * ordered_edges(c) * c.K, effective_base(c)
        u = O.philox_uniform(n, c.seed, base)
        assert u.dtype == np.float32 and u.shape == (n,)
        idx = set(range(n)) if n <= 1024 else set(range(64)) | set(range(n - 64, n)) | set(range(0, n, 97))
        for b in (1 << 32, 1 << 34):
            if base < b < base + n:
                idx |= set(range(max(0, b - base - 40), min(n, b - base + 40)))
        for i in sorted(idx):
            assert u[i] == _philox_scalar(base + i, c.seed), (c.id, i)
        checked += len(idx)
    assert checked > 5000
    for c in POSITION_CASES:                 # block indices >= 2^32 and wrapped positions really are in there
        assert effective_base(c) == 3 or effective_base(c) + c.B * ordered_edges(c) * c.K > 1 << 32


def test_oracle_block_index_beyond_2_32_uses_the_high_counter_word():
    """Positions 2^34 .. 2^34 + 3 are block 2^32 = counter (0, 1, 0, 0): not block 0 again."""
    a, b = O.philox_uniform(4, 5, 1 << 34), O.philox_uniform(4, 5, 0)
    assert not np.array_equal(a, b)
    assert [float(x) for x in a] == [float(_philox_scalar((1 << 34) + i, 5)) for i in range(4)]
