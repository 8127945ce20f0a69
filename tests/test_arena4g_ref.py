"""tests/arena4g_ref.py at toy size: the periodic expectation against the oracle applied record by
record, and the placements around a pretend boundary of 2^16."""
import numpy as np

import oracle
import arena4g_ref as R

K, L, N = 509, 128, 1100
BOUNDARY = 1 << 16
SEED = 810000


def test_periodic_expectation_equals_the_oracle_record_by_record():
    blk = R.periodic_block(L, SEED, K)
    assert blk.pt.size == K * L and blk.tags.size == 16 * K and ((1 << 16) // L) % K != 0
    xo, ct, tags = [], [], []
    for i in range(N):
        j = i % K
        k, nn = blk.keys[j].tobytes(), blk.nonces[j].tobytes()
        m = blk.pt[j * L:(j + 1) * L].tobytes()
        c, t = oracle.aead_seal(k, nn, m, blk.aad[blk.aoff[j]:blk.aoff[j + 1]].tobytes())
        ok, back = oracle.aead_open(k, nn, c, t, blk.aad[blk.aoff[j]:blk.aoff[j + 1]].tobytes())
        assert ok and back == m
        xo.append(oracle.chacha20_xor(k, nn, m, int(blk.ctr[j])))
        ct.append(c)
        tags.append(t)
    as_u8 = lambda parts: np.frombuffer(b"".join(parts), dtype=np.uint8)
    assert np.array_equal(R.periodic_expect(blk.xo, N, K, L), as_u8(xo))
    assert np.array_equal(R.periodic_expect(blk.ct, N, K, L), as_u8(ct))
    assert np.array_equal(R.periodic_expect(blk.tags, N, K, 16), as_u8(tags))
    # AAD lengths cycle inside the period; the counters wrap before, inside and after the two blocks
    assert {int(blk.aoff[j + 1] - blk.aoff[j]) for j in range(K)} == {0, 1, 16, 17}
    assert {int(-int(c)) & 0xFFFFFFFF for c in blk.ctr} == set(range(7))


def test_periodic_slices_tile_the_array_and_find_a_wrapped_record():
    want = R.periodic_expect(R.periodic_block(L, SEED, K).ct, N, K, L)
    blk = R.periodic_block(L, SEED, K).ct
    for max_bytes in (K * L, 2 * K * L + 7, 1 << 30):
        pieces = R.periodic_slices(N, K, L, max_bytes)
        assert pieces[0][0] == 0 and pieces[-1][1] == N * L
        assert all(a[1] == b[0] for a, b in zip(pieces, pieces[1:]))
        assert all(hi - lo == rows * K * L <= max_bytes for lo, hi, rows in pieces[:-1])
        assert pieces[-1][2] == 0 and pieces[-1][1] - pieces[-1][0] == (N % K) * L
        assert R.periodic_first_diff(want, blk, N, K, L, max_bytes) is None
    assert R.periodic_slices(2 * K, K, L, K * L) == [(0, K * L, 1), (K * L, 2 * K * L, 1)]
    # a record written one boundary lower (2^16 / L = 512 records, no multiple of K) is seen, at
    # the record it left unwritten or the one it overwrote, whichever comes first
    wrap = BOUNDARY // L
    for i in (wrap, wrap + 1, N - 1):
        got = want.copy()
        got[(i - wrap) * L:(i - wrap + 1) * L] = want[i * L:(i + 1) * L]
        assert R.periodic_first_diff(got, blk, N, K, L, 3 * K * L)[1] == i - wrap
    got = want.copy()
    got[N * L - 1] ^= 1
    assert R.periodic_first_diff(got, blk, N, K, L, K * L) == (N * L - 1, N - 1)


LENS = (1500, 65537 % 4099, 4140, 5119, 0, 1, 15, 16, 17, 63, 64, 65)


def test_high_base_tables():
    for mode in ("cut", "straddle"):
        offs = R.high_base_offsets(LENS, 2, BOUNDARY, mode)
        assert np.array_equal(np.diff(offs), LENS) and offs[0] > 0
        role = R.boundary_roles(offs, BOUNDARY)
        if mode == "cut":
            assert role == dict(ends=[1], straddles=[], starts=[2])
        else:
            assert role == dict(ends=[], straddles=[2], starts=[]) and offs[2] % 4 == 3
        assert (offs[:2] < BOUNDARY).all() and (offs[3:] > BOUNDARY).all()


def test_split_tables_layout():
    lens_c = (4140, 5119, 0, 1, 15, 16, 17, 63, 64, 65, 127, 1500)
    lens_a, lens_b = lens_c[:6], (129, 2000, 1500, 1025)
    s = R.split_tables(lens_a, lens_b, lens_c, BOUNDARY)
    n_tab = len(s.lens)
    assert n_tab == 6 + 4 + 12 + 2 and len(s.named) == n_tab - 2 and {s.u1, s.u2}.isdisjoint(s.named)
    assert max(s.named) >= len(s.named), "an index of the order must reach past count"
    for t in (s.cut, s.straddle):
        assert (np.diff(t) >= 0).all()
        assert all(int(t[i + 1] - t[i]) == s.lens[i] for i in s.named)
    # exactly one record ends at, one starts at (cut) and one straddles (straddle) the boundary
    assert R.boundary_roles(s.cut, BOUNDARY, s.named) == dict(ends=[s.B[-1]], straddles=[], starts=[s.C[0]])
    assert R.boundary_roles(s.straddle, BOUNDARY, s.named) == dict(ends=[], straddles=[s.C[0]], starts=[])
    assert s.straddle[s.C[0]] % 4 == 3
    # the unnamed fillers span the gap in one table and are empty in the other
    assert s.cut[s.u1 + 1] - s.cut[s.u1] > BOUNDARY // 2 and s.cut[s.u2 + 1] == s.cut[s.u2]
    assert s.straddle[s.u2 + 1] - s.straddle[s.u2] > BOUNDARY // 2 and s.straddle[s.u1 + 1] == s.straddle[s.u1]
    # B moves across the boundary between the tables; A stays low, C high
    assert all(s.cut[i] >= BOUNDARY - sum(lens_b) and s.straddle[i + 1] < BOUNDARY for i in s.B)
    assert all(s.cut[i + 1] < BOUNDARY and s.straddle[i + 1] < BOUNDARY for i in s.A)
    assert all(s.cut[i] >= BOUNDARY and s.straddle[i + 1] > BOUNDARY for i in s.C)
    # the alias records: live low records exactly one boundary below a high one
    assert R.aliases(s.cut, BOUNDARY, s.named) == [(s.A[0], s.C[0]), (s.A[1], s.C[1]), (s.A[3], s.C[3]),
                                                   (s.A[4], s.C[4]), (s.A[5], s.C[5])]
    assert R.aliases(s.straddle, BOUNDARY, s.named) == [(s.A[0], s.C[1])]
    order = R.mixed_order(s.named, 5)
    steps = np.sign(np.diff(order))
    assert sorted(order) == s.named and (steps > 0).any() and (steps < 0).any()
