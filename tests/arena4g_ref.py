"""Host-side helpers of tests/test_gpu_arena_4gib.py (numpy and the C oracle only; checked at toy
size by tests/test_arena4g_ref.py).

1. Periodic batches.  A uniform batch of n records of L bytes whose record i has the key, nonce,
   start counter, AAD and plaintext of record i mod K: the oracle runs over K records once
   (periodic_block) and every array of the n-record batch -- the arenas, tags, verdicts -- is that
   block repeated.  periodic_slices cuts such an array into pieces that are whole periods (so a piece
   viewed as [rows, K * width] compares against the block by broadcasting) plus the remainder.
2. Record references (records_ref): the oracle's ChaCha20 and AEAD seal of a list of records of
   given lengths, independent of where the records lie in an arena.
3. Placements around a boundary (2^32 on the device, 2^16 in the CPU test): high_base_offsets, one
   contiguous offsets table whose offsets[0] is not zero, and split_tables, a pair of offsets tables
   with unnamed filler records for the `order` / `count` form of a batch call.
"""
import functools
from types import SimpleNamespace

import numpy as np

import oracle
from util import splitmix_bytes

K_PERIOD = 509  # a prime: see the module text of tests/test_gpu_arena_4gib.py
AAD_LENS = (0, 1, 16, 17)


def _u8(b):
    return np.frombuffer(b or b"", dtype=np.uint8)


def start_counter(i, length):
    """A ChaCha20 start counter whose u32 wrap falls inside record i: before one of its first seven
    blocks (or after the last one of a shorter record), in the middle of a longer record."""
    blocks = (length + 63) // 64
    back = i % 7 if blocks <= 7 else blocks // 2
    return (-back) & 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def records_ref(lens, seed):
    """Record i of len(lens) records: key, nonce, start counter, AAD (lengths cycling through
    0, 1, 16, 17), plaintext, and the oracle's ChaCha20 (xo), seal (ct, tag) of it.  Read-only."""
    n = len(lens)
    keys = _u8(splitmix_bytes(seed + 1, 32 * n)).reshape(n, 32)
    nonces = _u8(splitmix_bytes(seed + 2, 12 * n)).reshape(n, 12)
    aoff = np.concatenate([[0], np.cumsum([AAD_LENS[i % 4] for i in range(n)])]).astype(np.int64)
    aad = _u8(splitmix_bytes(seed + 3, int(aoff[-1])))
    ctr = np.array([start_counter(i, lens[i]) for i in range(n)], dtype=np.uint32)
    pt, ct, xo = [], [], []
    tags = np.zeros((n, 16), dtype=np.uint8)
    for i in range(n):
        m = splitmix_bytes(seed + 100 + i, lens[i])
        k, nn = keys[i].tobytes(), nonces[i].tobytes()
        c, t = oracle.aead_seal(k, nn, m, aad[aoff[i]:aoff[i + 1]].tobytes())
        pt.append(_u8(m))
        ct.append(_u8(c))
        xo.append(_u8(oracle.chacha20_xor(k, nn, m, int(ctr[i]))))
        tags[i] = _u8(t)
    for a in (keys, nonces, aoff, aad, ctr, tags):
        a.setflags(write=False)
    return SimpleNamespace(n=n, lens=lens, keys=keys, nonces=nonces, aoff=aoff, aad=aad, ctr=ctr,
                           pt=pt, ct=ct, xo=xo, tags=tags)


# ------------------------------------------------------------------ periodic batches
@functools.lru_cache(maxsize=4)
def periodic_block(L, seed, K=K_PERIOD):
    """The K records of one period, L bytes each, laid out back to back: pt / ct / xo uint8 [K * L],
    tags [K * 16], keys [K, 32], nonces [K, 12], ctr uint32 [K], aad and aoff [K + 1]."""
    r = records_ref((L,) * K, seed)
    cat = lambda parts: np.concatenate(parts) if L else np.zeros(0, dtype=np.uint8)
    blk = SimpleNamespace(K=K, L=L, keys=r.keys, nonces=r.nonces, ctr=r.ctr, aad=r.aad, aoff=r.aoff,
                          pt=cat(r.pt), ct=cat(r.ct), xo=cat(r.xo), tags=r.tags.reshape(-1).copy())
    for a in (blk.pt, blk.ct, blk.xo, blk.tags):
        a.setflags(write=False)
    return blk


def periodic_slices(n, K, width, max_bytes):
    """An array of n items of `width` bytes, item i a copy of item i mod K of a K-item block, as
    pieces (lo, hi, rows) in bytes: hi - lo == rows * K * width <= max_bytes for the whole-period
    pieces (rows >= 1), and one last piece with rows == 0 holding the n mod K items left over (it
    equals the block's first hi - lo bytes).  The pieces tile [0, n * width) in order."""
    period = K * width
    assert 0 < period <= max_bytes
    per = max_bytes // period
    whole = n // K
    out, row = [], 0
    while row < whole:
        rows = min(per, whole - row)
        out.append((row * period, (row + rows) * period, rows))
        row += rows
    if n % K:
        out.append((whole * period, n * width, 0))
    return out


def periodic_expect(block, n, K, width):
    """The n-item array itself (host memory: toy sizes only)."""
    block = np.asarray(block).reshape(K, width)
    return block[np.arange(n) % K].reshape(-1)


def periodic_first_diff(arr, block, n, K, width, max_bytes):
    """None if arr[: n * width] is the periodic array of `block`, else (byte, item) of the first
    difference.  Works piece by piece, as the device compare does."""
    block = np.asarray(block).reshape(-1)
    for lo, hi, rows in periodic_slices(n, K, width, max_bytes):
        piece = arr[lo:hi]
        want = block[None, :] if rows else block[:hi - lo]
        bad = np.flatnonzero((piece.reshape(rows, -1) if rows else piece) != want)
        if bad.size:
            return lo + int(bad[0]), (lo + int(bad[0])) // width
    return None


# ------------------------------------------------------------------ placements
def high_base_offsets(lens, k, boundary, mode, below=5):
    """int64 [n + 1]: the records back to back.  mode "cut": the last non-empty record before k ends exactly at
    `boundary` and record k starts exactly there.  mode "straddle": record k starts below the boundary at an
    address = 3 mod 4, `below` bytes under the boundary, and ends above it.  (One contiguous table
    cannot hold both: the boundary is either a cut between two records or inside one.)  Records before k lie below, after k above."""
    lens = np.asarray(lens, dtype=np.int64)
    before = int(lens[:k].sum())
    if mode == "cut":
        assert before > 0 and lens[k] > 0
        start = boundary - before
    else:
        assert mode == "straddle" and 0 < below < lens[k] and below % 4 == 1 and boundary % 4 == 0
        start = boundary - below - before
    offs = start + np.concatenate([[0], np.cumsum(lens)])
    assert offs[0] > 0
    return offs.astype(np.int64)


def boundary_roles(offs, boundary, named=None):
    """Which records of a table end exactly at, straddle, and start exactly at the boundary
    (zero-length records have no role): dict of three index lists."""
    offs = np.asarray(offs)
    idx = range(len(offs) - 1) if named is None else named
    role = dict(ends=[], straddles=[], starts=[])
    for i in idx:
        lo, hi = int(offs[i]), int(offs[i + 1])
        if hi == lo:
            continue
        if hi == boundary:
            role["ends"].append(i)
        if lo == boundary:
            role["starts"].append(i)
        if lo < boundary < hi:
            role["straddles"].append(i)
    return role


def aliases(offs, boundary, named):
    """Pairs (low, high) of named records with offs[low] == offs[high] - boundary: an access to
    `high` that lost bit log2(boundary) of its address lands on the live record `low`."""
    at = {int(offs[i]): i for i in named if offs[i + 1] > offs[i] and offs[i] < boundary}
    return [(at[int(offs[j]) - boundary], j) for j in named
            if offs[j + 1] > offs[j] and int(offs[j]) - boundary in at]


def split_tables(lens_a, lens_b, lens_c, boundary):
    """Two offsets tables over the same records for the `order` / `count` form of a call: groups A,
    B, C of named records with an unnamed record after A (index u1) and one after B (index u2).
        cut:      A low | u1 spans up to B | B and C back to back, B's last record ending exactly at
                  the boundary and C's first starting there (u2 is empty)
        straddle: A and B back to back, low (u1 is empty) | u2 spans up to C | C, whose first record
                  starts at boundary - 5 (= 3 mod 4) and straddles it
    B lies above the boundary in the one table and below it in the other: a call reading through one
    table and writing through the other moves B across.  A starts where the table's first record
    that begins at or above the boundary would land with that address bit lost (cut: offset 0,
    A[i] under C[i] while the lengths agree; straddle: under C[1]).
    Returns SimpleNamespace(lens (fillers counted 0), cut, straddle (int64 [N + 1]), named, u1, u2,
    A, B, C index lists)."""
    a, b, c = len(lens_a), len(lens_b), len(lens_c)
    u1, u2 = a, a + 1 + b
    A, B, C = list(range(a)), list(range(a + 1, u2)), list(range(u2 + 1, u2 + 1 + c))
    lens = list(lens_a) + [0] + list(lens_b) + [0] + list(lens_c)
    N = len(lens)
    sa, sb = int(sum(lens_a)), int(sum(lens_b))
    assert lens_b[-1] > 0 and lens_c[0] > 5 and lens_c[1] > 0 and boundary % 4 == 0

    def table(filler_at, low_start, high_start):
        offs = np.zeros(N + 1, dtype=np.int64)
        pos = low_start
        for i in range(N):
            offs[i] = pos
            if i == filler_at:
                assert high_start >= pos, "the low records run into the high ones"
                pos = high_start
            else:
                pos += lens[i]
        offs[N] = pos
        return offs

    cut = table(u1, 0, boundary - sb)
    straddle = table(u2, lens_c[0] - 5, boundary - 5)
    assert sa + sb + lens_c[0] < boundary - sb
    for t in (cut, straddle):
        t.setflags(write=False)
    return SimpleNamespace(lens=tuple(lens), cut=cut, straddle=straddle, named=A + B + C, u1=u1, u2=u2,
                           A=A, B=B, C=C)


def mixed_order(named, seed):
    """The named indices in a fixed pseudo-random order (not monotone)."""
    key = np.frombuffer(splitmix_bytes(seed, 4 * len(named)), "<u4")
    return [named[k] for k in np.argsort(key, kind="stable")]
