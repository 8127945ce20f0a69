"""Device arenas at and past 4 GiB: the cipher, hash and tile kernels with offsets on both sides of
2^32, every byte against the CPU oracle (oracle.*) or hashlib, never against another kernel run.

Several kernels address their arenas with 32-bit offsets on purpose and rely on the host's routing
(csrc/record_route.hpp, csrc/long_route.hpp) to stay below 4 GiB; the others carry 64-bit offsets
through 32-bit lane arithmetic.  A truncated offset does not fault: it reads or writes 4 GiB lower,
inside the same arena.  Two arenas of 4 GiB + 64 MiB (input: uninitialised memory; output: 0x5A
before every call, with a 256-byte guard on each end) are allocated once for the module.

A. Sparse.  A few records placed around offset 2^32 (tests/arena4g_ref.py builds the tables):
   high base -- one contiguous table with offsets[0] = 2^32 - X, either with a cut exactly at 2^32
   (one record ends there, the next starts there) or with one record straddling it from an address
   = 3 mod 4 (a contiguous table cannot hold both, so every high-base call runs with each), records
   below and above, also in place;
   split -- the `order` / `count` form: named records near offset 0, an unnamed filler record of
   almost 4 GiB, named records around and above 2^32, the order mixing both sides.  Calls with two
   tables read through one and write through the other, so one group of records moves across 2^32
   in each direction; the low records lie exactly 2^32 below high ones, so an access that lost
   bit 32 lands on live data.
   After each call the named records' ranges are copied to the host and compared, then refilled,
   and every 8-byte word of the whole output arena (guards included) must hold the fill: that scan,
   on the device in 256 MiB slices, is what sees a store that went to offset - 2^32.  Tags, MACs,
   digests, verdicts and statuses sit between guards of their own, prefilled alike.
     1. ChaCha20 (counters wrapping inside the records), AEAD seal / open with AAD and tampering,
        on the per-lane record kernel at 1, 4 and 16 lanes per record;
     2. 1024 uniform records on each staged kernel (Stream, Lockstep, LineStaged, RunStaged) with a
        high base, 2^32 inside a record of the second workgroup;
     3. frames, wire frames, session wire frames, AEAD + HMAC, chunk store / fetch: on the duplex
        kernel, with the split form forced on, and on the two-pass path (the hash kernel's
        dest_off, guard_off, wire_in and zero_on_fail past 2^32); the session calls have only the
        duplex kernel;
     4. SHA-256 / HMAC-SHA256 / verify over 330 messages from offset 2^32 - 100;
     5. tiles: plan + tiles, uniform xor, uniform AEAD, and a long chunk hashed on host threads;
     6. chunk transfer frames, both arenas with a high base, one frame for each non-zero status.
   Announce, control and classify frames are left out: their arenas would need more than 3 M
   frames per call to reach 4 GiB.
B. Dense.  Uniform batches at the routing limits (rows 40-43 and 59-60 of
   tests/cpp/record_route_table.cpp), whole arena compared.  Record i has the key, nonce, counter,
   AAD and plaintext of record i mod K, K = 509: the oracle runs over K records once and the device
   compares the arena, viewed as [n // K, K L], against that block.  K is prime: a workgroup holds
   512 / P records (a power of two) and an access that wraps by 2^32 bytes lands 2^32 / L records
   lower (L = 4096, 65 536: a power of two; L = 1500: floor(2^32 / 1500) = 2 863 311 =
   509 * 5625 + 186), none a multiple of 509, so a wrapped or workgroup-shifted access always
   meets bytes of a different record of the period (asserted per case as
   ((1 << 32) // L) % K != 0).
Every call that has a route asserts it (record_route_counts / seg_batches / host_hash_batches)
before its bytes.  Memory held at once: the two arenas and the temporaries of one 256 MiB slice."""
import hashlib
import time
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
import arena4g_ref as R
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

DEV = "cuda"
BOUNDARY = 1 << 32
SIZE = BOUNDARY + (64 << 20)
SLICE = 256 << 20
GUARD = 256
DATA_SHIFT = 32 << 20  # chunk_frame_open's data_out: a second region of the output arena
FILL = 0x5A
PAT = 0x5A5A5A5A5A5A5A5A
KINDS = ("PerLane", "RunStaged", "LineStaged", "Lockstep", "Stream")
K = R.K_PERIOD
EDGE_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4096 + 44, 64 * 16 * 5 - 1)


class Arenas:
    """The module's input and output arena, each SIZE bytes between two GUARD-byte guards."""

    def __init__(self):
        import torch
        if DEV == "cuda":
            free = torch.cuda.mem_get_info()[0]
            assert free >= 12 << 30, f"the 4 GiB arena tests need 12 GiB of free device memory, have {free} bytes"
        self.in_big = torch.empty(SIZE + 2 * GUARD, dtype=torch.uint8, device=DEV)
        self.out_big = torch.empty(SIZE + 2 * GUARD, dtype=torch.uint8, device=DEV)
        self.inp = self.in_big[GUARD:GUARD + SIZE]
        self.out = self.out_big[GUARD:GUARD + SIZE]

    def fill_out(self):
        self.out_big.fill_(FILL)

    def assert_fill(self, what, lo=0):
        """Every byte of the output arena from offset lo on, and both guards, is FILL (the caller
        has refilled the ranges it owns).  lo must be a multiple of 8."""
        import torch
        words = self.out_big.view(torch.int64)
        start, step = (GUARD + lo) // 8, SLICE // 8
        bad = torch.zeros((), dtype=torch.int64, device=DEV)
        bad += torch.count_nonzero(words[:GUARD // 8] != PAT)
        for a in range(start, words.numel(), step):
            bad += torch.count_nonzero(words[a:a + step] != PAT)
        if int(bad):
            first = None
            for a in [0] + list(range(start, words.numel(), step)):
                b = GUARD // 8 if a == 0 else a + step
                hit = torch.nonzero(self.out_big[8 * a:8 * b] != FILL)
                if hit.numel():
                    first = 8 * a + int(hit[0]) - GUARD
                    break
            raise AssertionError(f"{what}: {int(bad)} 8-byte words outside the named records were written; first "
                                 f"byte at arena offset {first} ({first:#x}; 2^32 {first - BOUNDARY:+d})")


@pytest.fixture(scope="module")
def enet():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ephemeralnet_amd as E
    E.lib()
    t0 = time.time()
    yield E
    E.set_seg_min(-1)
    E.set_lanes_per_record(0)
    E.set_staging(-1)
    E.set_duplex_split(-1)
    E.set_host_hash_min(-1)
    print(f"\n[arena 4 GiB] module wall time {time.time() - t0:.1f} s, peak device memory "
          f"{torch.cuda.max_memory_allocated() / 2**30:.2f} GiB")


@pytest.fixture(scope="module")
def arenas(enet):
    import torch
    torch.cuda.reset_peak_memory_stats()
    a = Arenas()
    yield a
    del a.inp, a.out, a.in_big, a.out_big
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def timed(request):
    t0 = time.time()
    yield
    print(f"\n[arena 4 GiB] {request.node.name}: {time.time() - t0:.2f} s")


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to(DEV)


def routed(enet, want_route, want_seg, tag, fn, *a, **kw):
    """One batch call; what it adds to record_route_counts() and seg_batches() must be as given."""
    r0, s0 = enet.record_route_counts(), enet.seg_batches()
    fn(*a, **kw)
    r1, s1 = enet.record_route_counts(), enet.seg_batches()
    delta = {k: r1[k] - r0[k] for k in KINDS}
    assert delta == dict(dict.fromkeys(KINDS, 0), **want_route), (tag, fn.__name__, delta, want_route)
    assert s1 - s0 == want_seg, (tag, fn.__name__, "seg_batches moved by", s1 - s0)


# ================================================================== A. sparse
def spans(offs, named):
    """The named records' ranges [offs[i], offs[i+1]), merged where they touch: (lo, hi, records)."""
    out = []
    for i in sorted((i for i in named if offs[i + 1] > offs[i]), key=lambda i: int(offs[i])):
        lo, hi = int(offs[i]), int(offs[i + 1])
        if out and out[-1][1] == lo:
            out[-1] = (out[-1][0], hi, out[-1][2] + [i])
        else:
            assert not out or out[-1][1] < lo, "named records overlap"
            out.append((lo, hi, [i]))
    return out


def image(offs, span, parts, flips=()):
    lo, hi, recs = span
    img = np.full(hi - lo, FILL, dtype=np.uint8)
    for i in recs:
        img[int(offs[i]) - lo:int(offs[i + 1]) - lo] = parts[i]
    for i, pos, bit in flips:
        if i in recs:
            img[int(offs[i]) - lo + pos] ^= bit
    return img


def place(arena, offs, named, parts, flips=()):
    for sp in spans(offs, named):
        arena[sp[0]:sp[1]].copy_(dev(image(offs, sp, parts, flips)))


def check_ranges(A, offs, named, parts, what, shift=0):
    """The named records' ranges of the output arena (moved up by `shift` bytes) hold `parts`;
    they are refilled afterwards."""
    for sp in spans(offs, named):
        lo, hi, recs = sp
        got, want = A.out[shift + lo:shift + hi].cpu().numpy(), image(offs, sp, parts)
        d = np.flatnonzero(got != want)
        if d.size:
            at = lo + int(d[0])
            rec = next(i for i in recs if offs[i] <= at < offs[i + 1])
            raise AssertionError(f"{what}: first wrong byte at arena offset {at} ({at:#x}; 2^32 {at - BOUNDARY:+d}), "
                                 f"byte {at - int(offs[rec])} of record {rec} ({int(offs[rec + 1] - offs[rec])} bytes): "
                                 f"got {int(got[d[0]]):#x}, want {int(want[d[0]]):#x}; {d.size} bytes differ")
        A.out[shift + lo:shift + hi].fill_(FILL)


def check_out(A, offs, named, parts, what):
    """The named records of the output arena hold `parts`; nothing else in the arena was written."""
    check_ranges(A, offs, named, parts, what)
    A.assert_fill(what)


def small(n_items, width):
    """A sibling array (tags, verdicts, digests) of n items between two guards, all FILL."""
    import torch
    big = torch.full((n_items * width + 2 * GUARD,), FILL, dtype=torch.uint8, device=DEV)
    return big, big[GUARD:GUARD + n_items * width]


def check_small(big, want_rows, named, what, free=()):
    """Rows of the named items as given (those in `free`: any value), every other byte (guards
    included) still FILL."""
    n_items, width = want_rows.shape
    want = np.full((n_items, width), FILL, dtype=np.uint8)
    want[named] = want_rows[named]
    h = big.cpu().numpy()
    assert (h[:GUARD] == FILL).all() and (h[-GUARD:] == FILL).all(), f"{what}: guard bytes overwritten"
    got = h[GUARD:-GUARD].reshape(n_items, width)
    want[list(free)] = got[list(free)]
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: item {int(bad[0])} is {got[bad[0]].tolist()}, want {want[bad[0]].tolist()}; " \
                          f"{bad.size} items differ"


def run_sparse(enet, A, ref, t_in, t_out, named, *, order=None, ops=("xor", "seal", "open", "tamper"),
               inplace=False, hints=None, want_route, want_seg=0, tag, tag_victim=None, ct_victim=None):
    """The cipher calls over the named records of a table: ChaCha20 reads through t_in and writes
    through t_out; seal, open and the tampered open (tag_victim: one tag bit flipped; ct_victim =
    (record, byte): one ciphertext bit flipped; both come back ok = 0 and zeroed, every other named
    record intact) use t_in for both sides.  order None: the table is the batch."""
    import torch
    N = ref.n
    lens = ref.lens
    named = list(named)
    if hints is None:
        hints = dict(total_bytes_hint=sum(lens[i] for i in named), max_len_hint=max(lens[i] for i in named))
    d_in, d_out = dev(t_in), dev(t_out)
    keys, nonces, aad, aoff = dev(ref.keys), dev(ref.nonces), dev(ref.aad if ref.aad.size else np.zeros(1, np.uint8)), dev(ref.aoff)
    tord = None if order is None else torch.tensor(order, dtype=torch.int32, device=DEV)
    src = A.out if inplace else A.inp

    def batch(table):
        return enet.Batch(src, table, keys, nonces, order=tord, count=None if order is None else len(order), **hints)

    go = lambda fn, *a, **kw: routed(enet, want_route, want_seg, tag, fn, *a, **kw)
    ones = np.ones((N, 1), dtype=np.uint8)
    if "xor" in ops:
        A.fill_out()
        place(src, t_in, named, ref.pt)
        go(enet.chacha20_xor, batch(d_in), A.out, dev(ref.ctr.view(np.int32)), out_offsets=d_out)
        check_out(A, t_out, named, ref.xo, f"{tag} chacha20 xor")
    if "seal" in ops:
        A.fill_out()
        place(src, t_in, named, ref.pt)
        tbig, tags = small(N, 16)
        go(enet.aead_seal, batch(d_in), A.out, tags, aad, aoff)
        check_small(tbig, ref.tags, named, f"{tag} seal tags")
        check_out(A, t_in, named, ref.ct, f"{tag} seal ciphertext")
    if "open" in ops:
        A.fill_out()
        place(src, t_in, named, ref.ct)
        obig, ok = small(N, 1)
        go(enet.aead_open, batch(d_in), A.out, dev(ref.tags), ok, aad, aoff)
        check_small(obig, ones, named, f"{tag} open verdicts")
        check_out(A, t_in, named, ref.pt, f"{tag} open plaintext")
    if "tamper" in ops:
        v, pos = ct_victim
        assert tag_victim in named and v in named and v != tag_victim and 0 <= pos < lens[v]
        A.fill_out()
        place(src, t_in, named, ref.ct, flips=[(v, pos, 0x20)])
        bad_tags = dev(ref.tags)
        bad_tags[tag_victim, 5] ^= 0x08
        obig, ok = small(N, 1)
        go(enet.aead_open, batch(d_in), A.out, bad_tags, ok, aad, aoff)
        want_ok, want_pt = ones.copy(), list(ref.pt)
        for f in (tag_victim, v):
            want_ok[f] = 0
            want_pt[f] = np.zeros(lens[f], dtype=np.uint8)
        check_small(obig, want_ok, named, f"{tag} tampered open verdicts")
        check_out(A, t_in, named, want_pt, f"{tag} tampered open plaintext")


# two records below 2^32, record 2 at it, the edge lengths above
LENS_HB = (1500, 65537, 4096 + 44, 64 * 16 * 5 - 1) + EDGE_LENS[:14]
K_HB = 2
# the split tables' groups (arena4g_ref.split_tables): C around and above 2^32, A below, B moving
LENS_C = (4096 + 44, 64 * 16 * 5 - 1) + EDGE_LENS[:14] + (1500, 65537)
LENS_A = LENS_C[:8]
LENS_B = (129, 65537, 1500, 1025)


@pytest.mark.parametrize("P", [1, 4, 16])
def test_sparse_records_per_lane(enet, arenas, P):
    """A.1 on the per-lane record kernel at P lanes per record: ChaCha20 with start counters whose
    u32 wrap falls inside the records, seal with AAD lengths 0, 1, 16, 17, open, and an open with one
    tampered tag and one tampered ciphertext byte -- high base (cut and straddle), high base in
    place, and split with a mixed order."""
    enet.set_seg_min(-1)
    enet.set_staging(-1)
    enet.set_lanes_per_record(P)
    ref = R.records_ref(LENS_HB, 820000)
    n = ref.n
    for mode in ("cut", "straddle"):
        offs = R.high_base_offsets(LENS_HB, K_HB, BOUNDARY, mode)
        role = R.boundary_roles(offs, BOUNDARY)
        assert role == (dict(ends=[1], straddles=[], starts=[2]) if mode == "cut" else dict(ends=[], straddles=[2], starts=[]))
        assert offs[0] > 0 and offs[-1] < SIZE and (mode == "cut" or offs[2] % 4 == 3)
        # tampered: the straddling / first-above record's last partial block; the tag of the 64 KiB + 1 record
        kw = dict(want_route={"PerLane": n}, tag_victim=1, ct_victim=(2, LENS_HB[2] - 3))
        run_sparse(enet, arenas, ref, offs, offs, range(n), tag=f"P {P} high base {mode}", **kw)
        run_sparse(enet, arenas, ref, offs, offs, range(n), inplace=True, tag=f"P {P} high base {mode} in place", **kw)
    s = R.split_tables(LENS_A, LENS_B, LENS_C, BOUNDARY)
    sref = R.records_ref(s.lens, 821000)
    order = R.mixed_order(s.named, 821001)
    assert max(order) >= len(order) and s.straddle[-1] < SIZE and s.cut[-1] < SIZE
    assert R.boundary_roles(s.cut, BOUNDARY, s.named) == dict(ends=[s.B[-1]], straddles=[], starts=[s.C[0]])
    assert R.boundary_roles(s.straddle, BOUNDARY, s.named) == dict(ends=[], straddles=[s.C[0]], starts=[])
    assert len(R.aliases(s.cut, BOUNDARY, s.named)) >= 5 and len(R.aliases(s.straddle, BOUNDARY, s.named)) >= 1
    kw = dict(order=order, want_route={"PerLane": len(order)}, tag_victim=s.C[-1], ct_victim=(s.C[0], LENS_C[0] - 3))
    # group B reads above 2^32 and writes below it, then the reverse
    run_sparse(enet, arenas, sref, s.cut, s.straddle, s.named, ops=("xor",), tag=f"P {P} split cut -> straddle", **kw)
    run_sparse(enet, arenas, sref, s.straddle, s.cut, s.named, ops=("xor",), tag=f"P {P} split straddle -> cut", **kw)
    run_sparse(enet, arenas, sref, s.cut, s.cut, s.named, ops=("seal", "tamper"), tag=f"P {P} split cut", **kw)
    run_sparse(enet, arenas, sref, s.straddle, s.straddle, s.named, ops=("seal", "open", "tamper"),
               tag=f"P {P} split straddle", **kw)
    enet.set_lanes_per_record(0)


# kind, staging, lanes, L, bytes of the batch below 2^32: inside the second workgroup's records and
# inside a record, at an address = 0 mod 4 (line staging wants 4-byte-aligned starts)
STAGED = [
    ("Stream", -1, 2, 4096, 256 * 4096 + 100 * 4096 + 2052),
    ("Lockstep", -1, 2, 4160, 256 * 4160 + 100 * 4160 + 2052),
    ("LineStaged", -1, 1, 1500, 256 * 1500 + 100 * 1500 + 752),
    ("RunStaged", 4, 1, 1500, 256 * 1500 + 100 * 1500 + 752),
]


@pytest.mark.parametrize("kind,staging,P,L,below", STAGED, ids=[s[0] for s in STAGED])
def test_staged_kinds_with_a_high_base(enet, arenas, kind, staging, P, L, below):
    """A.2: 1024 uniform records whose table starts at 2^32 - below: four whole workgroups of the
    staged kernel (256 records each at these lane counts), 2^32 inside record 356 of the second one.
    The kernels' own offsets stay small; the base they add them to is what crosses 2^32.  The same
    batch with an order (reversed) runs per lane."""
    n = 1024
    enet.set_seg_min(-1)
    enet.set_lanes_per_record(P)
    enet.set_staging(staging)
    ref = R.records_ref((L,) * n, 830000 + L + staging)
    offs = (BOUNDARY - below + L * np.arange(n + 1)).astype(np.int64)
    assert offs[256] < BOUNDARY < offs[512] and offs[356] < BOUNDARY < offs[357] and offs[0] % 4 == 0
    hints = dict(total_bytes_hint=n * L, max_len_hint=L)
    kw = dict(hints=hints, tag_victim=356, ct_victim=(511, L - 1))
    run_sparse(enet, arenas, ref, offs, offs, range(n), want_route={kind: n}, tag=f"{kind} high base", **kw)
    run_sparse(enet, arenas, ref, offs, offs, range(n), want_route={kind: n}, inplace=True, ops=("seal", "xor"),
               tag=f"{kind} high base in place", **kw)
    run_sparse(enet, arenas, ref, offs, offs, range(n), order=list(range(n))[::-1], want_route={"PerLane": n},
               ops=("seal", "tamper"), tag=f"{kind} shape, reversed order", **kw)
    enet.set_staging(-1)
    enet.set_lanes_per_record(0)


def test_tiles_plan_route_across_the_boundary(enet, arenas):
    """A.5: records of 256 KiB + 100, 1 MiB and 3 * 65 536 - 1 bytes under a tile threshold of
    64 KiB, the 1 MiB record starting 5 * 65 536 + 5 bytes below 2^32 (= 3 mod 4): its sixth 64 KiB
    tile straddles 2^32, the first record lies below and the third above; also with the cut at 2^32
    between the first two.  Plan + tiles: one more seg_batches() per call."""
    lens = ((256 << 10) + 100, 1 << 20, 3 * 65536 - 1)
    ref = R.records_ref(lens, 840000)
    enet.set_lanes_per_record(0)
    enet.set_staging(-1)
    enet.set_seg_min(65536)
    for mode, below in (("straddle", 5 * 65536 + 5), ("cut", 0)):
        offs = R.high_base_offsets(lens, 1, BOUNDARY, mode, below=below)
        if mode == "straddle":
            assert offs[1] % 4 == 3 and offs[1] + 5 * 65536 < BOUNDARY < offs[1] + 6 * 65536
        kw = dict(want_route={"PerLane": 3}, want_seg=1, tag_victim=1, ct_victim=(2, 70000))
        run_sparse(enet, arenas, ref, offs, offs, range(3), tag=f"plan + tiles {mode}", **kw)
        run_sparse(enet, arenas, ref, offs, offs, range(3), inplace=True, ops=("xor", "seal"),
                   tag=f"plan + tiles {mode} in place", **kw)
    enet.set_seg_min(-1)


def test_tiles_uniform_routes_across_the_boundary(enet, arenas):
    """A.5: four uniform 1 MiB records on the one-launch uniform tile routes (ChaCha20: uniform xor;
    seal / open: uniform AEAD), the table starting 1.5 MiB + 5 bytes below 2^32: the second
    record's ninth tile straddles it."""
    L, n = 1 << 20, 4
    ref = R.records_ref((L,) * n, 841000)
    enet.set_lanes_per_record(0)
    enet.set_staging(-1)
    enet.set_seg_min(-1)
    offs = R.high_base_offsets((L,) * n, 1, BOUNDARY, "straddle", below=(1 << 19) + 5)
    assert offs[1] + 8 * 65536 < BOUNDARY < offs[1] + 9 * 65536
    kw = dict(hints=dict(total_bytes_hint=n * L, max_len_hint=L), want_route={}, want_seg=1,
              tag_victim=1, ct_victim=(2, L - 1))
    run_sparse(enet, arenas, ref, offs, offs, range(n), tag="uniform tiles", **kw)
    run_sparse(enet, arenas, ref, offs, offs, range(n), inplace=True, ops=("xor", "seal"), tag="uniform tiles in place", **kw)


# ------------------------------------------------------------------ A.4 hashes
SHA_LENS = (0, 1, 55, 56, 63, 64, 65, 119, 120, 4096, 65537)
KEY_LENS = (0, 32, 64, 65, 100)


def test_hashes_with_message_offsets_past_the_boundary(enet, arenas):
    """A.4: SHA-256, HMAC-SHA256 and its verify over 330 messages (more than one 256-thread
    workgroup) whose offsets start at 2^32 - 100: the padding-edge lengths, 4096 and 65 537 bytes,
    keys of 0, 32, 64, 65 and 100 bytes; digests against hashlib, MACs against the oracle; one
    corrupted MAC in the second workgroup."""
    import torch
    n = 330
    lens = [SHA_LENS[i % len(SHA_LENS)] for i in range(n)]
    offs = (BOUNDARY - 100 + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    assert offs[0] < BOUNDARY < offs[-1] < SIZE
    assert any(offs[i] < BOUNDARY < offs[i + 1] for i in range(n))
    msgs = [splitmix_bytes(850000 + i, lens[i]) for i in range(n)]
    klens = [KEY_LENS[(i // 3) % len(KEY_LENS)] for i in range(n)]
    keys = [splitmix_bytes(851000 + i, klens[i]) for i in range(n)]
    assert {(lens[i], klens[i]) for i in range(n)} >= {(L, kl) for L in (0, 64, 65537) for kl in KEY_LENS}
    koffs = np.concatenate([[0], np.cumsum(klens)]).astype(np.int64)
    lo, hi = int(offs[0]), int(offs[-1])
    arenas.inp[lo:hi].copy_(dev(np.frombuffer(b"".join(msgs), dtype=np.uint8)))
    t_off, t_koff, karena = dev(offs), dev(koffs), dev(np.frombuffer(b"".join(keys), dtype=np.uint8))
    rows = lambda parts: np.frombuffer(b"".join(parts), dtype=np.uint8).reshape(n, 32)
    everyone = list(range(n))

    big, dig = small(n, 32)
    enet.sha256(arenas.inp, t_off, dig)
    check_small(big, rows([hashlib.sha256(m).digest() for m in msgs]), everyone, "sha256 digests")
    want = rows([oracle.hmac_sha256(k, m) for k, m in zip(keys, msgs)])
    big, macs = small(n, 32)
    enet.hmac_sha256(karena, arenas.inp, t_off, macs, key_offsets=t_koff)
    check_small(big, want, everyone, "hmac macs")
    victim = 300
    macs[32 * victim + 31] ^= 0x80
    big, ok = small(n, 1)
    enet.hmac_sha256_verify(karena, arenas.inp, t_off, macs, ok, key_offsets=t_koff)
    want_ok = np.ones((n, 1), dtype=np.uint8)
    want_ok[victim] = 0
    check_small(big, want_ok, everyone, "hmac verify verdicts")
    # fixed 32-byte keys (key_offsets NULL), the other entry of the same kernel
    k32 = splitmix_bytes(852000, 32 * n)
    want = rows([oracle.hmac_sha256(k32[32 * i:32 * i + 32], msgs[i]) for i in range(n)])
    big, macs = small(n, 32)
    enet.hmac_sha256(dev(np.frombuffer(k32, dtype=np.uint8)), arenas.inp, t_off, macs)
    check_small(big, want, everyone, "hmac macs, 32-byte keys")


# ================================================================== B. dense
def tile_block(dst, blk, n, width):
    """dst[: n * width] = the periodic array of the K-item block blk (device tensors)."""
    for lo, hi, rows in R.periodic_slices(n, K, width, 1 << 62):
        if rows:
            dst[lo:hi].view(rows, K * width).copy_(blk.unsqueeze(0).expand(rows, K * width))
        else:
            dst[lo:hi].copy_(blk[:hi - lo])


def assert_periodic(arr, blk, n, width, what):
    """arr[: n * width] (device) is the periodic array of blk, compared in slices of <= 256 MiB, as
    32-bit words (every width here is a multiple of 4): the mismatch count stays a small temporary."""
    import torch
    assert width % 4 == 0
    pieces = R.periodic_slices(n, K, width, SLICE)
    b32 = blk.view(torch.int32)
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    for lo, hi, rows in pieces:
        a32 = arr[lo:hi].view(torch.int32)
        bad += torch.count_nonzero(a32.view(rows, -1) != b32 if rows else a32 != b32[:(hi - lo) // 4])
    if int(bad) == 0:
        return
    for lo, hi, rows in pieces:
        want = blk.unsqueeze(0).expand(rows, blk.numel()).reshape(-1) if rows else blk[:hi - lo]
        hit = torch.nonzero(arr[lo:hi] != want)
        if hit.numel():
            at = lo + int(hit[0])
            raise AssertionError(f"{what}: first wrong byte {at} ({at:#x}; 2^32 {at - BOUNDARY:+d}), byte {at % width} "
                                 f"of item {at // width} (item {at // width % K} of the period): got "
                                 f"{int(arr[at]):#x}, want {int(want[at - lo]):#x}; {int(bad)} 32-bit words differ")


def per_wg(kind, P):
    return (256 if kind in ("LineStaged", "RunStaged") else 512) // P


# L, lanes, n, kind, in place too, (full workgroups, rest) where the route table pins them
DENSE = [
    (4096, 2, (1 << 20) - 1, "Stream", True, (4095, 255)),
    (4096, 2, (1 << 20) + 300, "Lockstep", False, None),
    (65536, 16, 65535, "Stream", False, None),
    (65536, 16, 65536 + 40, "Lockstep", True, None),
    (1500, 1, 2863311, "LineStaged", True, (11184, 207)),
    (1500, 1, 2863312 + 600, "Lockstep", False, None),
]


def dense_batch(enet, blk, n, L, hinted=True):
    """Device arrays of the n-record periodic batch (everything but the arenas)."""
    import torch
    reps = n // K + 1
    i = torch.arange(n + 1, dtype=torch.int64, device=DEV)
    offs = i * L
    a_blk = dev(blk.aoff)
    aoff = (i // K) * int(blk.aoff[K]) + a_blk[i % K]
    return dict(offs=offs, keys=dev(blk.keys).repeat(reps, 1)[:n].contiguous(),
                nonces=dev(blk.nonces).repeat(reps, 1)[:n].contiguous(),
                ctr=dev(blk.ctr.view(np.int32)).repeat(reps)[:n].contiguous(),
                aad=dev(blk.aad).repeat(reps + 1), aoff=aoff,
                hints=dict(total_bytes_hint=n * L, max_len_hint=L) if hinted else dict(total_bytes_hint=0, max_len_hint=0))


def run_dense(enet, A, L, P, n, want_route, inplace, seed, hinted=True, ops=("xor", "seal", "open")):
    import torch
    assert ((1 << 32) // L) % K != 0 and n * L + 8 <= SIZE
    blk = R.periodic_block(L, seed)
    b = dense_batch(enet, blk, n, L, hinted)
    pt, ct, xo, tg = dev(blk.pt), dev(blk.ct), dev(blk.xo), dev(blk.tags)
    enet.set_seg_min(-1)
    enet.set_staging(-1)
    enet.set_lanes_per_record(P)
    tail = (n * L + 7) // 8 * 8  # the scan of the untouched rest starts at the next 8-byte word
    tag = f"L {L} P {P} n {n}" + ("" if hinted else " hints 0/0")
    go = lambda fn, *a: routed(enet, want_route, 0, tag, fn, *a)
    batch = lambda arena: enet.Batch(arena, b["offs"], b["keys"], b["nonces"], **b["hints"])

    def rest_untouched(what):
        assert bool((A.out[n * L:tail] == FILL).all()), f"{what}: bytes behind the last record written"
        A.assert_fill(what, lo=tail)

    tile_block(A.inp, pt, n, L)
    if "xor" in ops:
        A.fill_out()
        go(enet.chacha20_xor, batch(A.inp), A.out, b["ctr"])
        assert_periodic(A.out, xo, n, L, f"{tag} chacha20 xor")
        rest_untouched(f"{tag} chacha20 xor")
    if "seal" in ops:
        A.fill_out()
        tbig, tags = small(n, 16)
        go(enet.aead_seal, batch(A.inp), A.out, tags, b["aad"], b["aoff"])
        assert_periodic(A.out, ct, n, L, f"{tag} seal ciphertext")
        assert_periodic(tags, tg, n, 16, f"{tag} seal tags")
        assert bool((tbig[:GUARD] == FILL).all()) and bool((tbig[-GUARD:] == FILL).all()), f"{tag} tag guards"
        rest_untouched(f"{tag} seal")
    if "open" in ops:
        # the sealed arena back into the input arena, one tag of the last whole workgroup tampered
        kind = next((k for k in want_route if k != "PerLane"), "PerLane")
        whole = want_route.get(kind, 0) if kind != "PerLane" else n
        v = whole - 4
        assert "seal" in ops and 0 <= v < n
        tags[16 * v + 9] ^= 0x01
        A.in_big.fill_(FILL)
        obig, ok = small(n, 1)
        go(enet.aead_open, batch(A.out), A.inp, tags, ok, b["aad"], b["aoff"])
        want_ok = torch.ones(n, dtype=torch.uint8, device=DEV)
        want_ok[v] = 0
        miss = torch.nonzero(ok != want_ok)
        assert miss.numel() == 0, f"{tag} open verdicts: record {int(miss[0])} has {int(ok[int(miss[0])])}; {miss.numel()} wrong"
        assert bool((obig[:GUARD] == FILL).all()) and bool((obig[-GUARD:] == FILL).all()), f"{tag} verdict guards"
        assert not bool(A.inp[v * L:(v + 1) * L].any()), f"{tag} tampered record {v} not zeroed"
        A.inp[v * L:(v + 1) * L].copy_(pt[(v % K) * L:(v % K + 1) * L])
        assert_periodic(A.inp, pt, n, L, f"{tag} open plaintext")
        assert bool((A.inp[n * L:n * L + 4096] == FILL).all()) and bool((A.in_big[:GUARD] == FILL).all()), \
            f"{tag} open: bytes outside the records written"
    if inplace:
        tile_block(A.out, pt, n, L)
        A.out_big[:GUARD].fill_(FILL)
        A.out[n * L:].fill_(FILL)
        tbig, tags = small(n, 16)
        src = enet.Batch(A.out, b["offs"], b["keys"], b["nonces"], **b["hints"])
        go(enet.aead_seal, src, A.out, tags, b["aad"], b["aoff"])
        assert_periodic(A.out, ct, n, L, f"{tag} in-place seal ciphertext")
        assert_periodic(tags, tg, n, 16, f"{tag} in-place seal tags")
        rest_untouched(f"{tag} in-place seal")
    enet.set_lanes_per_record(0)


@pytest.mark.parametrize("L,P,n,kind,inplace,pinned", DENSE, ids=[f"L{c[0]}_n{c[2]}_{c[3]}" for c in DENSE])
def test_dense_uniform_batch_at_the_routing_limit(enet, arenas, L, P, n, kind, inplace, pinned):
    """B: the whole arena of a uniform batch whose L n is the last below (Stream, LineStaged: their
    last workgroup ends under the 32-bit limit) or the first shapes above 2^32 (Lockstep: its
    workgroups run on both sides), at default staging: ChaCha20, seal, open of the sealed arena with
    one tampered tag in the last whole workgroup, and for one case of each pair a seal in place."""
    full = n // per_wg(kind, P)
    rest = n - full * per_wg(kind, P)
    if pinned:
        assert (full, rest) == pinned
    assert (L * n <= 0xFFFFFFFF) == (kind != "Lockstep")
    route = {kind: full * per_wg(kind, P)}
    if rest:
        route["PerLane"] = rest
    run_dense(enet, arenas, L, P, n, route, inplace, 860000 + L)


def test_dense_unhinted_batch_runs_per_lane_past_the_boundary(enet, arenas):
    """B: the first 4096-byte shape above 2^32 once more with hints 0 / 0: the per-lane record kernel
    over every record, 300 of them past 2^32."""
    n = (1 << 20) + 300
    run_dense(enet, arenas, 4096, 2, n, {"PerLane": n}, False, 860000 + 4096, hinted=False, ops=("xor", "seal"))


# ================================================================== A.3 hash + cipher calls
# groups of the split tables (arena4g_ref.split_tables); the same records, back to back with the
# two empty filler records among them, are the high-base batch (record HB_K at 2^32)
DUP_C = (4096 + 44, 65537, 0, 1, 1500, 65536, 129, 64 * 16 * 5 - 1)
DUP_A = DUP_C[:4]
DUP_B = (64, 1025, 300, 1500)
SESS = 5
WAYS = {"duplex": (-1, 0), "duplex_split": (-1, 1), "two_pass": (0, -1)}  # set_staging, set_duplex_split


def rows_of(parts, width):
    return np.frombuffer(b"".join(parts), dtype=np.uint8).reshape(len(parts), width)


def u8(b):
    return np.frombuffer(b, dtype=np.uint8)


@pytest.fixture(scope="module")
def world():
    return make_world()


def make_world():
    """The records of the A.3 calls and everything the oracle says about them, indexed like the
    split tables (the two fillers are empty records of their own)."""
    s = R.split_tables(DUP_A, DUP_B, DUP_C, BOUNDARY)
    lens, n = s.lens, len(s.lens)
    w = SimpleNamespace(s=s, lens=lens, n=n, hb_k=s.C[0])
    w.msgs = [splitmix_bytes(870000 + i, L) for i, L in enumerate(lens)]
    w.keys = [splitmix_bytes(871000 + i, 32) for i in range(n)]
    w.nonces = [splitmix_bytes(872000 + i, 12) for i in range(n)]
    w.table = [splitmix_bytes(873000 + j, 32) for j in range(SESS)]
    w.sess = [(3 * i + 1) % SESS for i in range(n)]
    w.ids = [(b"\xff\xff\xff\xff" if i % 3 == 0 else b"") + splitmix_bytes(874000 + i, 32)[4 if i % 3 == 0 else 0:]
             for i in range(n)]
    w.macs = [oracle.hmac_sha256(k, m) for k, m in zip(w.keys, w.msgs)]
    w.bodies = [oracle.frame_seal(k, nn, m) for k, nn, m in zip(w.keys, w.nonces, w.msgs)]
    wire = lambda nn, body: nn + len(body).to_bytes(4, "big") + body
    w.wires = [wire(nn, b) for nn, b in zip(w.nonces, w.bodies)]
    w.swires = [wire(w.nonces[i], oracle.frame_seal(w.table[w.sess[i]], w.nonces[i], w.msgs[i])) for i in range(n)]
    w.smacs = [oracle.hmac_sha256(w.table[w.sess[i]], w.msgs[i]) for i in range(n)]
    sealed = [oracle.aead_seal(k, nn, m) for k, nn, m in zip(w.keys, w.nonces, w.msgs)]
    w.ct, w.tags = [c for c, _ in sealed], [t for _, t in sealed]
    w.hashes = [hashlib.sha256(m).digest() for m in w.msgs]
    w.chunk_ct = [oracle.chacha20_xor(w.keys[i], w.nonces[i], w.msgs[i], oracle.derive_counter(w.ids[i])) for i in range(n)]
    w.chunk_ct_own = [oracle.chacha20_xor(w.keys[i], w.nonces[i], w.msgs[i], oracle.derive_counter(w.hashes[i])) for i in range(n)]
    return w


def grow(lens_tuple, by):
    return tuple(L + by for L in lens_tuple)


def placements(w, in_by, out_by):
    """(tag, input table, output table, named, order) of the records with in_by / out_by bytes
    added to every record's length: high base both ways round (every record of the table, the two
    fillers as empty messages), then split both ways round (the fillers unnamed and huge)."""
    s = w.s
    lens_in, lens_out = [L + in_by for L in w.lens], [L + out_by for L in w.lens]
    everyone = list(range(w.n))
    for a, b in (("cut", "straddle"), ("straddle", "cut")):
        yield (f"high base {a} -> {b}", R.high_base_offsets(lens_in, w.hb_k, BOUNDARY, a),
               R.high_base_offsets(lens_out, w.hb_k, BOUNDARY, b), everyone, None)
    si = R.split_tables(grow(DUP_A, in_by), grow(DUP_B, in_by), grow(DUP_C, in_by), BOUNDARY)
    so = R.split_tables(grow(DUP_A, out_by), grow(DUP_B, out_by), grow(DUP_C, out_by), BOUNDARY)
    order = R.mixed_order(s.named, 875000)
    yield "split cut -> straddle", si.cut, so.straddle, s.named, order
    yield "split straddle -> cut", si.straddle, so.cut, s.named, order


def one_table_placements(w):
    """The placements of the calls that take one offsets table for both arenas."""
    for tag, t_in, _, named, order in placements(w, 0, 0):
        yield tag.split(" ->")[0], t_in, t_in, named, order


def run_io(enet, A, w, way, tag, t_in, in_parts, t_out, out_parts, named, order, launch, *, keys=None, nonces=True,
           smalls=(), flips=(), per_lane=None):
    """One hash + cipher call: the named records' inputs placed through t_in, everything else of
    the call's outputs prefilled; launch(batch, out arena, device output table, *sibling arrays).
    smalls: (rows the call must leave, width, rows whose value is not pinned) per sibling array.
    per_lane: records the call hands to the per-lane record kernel on the two-pass path (None: as
    many as named); the duplex kernels move no route counter."""
    import torch
    named = list(named)
    in_lens = [len(in_parts[i]) for i in range(w.n)]
    hints = dict(total_bytes_hint=sum(in_lens[i] for i in named), max_len_hint=max(in_lens[i] for i in named))
    tord = None if order is None else torch.tensor(order, dtype=torch.int32, device=DEV)
    A.fill_out()
    place(A.inp, t_in, named, [u8(p) for p in in_parts], flips)
    d_keys = dev(rows_of(w.keys if keys is None else keys, 32))
    b = enet.Batch(A.inp, dev(t_in), d_keys, dev(rows_of(w.nonces, 12)) if nonces else None, order=tord,
                   count=None if order is None else len(order), **hints)
    bufs = [small(w.n, width) for _, width, _ in smalls]
    staging, split = WAYS[way]
    enet.set_staging(staging)
    enet.set_duplex_split(split)
    route = {"PerLane": len(named) if per_lane is None else per_lane} if way == "two_pass" or per_lane is not None else {}
    try:
        routed(enet, route, 0, f"{tag} {way}", launch, b, A.out, dev(t_out), *[v for _, v in bufs])
    finally:
        enet.set_staging(-1)
        enet.set_duplex_split(-1)
    for (big, _), (rows, width, free) in zip(bufs, smalls):
        check_small(big, rows, named, f"{tag} {way} sibling array of width {width}", free)
    check_out(A, t_out, named, [u8(p) for p in out_parts], f"{tag} {way}")


def zeroed(parts, failed):
    return [bytes(len(p)) if i in failed else p for i, p in enumerate(parts)]


def verdicts(n, failed):
    ok = np.ones((n, 1), dtype=np.uint8)
    ok[list(failed)] = 0
    return ok


@pytest.mark.parametrize("way", list(WAYS))
def test_frames_and_wire_frames_across_the_boundary(enet, arenas, world, way):
    """A.3: frame_seal / frame_open and wire_seal / wire_open (their outputs 32 / 48 bytes longer or
    shorter than their inputs, so the two tables differ record by record), every placement.  The
    opens carry a flipped body byte in the 64 KiB + 1 record and a flipped MAC byte in a short one
    (wire: also a flipped length field): ok = 0, zeroed, neighbours intact."""
    w = world
    s = w.s
    big_rec, short_rec, hdr_rec = s.C[1], s.B[1], s.C[4]
    for hdr, sealed, seal, open_ in ((0, w.bodies, enet.frame_seal, enet.frame_open),
                                     (16, w.wires, enet.wire_seal, enet.wire_open)):
        grow_by = 32 + hdr
        for tag, t_in, t_out, named, order in placements(w, 0, grow_by):
            run_io(enet, arenas, w, way, f"{seal.__name__} {tag}", t_in, w.msgs, t_out, sealed, named, order,
                   lambda b, out, d_out: seal(b, out, d_out))
        failed = {big_rec, short_rec} | ({hdr_rec} if hdr else set())
        flips = [(big_rec, hdr + 70, 0x04), (short_rec, hdr + w.lens[short_rec] + 31, 0x80)] + ([(hdr_rec, 14, 0x01)] if hdr else [])
        for tag, t_in, t_out, named, order in placements(w, grow_by, 0):
            run_io(enet, arenas, w, way, f"{open_.__name__} {tag}", t_in, sealed, t_out, zeroed(w.msgs, failed), named,
                   order, lambda b, out, d_out, macs, ok: open_(b, out, d_out, macs, ok), nonces=not hdr, flips=flips,
                   smalls=[(rows_of(w.macs, 32), 32, failed), (verdicts(w.n, failed), 1, ())])


def test_session_wire_frames_across_the_boundary(enet, arenas, world):
    """A.3: wire_seal_sessions / wire_open_sessions under a table of 5 session keys and its
    midstates (duplex kernel only: these calls have no two-pass path and no split form).  Seal: a
    session index past the table zeroes that frame's whole slot.  Open: a flipped body byte, a
    frame filed under another session and an index past the table give ok = 0 and zeros; the
    neighbours are intact."""
    import torch
    w, way = world, "duplex"
    s = w.s
    tbl = dev(rows_of(w.table, 32))
    mid = torch.zeros(16 * SESS, dtype=torch.int32, device=DEV)
    enet.hmac_midstates(tbl, SESS, mid)
    past, other, body = s.C[3], s.B[2], s.C[1]
    sess = np.array(w.sess, dtype=np.uint32)
    sess_seal = sess.copy()
    sess_seal[past] = SESS + 2
    for tag, t_in, t_out, named, order in placements(w, 0, 48):
        run_io(enet, arenas, w, way, f"wire_seal_sessions {tag}", t_in, w.msgs, t_out, zeroed(w.swires, {past}), named,
               order, lambda b, out, d_out: enet.wire_seal_sessions(b, out, d_out, dev(sess_seal.view(np.int32)), SESS, mid),
               keys=w.table + [bytes(32)] * (w.n - SESS))
    sess_open = sess.copy()
    sess_open[past] = 0xFFFFFFF0
    sess_open[other] = (sess_open[other] + 1) % SESS
    failed = {past, other, body}
    for tag, t_in, t_out, named, order in placements(w, 48, 0):
        run_io(enet, arenas, w, way, f"wire_open_sessions {tag}", t_in, w.swires, t_out, zeroed(w.msgs, failed), named,
               order, lambda b, out, d_out, macs, ok: enet.wire_open_sessions(b, out, d_out, dev(sess_open.view(np.int32)),
                                                                              SESS, mid, macs, ok),
               keys=w.table + [bytes(32)] * (w.n - SESS), nonces=False, flips=[(body, 16 + 4000, 0x10)],
               smalls=[(rows_of(w.smacs, 32), 32, failed), (verdicts(w.n, failed), 1, ())])


@pytest.mark.parametrize("way", list(WAYS))
def test_aead_hmac_across_the_boundary(enet, arenas, world, way):
    """A.3: aead_hmac_seal / aead_hmac_open, every placement; the open with a flipped ciphertext
    byte (Poly1305 rejects), a flipped MAC (HMAC rejects) and a flipped tag, one record each."""
    w = world
    s = w.s
    for tag, t_in, t_out, named, order in one_table_placements(w):
        run_io(enet, arenas, w, way, f"aead_hmac_seal {tag}", t_in, w.msgs, t_out, w.ct, named, order,
               lambda b, out, d_out, tags, macs: enet.aead_hmac_seal(b, out, tags, macs),
               smalls=[(rows_of(w.tags, 16), 16, ()), (rows_of(w.macs, 32), 32, ())])
    poly, mac, tg = s.C[1], s.B[3], s.C[5]
    failed = {poly, mac, tg}
    bad_tags, bad_macs = rows_of(w.tags, 16).copy(), rows_of(w.macs, 32).copy()
    bad_tags[tg, 0] ^= 1
    bad_macs[mac, 31] ^= 2
    for tag, t_in, t_out, named, order in one_table_placements(w):
        run_io(enet, arenas, w, way, f"aead_hmac_open {tag}", t_in, w.ct, t_out, zeroed(w.msgs, failed), named, order,
               lambda b, out, d_out, ok: enet.aead_hmac_open(b, out, dev(bad_tags), dev(bad_macs), ok),
               flips=[(poly, w.lens[poly] - 1, 0x01)], smalls=[(verdicts(w.n, failed), 1, ())])


@pytest.mark.parametrize("way", list(WAYS))
def test_chunk_store_and_fetch_across_the_boundary(enet, arenas, world, way):
    """A.3: chunk_store with ids given (counters from LE32(id), some 0xFFFFFFFF) and with ids
    derived from the content, chunk_fetch with one tampered chunk (ok = 0, zeroed)."""
    w = world
    s = w.s
    ids = dev(rows_of(w.ids, 32))
    bad = s.C[1]
    for tag, t_in, t_out, named, order in one_table_placements(w):
        run_io(enet, arenas, w, way, f"chunk_store {tag}", t_in, w.msgs, t_out, w.chunk_ct, named, order,
               lambda b, out, d_out, hashes: enet.chunk_store(b, out, hashes, chunk_ids=ids),
               smalls=[(rows_of(w.hashes, 32), 32, ())])
        run_io(enet, arenas, w, way, f"chunk_store, ids derived {tag}", t_in, w.msgs, t_out, w.chunk_ct_own, named, order,
               lambda b, out, d_out, hashes: enet.chunk_store(b, out, hashes), per_lane=len(named),
               smalls=[(rows_of(w.hashes, 32), 32, ())])
        run_io(enet, arenas, w, way, f"chunk_fetch {tag}", t_in, w.chunk_ct, t_out, zeroed(w.msgs, {bad}), named, order,
               lambda b, out, d_out, ok: enet.chunk_fetch(b, out, ids, dev(rows_of(w.hashes, 32)), ok),
               flips=[(bad, 65000, 0x08)], smalls=[(verdicts(w.n, {bad}), 1, ())])


def test_long_chunk_hashed_on_the_host_from_past_the_boundary(enet, arenas):
    """A.5: chunk_store / chunk_fetch of a 1 MiB + 3 chunk straddling 2^32 between two short ones,
    with the host-hash threshold forced down to 64 KiB: the host threads copy the long chunk from
    device offsets past 2^32 (csrc/chunk_hybrid.cpp), the device ciphers it on the tiles."""
    lens = (1500, (1 << 20) + 3, 4096 + 44)
    n = len(lens)
    msgs = [splitmix_bytes(880000 + i, L) for i, L in enumerate(lens)]
    keys = [splitmix_bytes(881000 + i, 32) for i in range(n)]
    nonces = [splitmix_bytes(882000 + i, 12) for i in range(n)]
    ids = [splitmix_bytes(883000 + i, 32) for i in range(n)]
    hashes = [hashlib.sha256(m).digest() for m in msgs]
    ct = [oracle.chacha20_xor(keys[i], nonces[i], msgs[i], oracle.derive_counter(ids[i])) for i in range(n)]
    offs = R.high_base_offsets(lens, 1, BOUNDARY, "straddle", below=(1 << 19) + 1)
    w = SimpleNamespace(n=n, lens=lens, keys=keys, nonces=nonces)
    d_ids = dev(rows_of(ids, 32))
    enet.set_seg_min(-1)
    enet.set_lanes_per_record(0)
    enet.set_host_hash_min(65536)
    try:
        for what, in_parts, out_parts, launch, smalls, flips in (
                ("chunk_store", msgs, ct, lambda b, out, d_out, h: enet.chunk_store(b, out, h, chunk_ids=d_ids),
                 [(rows_of(hashes, 32), 32, ())], ()),
                ("chunk_fetch", ct, msgs, lambda b, out, d_out, ok: enet.chunk_fetch(b, out, d_ids, dev(rows_of(hashes, 32)), ok),
                 [(verdicts(n, ()), 1, ())], ()),
                ("chunk_fetch, tampered", ct, zeroed(msgs, {1}),
                 lambda b, out, d_out, ok: enet.chunk_fetch(b, out, d_ids, dev(rows_of(hashes, 32)), ok),
                 [(verdicts(n, {1}), 1, ())], [(1, (1 << 19) + 77, 0x01)])):
            before = enet.host_hash_batches()
            run_io_unrouted(enet, arenas, w, what, offs, in_parts, out_parts, launch, smalls, flips)
            assert enet.host_hash_batches() == before + 1, f"{what}: the long chunk did not take the host-hash route"
    finally:
        enet.set_host_hash_min(-1)


def run_io_unrouted(enet, A, w, what, offs, in_parts, out_parts, launch, smalls, flips):
    """run_io for a high-base batch without an order whose route the caller asserts itself."""
    named = list(range(w.n))
    A.fill_out()
    place(A.inp, offs, named, [u8(p) for p in in_parts], flips)
    b = enet.Batch(A.inp, dev(offs), dev(rows_of(w.keys, 32)), dev(rows_of(w.nonces, 12)),
                   total_bytes_hint=sum(w.lens), max_len_hint=max(w.lens))
    bufs = [small(w.n, width) for _, width, _ in smalls]
    launch(b, A.out, dev(offs), *[v for _, v in bufs])
    for (big, _), (rows, width, free) in zip(bufs, smalls):
        check_small(big, rows, named, f"{what} sibling array of width {width}", free)
    check_out(A, offs, named, [u8(p) for p in out_parts], what)


# ================================================================== A.6 chunk transfer frames
def test_chunk_frames_across_the_boundary(enet, arenas):
    """A.6: chunk_frame_seal (stored ciphertext -> wire frame, 90 bytes longer) and chunk_frame_open
    (wire frame -> plaintext, and the ciphertext to store into a second region of the output arena,
    32 MiB further up) with both arenas in high base placement, cut on one side and straddle on the
    other, both ways round.  Data lengths 0, 1, 1458 and 65 536; one frame for each status 1 .. 4
    (a flipped body byte, a message re-signed with version 0, another chunk id, another hash):
    status as expected, plaintext, data and ttl zeroed, neighbours intact."""
    import torch
    from chunk_frame_ref import OVERHEAD, chunk_header, chunk_message, stored_data, wire_frame
    lens = (1458, 65536, 1458, 0, 1, 1458, 65536, 1458, 1458)
    n, k = len(lens), 2
    pts = [splitmix_bytes(890000 + i, L) for i, L in enumerate(lens)]
    ids = [(b"\xff\xff\xff\xff" if i % 2 else b"") + splitmix_bytes(891000 + i, 32)[4 if i % 2 else 0:] for i in range(n)]
    ckeys = [splitmix_bytes(892000 + i, 32) for i in range(n)]
    cnonces = [splitmix_bytes(893000 + i, 12) for i in range(n)]
    skeys = [splitmix_bytes(894000 + i, 32) for i in range(n)]
    fnonces = [splitmix_bytes(895000 + i, 12) for i in range(n)]
    ttl = [[3600, 0, 1, 0xFFFFFFFF, 0x01020304][i % 5] for i in range(n)]
    versions = [[1, 4, 2, 3][i % 4] for i in range(n)]
    data = [stored_data(ckeys[i], cnonces[i], ids[i], pts[i]) for i in range(n)]
    hashes = [oracle.sha256(p) for p in pts]
    frames = [wire_frame(skeys[i], fnonces[i], chunk_message(versions[i], ttl[i], ids[i], data[i])) for i in range(n)]
    assert all(len(f) == L + OVERHEAD for f, L in zip(frames, lens))
    A = arenas
    named = list(range(n))
    d_ids, d_ttl = dev(rows_of(ids, 32)), dev(np.array(ttl, dtype=np.uint32).view(np.int32))
    keys, nonces = dev(rows_of(skeys, 32)), dev(rows_of(fnonces, 12))
    flens = tuple(L + OVERHEAD for L in lens)
    # the failures of the open
    bad_frames, bad_ids, bad_hashes = list(frames), list(ids), list(hashes)
    flip = lambda b, at, bit=1: b[:at] + bytes([b[at] ^ bit]) + b[at + 1:]
    bad_frames[1] = flip(frames[1], 16 + 42 + 60000)                                                    # FRAME
    bad_frames[5] = wire_frame(skeys[5], fnonces[5], chunk_header(0, ttl[5], ids[5], lens[5]) + data[5])  # HEADER
    bad_ids[6] = flip(ids[6], 31)                                                                       # CHUNK_ID
    bad_hashes[7] = flip(hashes[7], 9, 0x10)                                                            # HASH
    want_status = np.zeros((n, 1), dtype=np.uint8)
    want_status[[1, 5, 6, 7], 0] = [1, 2, 3, 4]
    failed = {1, 5, 6, 7}
    want_ttl = np.array([0 if i in failed else ttl[i] for i in range(n)], dtype="<u4").view(np.uint8).reshape(n, 4)
    shift = DATA_SHIFT
    for a, b_ in (("cut", "straddle"), ("straddle", "cut")):
        t_data = R.high_base_offsets(lens, k, BOUNDARY, a)
        t_frames = R.high_base_offsets(flens, k, BOUNDARY, b_)
        tag = f"data {a}, frames {b_}"
        # seal
        A.fill_out()
        place(A.inp, t_data, named, [u8(d) for d in data])
        b = enet.Batch(A.inp, dev(t_data), keys, nonces, total_bytes_hint=sum(lens), max_len_hint=max(lens))
        enet.chunk_frame_seal(b, A.out, dev(t_frames), d_ids, d_ttl, versions=dev(np.array(versions, dtype=np.uint8)))
        check_out(A, t_frames, named, [u8(f) for f in frames], f"chunk_frame_seal {tag}")
        # open: the frames where the seal wrote them (in the input arena), plaintext where the data lay
        A.fill_out()
        place(A.inp, t_frames, named, [u8(f) for f in bad_frames])
        b = enet.Batch(A.inp, dev(t_frames), keys, None, total_bytes_hint=sum(flens), max_len_hint=max(flens))
        sbig, status = small(n, 1)
        tbig, ttl_out = small(n, 4)
        enet.chunk_frame_open(b, A.out, dev(t_data), dev(rows_of(bad_ids, 32)), dev(rows_of(ckeys, 32)),
                              dev(rows_of(cnonces, 12)), dev(rows_of(bad_hashes, 32)), status,
                              data_out=A.out[shift:], ttl_out=ttl_out.view(torch.int32))
        check_small(sbig, want_status, named, f"chunk_frame_open {tag} status")
        check_small(tbig, want_ttl, named, f"chunk_frame_open {tag} ttl")
        check_ranges(A, t_data, named, [u8(x) for x in zeroed(data, failed)], f"chunk_frame_open {tag} data_out", shift=shift)
        check_out(A, t_data, named, [u8(x) for x in zeroed(pts, failed)], f"chunk_frame_open {tag} plaintext")
