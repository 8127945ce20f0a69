"""Crafted Poly1305 accumulators through every AEAD kernel.

Every batch here is made of records whose ciphertext was solved (tests/poly1305_ref.py) so that one
accumulator of the record's MAC -- the final H, the radix-2^32 state of one lane at the end of its
run of blocks or in its middle, or one tile's partial -- takes a boundary value: 0..5 and p-1 for
the final subtraction, k 2^128 + d for the carry that ripples out of all four words of
poly32_block, p-1 for the limb multiplication, 2^(26j) and 2^(32j) for the repacking, -s for the
zero tag.  Seeded random data never gets there, so the other GPU tests would pass with a wrong
carry in any of that code.  Expected tags come from the big-integer reference, not from the oracle.

Each case first confirms the kernel it ran on (the routing counters, or the tile-batch counter),
then: seal gives the crafted ciphertext and the reference tag bit for bit; open verifies every
record and returns the plaintext; with one bit of every tag flipped, no record verifies and
nothing but zeros comes out.

Measured once on libraries built with one line of csrc/enet_device.hpp changed: without the last
"+ cy" of poly32_block, or with pfinish never subtracting p, every kernel's case here fails; with
one carry pass in pfinish instead of two, every case whose tag is a sum over several lanes fails
(one lane's accumulator and a tile combine's are already carried: there the second pass changes
nothing).  tests/test_gpu_parity.py -k aead passes in all three.

Lane split (csrc/records_body.hpp "Lane layout"): with P lanes per record lane j owns the ChaCha20
blocks [jB, (j+1)B), B = ceil(blocks / P), lane 0 also the AAD, the lane with the last block also
the length block.  Tiles (csrc/segments.hip): tile t owns blocks [1024 t, 1024 t + 1024), lane j
of its 256 four of them."""
import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
import poly1305_ref as ref
from poly1305_ref import FINAL_TARGETS, STATE_TARGETS
from test_gpu_uniform_matrix import KINDS, expected_route, shape

pytestmark = pytest.mark.gpu

LENS = [0, 1, 15, 16, 17, 63, 64, 65, 100, 1500, 4096]
AADS = [0, 1, 16, 17]
TILE_BLOCKS = 1024
# final-H targets and lane-sum targets in one list: record i of a uniform batch takes entry i mod 44
COMBINED = [("final",) + t + (None,) for t in FINAL_TARGETS] + [("run",) + t for t in STATE_TARGETS]
ATTEMPTS = {}  # scope kind -> most nonces tried by a crafted record (printed with the wall time)


@pytest.fixture(scope="module")
def enet():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ephemeralnet_amd as E
    E.lib()
    t0 = time.time()
    yield E
    E.set_lanes_per_record(0)
    E.set_staging(-1)
    E.set_seg_min(-1)
    E.set_duplex_split(-1)
    print(f"\n[poly1305 edges] module wall time {time.time() - t0:.1f} s; most nonces tried {ATTEMPTS}")


# ------------------------------------------------------------------------------- geometry
def lane_runs(L, alen, P):
    """{lane: (first, last) MAC-stream block of its run} for the lanes that have one."""
    na, nct, N = ref.counts(L, alen)
    nb = (L + 63) // 64
    B = -(-nb // P)
    jlast = (nb - 1) // B if nb else 0
    runs = {}
    for j in range(P):
        c0 = min(j * B, nb)
        c1 = min(c0 + B, nb)
        a = 0 if j == 0 else na + 4 * c0
        b = N - 1 if j == jlast else na + min(4 * c1, nct) - 1
        if b >= a and (j == 0 or c1 > c0):
            runs[j] = (a, b)
    return runs


def tile_count(L):
    return max(1, -(-((L + 63) // 64) // TILE_BLOCKS))


def tile_run(L, alen, t, j=None):
    """Blocks of tile t (j None) or of its lane j."""
    na, nct, N = ref.counts(L, alen)
    nb = (L + 63) // 64
    tb0 = t * TILE_BLOCKS
    tb1 = min(tb0 + TILE_BLOCKS, nb)
    c0, c1 = (tb0, tb1) if j is None else (min(tb0 + 4 * j, tb1), min(min(tb0 + 4 * j, tb1) + 4, tb1))
    first = t == 0 and (j is None or j == 0)
    a = 0 if first else na + 4 * c0
    b = N - 1 if (c1 == nb and (c1 > c0 or nb == 0)) else na + min(4 * c1, nct) - 1
    return a, b


def pick(seq, pos):
    """First, middle or last (pos 0, 1, 2) of a sequence."""
    return seq[(len(seq) - 1) * pos // 2]


def record_key(seed):
    return ref.seeded_bytes(1_000_000 + seed, 32)


def note(rec, kind):
    ATTEMPTS[kind] = max(ATTEMPTS.get(kind, 0), rec.attempts)
    return rec


def final_record(seed, L, alen, ti, pos):
    name, t = FINAL_TARGETS[ti % len(FINAL_TARGETS)]
    f = pick(ref.full_blocks(L, alen), pos)
    return note(ref.craft(record_key(seed), ref.nonce_seq(seed), L, alen, f, t, ("final",), fill=seed), "final")


def state_record(seed, L, alen, run, target, pos, kind="range"):
    """The blocks run = (a, b) summed from zero land on the state target at the run's end -- or,
    for a target with a next block, at a block inside the run that a full block follows."""
    a, b = run
    name, t, then = target
    full = [i for i in ref.full_blocks(L, alen) if a <= i <= b]
    e = b
    if then is not None:
        e = pick([i for i in range(a + 1, b) if i + 1 in full], pos)
        full = [i for i in full if i <= e]
    assert e > a, "the scope needs a second block"
    return note(ref.craft(record_key(seed), ref.nonce_seq(seed), L, alen, pick(full, pos), t, ("range", a, e),
                          fill=seed, then=then), kind)


def special_records(seed, L, alen):
    """Not crafted: ciphertext and AAD all 0xFF and all 0x00, and the same again and seeded bytes
    under a heavy r (every column sum of the multiplications near its largest)."""
    key = record_key(seed)
    plain_nonce = next(ref.nonce_seq(seed))
    heavy, _ = ref.heavy_nonce(key, ref.nonce_seq(seed + 1))
    out = [ref.plain(key, n, byte * alen, byte * L) for n in (plain_nonce, heavy) for byte in (b"\xff", b"\x00")]
    return out + [ref.plain(key, heavy, ref.seeded_bytes(seed, alen), ref.seeded_bytes(seed + 1, L))]


def pack(recs, hmac=False):
    """Everything the device run needs, computed once per case."""
    d = SimpleNamespace(n=len(recs), keys=[r.key for r in recs], nonces=[r.nonce for r in recs],
                        aads=[r.aad for r in recs], cts=[r.ct for r in recs], pts=[r.pt for r in recs],
                        tags=b"".join(r.tag for r in recs))
    d.macs = b"".join(oracle.hmac_sha256(r.key, p) for r, p in zip(recs, d.pts)) if hmac else None
    return d


# ------------------------------------------------------------------------------- the device run
def first_bad(got, want):
    return next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), None)


def run_records(enet, d, want, label, hmac=False):
    """want: "tiles" (one more sequence-parallel batch per call), the routing counters' delta, or
    None (the AEAD + HMAC paths have no counter: the split setting alone picks their kernel)."""
    import torch
    n = d.n

    def routed(fn):
        r0, s0 = enet.record_route_counts(), enet.seg_batches()
        fn()
        torch.cuda.synchronize()
        r1, s1 = enet.record_route_counts(), enet.seg_batches()
        if want == "tiles":
            assert s1 == s0 + 1, (label, "the batch did not take the tiles")
        elif want is not None:
            assert {k: r1[k] - r0[k] for k in KINDS} == want and s1 == s0, (label, r0, r1, want, s1 - s0)

    dev = lambda b: torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).cuda()
    b_pt = enet.make_batch(d.pts, d.keys, d.nonces)
    b_ct = enet.make_batch(d.cts, d.keys, d.nonces)
    offs = b_pt.offsets.cpu().tolist()
    cut = lambda t: [t.cpu().numpy().tobytes()[offs[i]:offs[i + 1]] for i in range(n)]
    aad = aoff = None
    if not hmac:
        aad = dev(b"".join(d.aads))
        aoff = torch.tensor(np.concatenate([[0], np.cumsum([len(a) for a in d.aads])]), dtype=torch.int64).cuda()
    ref_tags, ref_macs = dev(d.tags), dev(d.macs) if hmac else None

    # ---- seal: the crafted ciphertext comes back, the tag is the reference's
    out = torch.full_like(b_pt.arena, 0xA5)
    tags = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    macs = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    if hmac:
        routed(lambda: enet.aead_hmac_seal(b_pt, out, tags, macs))
        assert macs.cpu().numpy().tobytes() == d.macs, (label, "seal HMAC")
    else:
        routed(lambda: enet.aead_seal(b_pt, out, tags, aad, aoff))
    got = cut(out)
    assert got == d.cts, (label, "seal ciphertext, record", first_bad(got, d.cts))
    th = tags.cpu().numpy().tobytes()
    if th != d.tags:
        bad = [i for i in range(n) if th[16 * i:16 * i + 16] != d.tags[16 * i:16 * i + 16]]
        raise AssertionError((label, "seal tag, records", bad[:16], len(bad), "of", n,
                              th[16 * bad[0]:16 * bad[0] + 16].hex(), d.tags[16 * bad[0]:16 * bad[0] + 16].hex()))

    # ---- open: every record verifies
    def open_with(tag_t):
        back = torch.full_like(b_ct.arena, 0xA5)
        ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        if hmac:
            routed(lambda: enet.aead_hmac_open(b_ct, back, tag_t, ref_macs, ok))
        else:
            routed(lambda: enet.aead_open(b_ct, back, tag_t, ok, aad, aoff))
        return cut(back), ok.cpu().tolist()

    got, ok = open_with(ref_tags)
    assert ok == [1] * n, (label, "open verdicts, records", [i for i in range(n) if ok[i] != 1][:16])
    assert got == d.pts, (label, "open plaintext, record", first_bad(got, d.pts))

    # ---- one flipped bit in every tag: nothing verifies, nothing is released
    flipped = np.frombuffer(d.tags, dtype=np.uint8).copy()
    for i in range(n):
        bit = (37 * i) % 128
        flipped[16 * i + bit // 8] ^= 1 << (bit % 8)
    got, ok = open_with(torch.from_numpy(flipped).cuda())
    assert ok == [0] * n, (label, "flipped tags verified, records", [i for i in range(n) if ok[i] != 0][:16])
    zeros = [bytes(len(p)) for p in d.pts]
    assert got == zeros, (label, "flipped tag released plaintext, record", first_bad(got, zeros))


def delta(kind, staged, rest):
    w = dict.fromkeys(KINDS, 0)
    w[kind] += staged
    w["PerLane"] += rest
    return w


# ------------------------------------------------------------------------------- per-lane kernel
@functools.lru_cache(maxsize=None)
def per_lane_case(P):
    """About 200 ragged records cycling through the final-H set (every length and AAD length; a
    shape with no full block gets 16 bytes of AAD); for every lane of a record of 3 blocks per lane
    (the last one partial) every lane-sum target, the free block first, in the middle and last of the
    lane's run; and the records that are not crafted, at two lengths."""
    recs = []
    seed = 10_000 * P
    for i in range(200):
        L, alen = LENS[i % len(LENS)], AADS[i % len(AADS)]
        if not ref.full_blocks(L, alen):
            alen = 16
        recs.append(final_record(seed + i, L, alen, i, i % 3))
    L = 64 * 3 * P - 27
    for j in range(P):
        for ti, target in enumerate(STATE_TARGETS):
            alen = AADS[(j + ti) % len(AADS)]
            run = lane_runs(L, alen, P)[j]
            recs.append(state_record(seed + 1000 + 16 * j + ti, L, alen, run, target, ti % 3))
    recs += special_records(seed + 5000, 1500, 17) + special_records(seed + 5010, 64 * P, 0)
    return pack(recs)


@pytest.mark.parametrize("P", [1, 2, 4, 8, 16])
def test_per_lane_kernel(enet, P):
    d = per_lane_case(P)
    enet.set_seg_min(-1)
    enet.set_lanes_per_record(P)
    enet.set_staging(0)
    run_records(enet, d, delta("PerLane", 0, d.n), ("per lane", P))


# ------------------------------------------------------------------------------- uniform kernels
def uniform_records(P, L, n, seed, specials=False):
    """n records of L bytes: record i takes entry i mod 44 of the combined target list, a lane-sum
    target on lane i mod P, the free block at position i mod 3, AAD length i mod 4 of the list."""
    recs = []
    if specials:
        recs = special_records(seed + 90_000, L, 17)
    for i in range(len(recs), n):
        kind, name, t, then = COMBINED[i % len(COMBINED)]
        alen = AADS[i % len(AADS)]
        if kind == "final":
            recs.append(final_record(seed + i, L, alen, i % len(COMBINED), i % 3))
        else:
            run = lane_runs(L, alen, P)[i % P]
            recs.append(state_record(seed + i, L, alen, run, (name, t, then), i % 3))
    return recs


UNIFORM_B = {1: 5, 4: 4, 5: 6}  # staging -> blocks per lane (staging 1 with an odd B: lockstep)


@functools.lru_cache(maxsize=None)
def uniform_case(P, B):
    L, n, full = shape(P, B, 0)
    return pack(uniform_records(P, L, n, 20_000 * P + 100 * B))


@pytest.mark.parametrize("P", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("staging", [1, 4, 5])
def test_uniform_kernels(enet, staging, P):
    """The uniform matrix's shapes, L = 64 P B and n = full (512 / P) + 3: one launch holds the whole
    target set on every lane position of a workgroup, the three trailing records run per lane."""
    B = UNIFORM_B[staging]
    d = uniform_case(P, B)
    want = expected_route(staging, P, B, 0, d.n)
    assert want[0] == {1: "Lockstep", 4: "RunStaged", 5: "Lockstep"}[staging] and want[2] == 3
    enet.set_seg_min(-1)
    enet.set_lanes_per_record(P)
    enet.set_staging(staging)
    run_records(enet, d, delta(*want), ("uniform", staging, P, B))


@functools.lru_cache(maxsize=None)
def line_staged_case():
    return pack(uniform_records(1, 1500, 259, 777_000))


def test_line_staged_kernel(enet):
    """One lane, L = 1500: 256 records line-staged and 3 per lane."""
    d = line_staged_case()
    enet.set_seg_min(-1)
    enet.set_lanes_per_record(1)
    enet.set_staging(1)
    run_records(enet, d, delta("LineStaged", 256, 3), "line staged")


# ------------------------------------------------------------------------------- stream kernel
@functools.lru_cache(maxsize=None)
def stream_case(P, L, n):
    return pack(uniform_records(P, L, n, 30_000 * P + n, specials=True))


@pytest.mark.parametrize("P,L,n", [(2, 4096, 256), (2, 4096, 259), (4, 8192, 128)])
def test_stream_kernel(enet, P, L, n):
    """One workgroup of the streaming kernel (and 3 records per lane): the leader lane (0) makes r,
    its powers' base and the tag for the record's other lanes, so lane-sum targets sit on the
    leader and on every other lane; the extreme-data and heavy-r records ride along."""
    d = stream_case(P, L, n)
    per = 512 // P
    enet.set_seg_min(-1)
    enet.set_lanes_per_record(P)
    enet.set_staging(1)
    run_records(enet, d, delta("Stream", n // per * per, n % per), ("stream", P, L, n))


# ------------------------------------------------------------------------------- tiles
LONG = [65536, 65537, (2 << 16) + 17, 3 * 65536 - 1, (256 << 10) + 100]
TILE_LANES = [0, 1, 63, 64, 255]
TILE_STATES = [t for t in STATE_TARGETS if t[2] is None]


def tile_records(L, alen, seed, k):
    """Three records of one long length: the final H; one tile's partial at the tile's end; one
    lane's run inside a tile -- the ragged last tile where that has a run worth crafting
    (a full block and two more), else a whole one."""
    nt = tile_count(L)
    recs = [final_record(seed, L, alen, 7 * k, k % 3)]
    t = (nt - 1, 0, nt // 2)[k % 3]
    recs.append(state_record(seed + 1, L, alen, tile_run(L, alen, t), TILE_STATES[k % len(TILE_STATES)], k % 3,
                             kind="tile"))
    a, b = tile_run(L, alen, nt - 1, 0)
    ragged_ok = L % 65536 != 0 and b - a >= 2 and any(a <= i <= b for i in ref.full_blocks(L, alen))
    run = (a, b) if ragged_ok else tile_run(L, alen, k % (L // 65536), TILE_LANES[k % len(TILE_LANES)])
    recs.append(state_record(seed + 2, L, alen, run, STATE_TARGETS[(k + 3) % len(STATE_TARGETS)], k % 3,
                             kind="tile lane"))
    return recs


@functools.lru_cache(maxsize=None)
def tiles_mixed_case():
    recs = []
    shorts = [(0, 16), (17, 0), (100, 1), (1500, 17), (4096, 16)]
    for k, L in enumerate(LONG):
        Ls, alen = shorts[k]
        recs.append(final_record(400_000 + k, Ls, alen, 11 * k + 3, k % 3))
        recs += tile_records(L, AADS[k % len(AADS)], 410_000 + 10 * k, k)
    # one lane run inside a whole tile of the longest record (its ragged last tile took the others)
    L = LONG[-1]
    recs.append(state_record(420_000, L, 17, tile_run(L, 17, 2, 63), STATE_TARGETS[-1], 1, kind="tile lane"))
    return pack(recs)


def test_tiles_mixed_batch(enet):
    """Plan, tiles and combine: short crafted records around long ones of 1 to 5 tiles."""
    d = tiles_mixed_case()
    enet.set_lanes_per_record(0)
    enet.set_staging(-1)
    enet.set_seg_min(0)
    try:
        run_records(enet, d, "tiles", "tiles, mixed")
    finally:
        enet.set_seg_min(-1)


@functools.lru_cache(maxsize=None)
def tiles_uniform_case(k):
    """Four records of 256 KiB (four whole tiles, the last one with the length block): a final H
    of k (the subtraction of p), another final target, the partial of tile k, and in the next tile
    a lane's run on k 2^128 + d (the rippling carry)."""
    L, seed = 256 << 10, 430_000 + 10 * k
    alen = AADS[k % len(AADS)]
    recs = [final_record(seed, L, alen, k, k % 3),
            final_record(seed + 1, L, AADS[(k + 1) % len(AADS)], 9 * k + 6, (k + 1) % 3),
            state_record(seed + 2, L, alen, tile_run(L, alen, k), TILE_STATES[2 * k % len(TILE_STATES)], k % 3,
                         kind="tile"),
            state_record(seed + 3, L, alen, tile_run(L, alen, (k + 1) % 4, TILE_LANES[k]), STATE_TARGETS[k],
                         (k + 2) % 3, kind="tile lane")]
    return pack(recs)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_tiles_uniform_long_batch(enet, k):
    """Four records of 256 KiB, which the hints call uniform and long: the one-launch AEAD kernel."""
    d = tiles_uniform_case(k)
    assert d.n == 4 and all(len(c) == 256 << 10 for c in d.cts)
    enet.set_lanes_per_record(0)
    enet.set_staging(-1)
    enet.set_seg_min(0)
    try:
        run_records(enet, d, "tiles", ("tiles, uniform", k))
    finally:
        enet.set_seg_min(-1)


# ------------------------------------------------------------------------------- AEAD + HMAC
@functools.lru_cache(maxsize=None)
def duplex_case():
    """64 lengths from 512 B to 64 KiB (log-uniform, the ends included), no AAD: three records in
    four walk the final-H set, the fourth takes a prefix target early, halfway, at the last
    ciphertext block or at the length block."""
    rng = np.random.default_rng(1305)
    lens = np.exp(rng.uniform(np.log(512), np.log(65536), 64)).astype(int).tolist()
    lens[:4] = [512, 65536, 1000, 16384 + 37]
    recs = []
    for i, L in enumerate(lens):
        q = i // 4
        if i % 4 != 3:
            recs.append(final_record(500_000 + i, L, 0, 3 * q + i % 4, i % 3))
        else:
            na, nct, N = ref.counts(L, 0)
            e = (2, nct // 2, nct - 1, N - 1)[q % 4]
            recs.append(state_record(500_000 + i, L, 0, (0, e), STATE_TARGETS[q % len(STATE_TARGETS)], q % 3,
                                     kind="prefix"))
    assert 3 * (len(lens) // 4) >= len(FINAL_TARGETS) and len(lens) // 4 >= len(STATE_TARGETS)
    return pack(recs, hmac=True)


@pytest.mark.parametrize("split", [-1, 1], ids=["split-auto", "split-on"])
@pytest.mark.parametrize("lanes", [0, 1, 4])
def test_aead_hmac_kernels(enet, lanes, split):
    """duplex.hip, and duplex_split.hip forced on: one Poly1305 accumulator per record, so the
    targets are the final H and Horner prefixes.  The HMAC is the oracle's as in the other tests."""
    d = duplex_case()
    enet.set_seg_min(-1)
    enet.set_staging(-1)
    enet.set_lanes_per_record(lanes)
    enet.set_duplex_split(split)
    try:
        run_records(enet, d, None, ("aead + hmac", lanes, split), hmac=True)
    finally:
        enet.set_duplex_split(-1)
