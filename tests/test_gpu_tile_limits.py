"""The long-record tile paths (csrc/segments.hip, csrc/long_records.cpp) past their launch caps, past
their scratch floors, at the edges of the one-launch combine's geometry, and on two streams at once.

The other GPU modules stay inside one trip of each capped loop and inside the scratch floors.  Here:
  1. plan + tiles over 4 300 records that are one tile or more each (4 328 tiles on
     kSegTileBlocksMax = 4 096 workgroups: 232 tiles, ragged ones, in a second trip of seg_kernel's
     loop), the plan scratch grown to 3.8 MB;
  2. one record of 4 113 tiles beside one of 5: whole tiles in the second trip, a counter that wraps
     there, and a last-arriver combine (17 tiles per lane) over partials written in both trips;
  3. 262 444 positions on kSegPlanBlocksMax = 1 024 plan workgroups of 256: a second trip of
     seg_plan_kernel, over claim bytes an earlier call on the stream left non-zero;
  4. the one-launch AEAD kernel at 1, 2, 16 and 17 tiles per record (arrival groups of one member,
     group 0 alone with two) and at 257, 258, 513, 514 and 2 050 tiles (lq = 0, 1, 1, 2, 4: the
     combine's tiles per lane, 2^lq), the partials grown past their 64 KiB floor;
  5. two threads, each with a stream, data and buffers of its own, 20 rounds of those paths while
     the other thread's scratch grows.
Every expected byte is the CPU oracle's (oracle.aead_seal, oracle.chacha20_xor); outputs, tags and
verdicts are prefilled with 0x5A between guards (run_ops of test_gpu_record_order.py).  Each test
first asserts, by arithmetic from its lengths (seg_layout / seg_grid below restate
csrc/long_route.hpp; tests/cpp/route_table.cpp rows 108 .. 111 and 205 .. 207 pin the same figures
against the header), that its shape is past the cap it is about.

Measured once on library copies with one line of a kernel changed (arithmetic or skipped work, no
address touched), each against this module and tests/test_gpu_segments.py, the last against
tests/test_gpu_shamir.py:
  a. seg_kernel leaves its tile loop after one trip: tests 1 and 2 (all three) and test 5 fail,
     test_gpu_segments.py passes;
  b. seg_plan_kernel leaves its loop after one trip: both cases of test 3 fail (records at
     positions from 262 144 on left as prefilled), test_gpu_segments.py passes;
  c. the power wave reads pw_s[12 + b] for pw_s[12 + lq + b]: the lq cases 258, 513, 514 and 2 050,
     the lying-hint case and test 5 (its 33 MiB record) fail, 257 passes (lq = 0) -- and
     test_gpu_segments.py's 1 x 32 MiB case (512 tiles, lq = 1) fails too: that module was not
     blind to this line, only to lq >= 2;
  d. the arrival groups with ng = 16 for every T (const uint32_t ng = kUGroups): no record of fewer
     than 16 tiles is ever finished, and its top counter is left non-zero, so every arrival-group
     case, the 2 050-tile case (its 5-tile batches) and test 5 fail; test_gpu_segments.py's
     5 x 300 KiB cases fail too.  Changing only the divisor of `members` to 16 is no mutation: for
     T < 16 both ceil((T - g) / T) and ceil((T - g) / 16) are 1, for T >= 16 ng is 16 already;
  e. the Shamir kernels leave their loops after one trip: test_split_and_combine_past_the_block_cap
     fails at record 2 097 152, the other kernel tests of test_gpu_shamir.py pass.
"""
import threading
import time

import numpy as np
import pytest

from test_gpu_record_order import FILL, Guarded, batch_data, run_ops, same
from test_gpu_segments import H53, make, shapes

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
TILE = 64 * KiB                 # kSegTileBytes
SEG_MIN = 256 * KiB             # kSegMin, the automatic threshold
ENTRY = 864                     # sizeof(SegEntry)
PLAN_THREADS, PLAN_BLOCKS_MAX, TILE_BLOCKS_MAX = 256, 1024, 4096  # kSegPlanThreads, kSeg*BlocksMax
PLAN_FLOOR, PARTIALS_FLOOR = 256 * KiB, 64 * KiB                   # long_records.cpp grow() floors
U_THREADS = 256                 # kSegThreads: lanes of the one-launch combine


def seg_layout(count, max_len_hint, total_bytes_hint, long_min):
    """csrc/long_route.hpp seg_layout, restated."""
    total = total_bytes_hint or min(count, 1024) * max_len_hint
    ecap = min(total // long_min + 1 if long_min else count, count)
    tcap = min(total // TILE + ecap + 1, 0xFFFFFFFF)
    o_cl = 256 + ecap * ENTRY
    o_part = (o_cl + count + 255) & ~255
    return dict(ecap=ecap, tcap=tcap, o_cl=o_cl, o_part=o_part, bytes=o_part + tcap * 32)


def seg_grid(count, lay):
    """csrc/long_route.hpp seg_grid: (plan workgroups, tile workgroups)."""
    return min(-(-count // PLAN_THREADS), PLAN_BLOCKS_MAX), min(lay["tcap"], TILE_BLOCKS_MAX)


def tiles_of(L):
    return max(1, -(-L // TILE))  # an empty record claims one tile (seg_plan_kernel)


def lq_of(T):
    """The one-launch combine's log2(tiles per lane) for a record of T tiles (segments.hip)."""
    lq = 0
    while (U_THREADS << lq) < T - 1:
        lq += 1
    return lq


@pytest.fixture(scope="module")
def enet():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ephemeralnet_amd as E
    E.lib()
    yield E
    E.set_seg_min(-1)
    E.set_lanes_per_record(0)
    E.set_staging(-1)
    PAIR.clear()


@pytest.fixture(autouse=True)
def settings_and_wall_time(enet, request):
    enet.set_lanes_per_record(0)
    enet.set_staging(-1)
    t0 = time.time()
    try:
        yield
    finally:
        enet.set_seg_min(-1)
        print(f"\n[tile limits] {request.node.name}: {time.time() - t0:.1f} s")


def own_stream():
    """A stream for one test: its tile scratch starts at the floors unless an earlier test drew the
    same stream from torch's pool (nothing here depends on that)."""
    import torch
    torch.cuda.synchronize()
    return torch.cuda.Stream()


# ------------------------------------------------------------------ 1. tile loop, ragged later trips
N1 = 4300
CYCLE1 = (0, 1, 15, 16, 17, 63, 64, 65, 100, 1500, 4095)
BIG1 = {300: 65536, 900: 65537, 1500: 3 * 65536 - 1, 2100: (256 << 10) + 100, 2700: 300 << 10,
        3300: (2 << 16) + 17, 4299: 1 << 20}
LENS1 = tuple(BIG1.get(i, CYCLE1[i % len(CYCLE1)]) for i in range(N1))


def data1():
    return batch_data(LENS1, 760000, 3, "wrap977")


def test_tile_loop_second_trip_ragged_tiles(enet):
    """4 300 records under set_seg_min(0): every one is claimed, an empty one included, so the batch
    is 4 328 tiles on 4 096 tile workgroups (which 232 run in the second trip is the plan's CAS
    order's choice).  ChaCha20 with counters that wrap inside the long records, seal with AAD (0, 1,
    16, 17 bytes), open, and an open with a flipped tag bit on a 1 500-byte record, a flipped
    ciphertext byte in the 1 MiB record and a flipped AAD byte on a third: those three come back
    zeroed with ok = 0, every other record, the guards and the gap stay as they must.  Every call
    is one more seg_batches().  Then seal again on the stream: the plan scratch (3 859 680 bytes,
    past the 256 KiB floor: route_table.cpp row 108) is reused as the first calls left it."""
    import torch
    lay = seg_layout(N1, max(LENS1), sum(LENS1), 0)
    assert sum(tiles_of(L) for L in LENS1) == 4328 > TILE_BLOCKS_MAX      # kSegTileBlocksMax
    assert seg_grid(N1, lay) == (17, TILE_BLOCKS_MAX) and lay["tcap"] == 4367
    assert lay["bytes"] == 3859680 > PLAN_FLOOR
    d = data1()
    tv, cv, av = 1505, 4299, 1489  # 1 500 bytes; 1 MiB; 17 bytes with a 1-byte AAD
    assert LENS1[tv] == 1500 and LENS1[cv] == 1 << 20 and LENS1[av] == 17 and d.aoff[av + 1] - d.aoff[av] == 1
    for i in (2100, 2700, 4299):  # the u32 counter wraps inside these
        assert 0 < (1 << 32) - int(d.ctr[i]) < (LENS1[i] + 63) // 64
    enet.set_seg_min(0)
    with torch.cuda.stream(own_stream()):
        kw = dict(tag_victim=tv, ct_victim=(cv, 15 * TILE + 5), want_route={"PerLane": N1}, want_seg=1)
        run_ops(enet, d, None, aad_victim=av, tag="4300 records", **kw)
        run_ops(enet, d, None, ops=("seal",), tag="4300 records, seal again", **kw)


# ------------------------------------------------------------------ 2. whole tiles in the second trip
LENS2 = ((257 << 20) + 17, 300 << 10)
WRAP2 = 4100 * 1024 + 7  # the block of the big record whose counter is 0: in tile 4 100


PAIR = {}  # make()'s batch of the two records, shared by the two tests, dropped at teardown


def premise2():
    """4 118 tiles on 4 096 workgroups, one record of 4 113: wherever the plan puts it, its tiles
    from 4 096 - 5 on at the latest run in the second trip (kSegTileBlocksMax)."""
    lay = seg_layout(2, max(LENS2), sum(LENS2), SEG_MIN)
    assert [tiles_of(L) for L in LENS2] == [4113, 5]
    assert seg_grid(2, lay) == (1, TILE_BLOCKS_MAX) and lay["tcap"] == 4119
    assert -(-(4113 - 1) // U_THREADS) == 17  # the plan + tiles combine's tiles per lane
    # route_table.cpp row 109: this layout stays inside the plan scratch's floor (test 1 passes it)
    assert lay["bytes"] == 133856 < PLAN_FLOOR


def device_pair(enet):
    if not PAIR:
        PAIR["made"] = make(enet, list(LENS2), 770000)
    b = PAIR["made"][0]
    assert b.total_bytes_hint == sum(LENS2) and b.max_len_hint == max(LENS2)
    return PAIR["made"]


def test_tile_loop_second_trip_whole_tiles_chacha20(enet):
    """ChaCha20 over [257 MiB + 17, 300 KiB] (truthful hints, automatic threshold: planned).  The big
    record's counter wraps at its block 4 100 * 1 024 + 7, in a tile only a second trip reaches."""
    import torch
    import oracle
    premise2()
    assert 4096 * 1024 < WRAP2 < (LENS2[0] + 63) // 64
    b, items, keys, nonces = device_pair(enet)
    ctr = np.array([(1 << 32) - WRAP2, 0xFFFFFFFE], dtype=np.uint32)
    out = torch.full_like(b.arena, FILL)
    before = enet.seg_batches()
    enet.chacha20_xor(b, out, counters=torch.tensor(ctr.view(np.int32)).cuda())
    torch.cuda.synchronize()
    assert enet.seg_batches() == before + 1
    oh = out.cpu().numpy()
    offs = b.offsets.cpu().tolist()
    for i in range(2):
        want = np.frombuffer(oracle.chacha20_xor(keys[i], nonces[i], items[i], int(ctr[i])), dtype=np.uint8)
        same(oh[offs[i]:offs[i + 1]], want, np.array([0, LENS2[i]]), f"chacha20 record {i}")


def test_tile_loop_second_trip_whole_tiles_aead(enet):
    """Seal, open and a tampered open of the same two records: the big record's tag is combined by
    its last tile to arrive from partials written in both trips.  The tampered open flips one
    ciphertext byte past 4 096 * 65 536 of the big record (a second-trip tile) and one tag bit of
    the small one: both zeroed, ok = 0.  Then the 4 300 records of test 1 are sealed on the same
    stream, in the scratch this call left."""
    import torch
    import oracle
    premise2()
    b, items, keys, nonces = device_pair(enet)
    offs = b.offsets.cpu().tolist()
    ct = torch.full_like(b.arena, FILL)
    tags = torch.full((32,), FILL, dtype=torch.uint8, device="cuda")
    before = enet.seg_batches()
    enet.aead_seal(b, ct, tags)
    torch.cuda.synchronize()
    assert enet.seg_batches() == before + 1
    cth, th = ct.cpu().numpy(), tags.cpu().numpy().tobytes()
    for i in range(2):
        c, t = oracle.aead_seal(keys[i], nonces[i], items[i])
        same(cth[offs[i]:offs[i + 1]], np.frombuffer(c, dtype=np.uint8), np.array([0, LENS2[i]]), f"ciphertext {i}")
        assert th[16 * i:16 * i + 16] == t, f"tag {i}"
    del cth
    hint = dict(total_bytes_hint=b.total_bytes_hint, max_len_hint=b.max_len_hint)
    back = torch.full_like(ct, FILL)
    ok = torch.full((2,), FILL, dtype=torch.uint8, device="cuda")
    enet.aead_open(enet.Batch(ct, b.offsets, b.keys, b.nonces, **hint), back, tags, ok)
    assert ok.cpu().tolist() == [1, 1] and torch.equal(back, b.arena)
    flip = 4100 * TILE + 5
    assert 4096 * TILE < flip < LENS2[0]
    ct[offs[0] + flip] ^= 0x10
    tags[16 + 9] ^= 0x02
    back.fill_(FILL)
    ok.fill_(FILL)
    enet.aead_open(enet.Batch(ct, b.offsets, b.keys, b.nonces, **hint), back, tags, ok)
    assert enet.seg_batches() == before + 3
    assert ok.cpu().tolist() == [0, 0] and int(back.count_nonzero()) == 0, "a tampered record released plaintext"
    del ct, back
    enet.set_seg_min(0)
    run_ops(enet, data1(), None, tag_victim=None, ct_victim=None, ops=("seal",), want_seg=1, tag="4300 records after 257 MiB")


# ------------------------------------------------------------------ 3. plan kernel, second trip
N3 = PLAN_THREADS * PLAN_BLOCKS_MAX + 300
LONG3 = ((256 << 10) + 100, 65536 + 1, 300 << 10)
AT3 = {"late": (262150, 262300, N3 - 1), "early": (5, 300, 70000)}
HINTS3 = dict(total_bytes_hint=1159863, max_len_hint=300 << 10)


def lens3(which):
    lens = [1 + i % 3 for i in range(N3)]
    for p, L in zip(AT3[which], LONG3):
        lens[p] = L
    return tuple(lens)


def refs3():
    """The records test 3 checks against the oracle: every 61st, the first and last 300 (the
    positions from 262 144 on, in batch order and reversed) and wherever a long record may sit."""
    keep = set(range(0, N3, 61)) | set(range(300)) | set(range(N3 - 300, N3))
    keep |= set(AT3["late"]) | set(AT3["early"]) | {N3 - 1 - p for p in AT3["late"] + AT3["early"]}
    return tuple(sorted(keep))


def run_sparse(enet, d, reverse, mode, tag):
    """One ChaCha20 or seal call over all of d (in batch order, or reversed by an `order`) into
    prefilled outputs; the records of d.refs bit-exact against the oracle.  Seal: no record's tag
    is left as prefilled, whether in d.refs or not."""
    import torch
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    tord = torch.arange(d.n - 1, -1, -1, dtype=torch.int32, device="cuda") if reverse else None
    b = enet.Batch(dev(d.pt), dev(d.offs), dev(d.keys), dev(d.nonces), key_stride=d.key_stride, order=tord,
                   count=d.n if reverse else None, **HINTS3)
    picked = np.zeros(d.n, dtype=bool)
    picked[list(d.refs)] = True
    in_refs = np.repeat(picked, np.array(d.lens))
    before = enet.seg_batches()
    out = Guarded(d.size)
    if mode == "xor":
        enet.chacha20_xor(b, out.view, dev(d.ctr.view(np.int32)))
        want = d.xo
    else:
        tags = Guarded(16 * d.n)
        enet.aead_seal(b, out.view, tags.view, dev(d.aad), dev(d.aoff))
        want = d.ct
    assert enet.seg_batches() == before + 1, tag
    got = out.host()
    same(np.where(in_refs, got, 0), want, d.offs, f"{tag} {mode}")  # want is zero outside d.refs
    if mode == "seal":
        th = tags.host()
        same(np.where(np.repeat(picked, 16), th, 0), d.tags, 16 * np.arange(d.n + 1), f"{tag} tags")
        unwritten = np.flatnonzero((th.reshape(d.n, 16) == FILL).all(axis=1))
        assert unwritten.size == 0, f"{tag}: records never sealed (first {unwritten[:5].tolist()} of {unwritten.size})"


@pytest.mark.parametrize("reverse", [False, True], ids=["batch_order", "reversed"])
def test_plan_kernel_second_trip_and_stale_claim_bytes(enet, reverse):
    """n = 262 444 records of 1 .. 3 bytes under one shared key, threshold 64 KiB, but three records
    of 256 KiB + 100, 64 KiB + 1 and 300 KiB: 1 024 plan workgroups of 256 threads reach positions
    from 262 144 on only in a second trip (kSegPlanBlocksMax).  Two batches with the same hints
    (route_table.cpp row 110: claim bytes at [15 808, 278 252) of a 279 424-byte scratch, past the
    256 KiB floor): "late" has the long records at positions 262 150, 262 300 and n - 1, "early" at
    5, 300 and 70 000.  In batch order late runs first, so early's second trip must clear claim
    bytes that were 1; reversed (order[k] = n - 1 - k) early runs first, for the same reason.
    Before them the first 320 records of test 1's batch are sealed on the stream under threshold 0:
    that call's partials (row 111: from byte 277 248, 32 per tile, 320 tiles and more) lie on the
    claim bytes of positions 262 144 .. 262 443, so a plan kernel that skipped its second trip would
    hand the record engine skip flags made of Poly1305 limbs.  ChaCha20 and seal; checked: every
    record at a position from 262 144 on, every long record, and every 61st of the rest; and no
    record's tag is left unwritten."""
    import torch
    lay = seg_layout(N3, HINTS3["max_len_hint"], HINTS3["total_bytes_hint"], TILE)
    assert N3 > PLAN_THREADS * PLAN_BLOCKS_MAX and seg_grid(N3, lay) == (PLAN_BLOCKS_MAX, 36)
    assert (lay["o_cl"], lay["o_part"], lay["bytes"]) == (15808, 278272, 279424) and lay["bytes"] > PLAN_FLOOR
    assert HINTS3["total_bytes_hint"] == max(sum(lens3("late")), sum(lens3("early")))
    first = seg_layout(320, max(LENS1[:320]), sum(LENS1[:320]), 0)
    second_trip = (lay["o_cl"] + PLAN_THREADS * PLAN_BLOCKS_MAX, lay["o_cl"] + N3)
    assert first["o_part"] <= second_trip[0] and first["o_part"] + 32 * 320 >= second_trip[1]
    refs = refs3()
    sequence = ("early", "late") if reverse else ("late", "early")
    # the first call claims at a position of the second trip, where the second call has short records
    at = [[N3 - 1 - p if reverse else p for p in AT3[which]] for which in sequence]
    assert max(at[0]) >= PLAN_THREADS * PLAN_BLOCKS_MAX > max(at[1])
    data = {w: batch_data(lens3(w), 800000 + k, 0, "wrap977", shared_key=True, refs=refs)
            for k, w in enumerate(("late", "early"))}
    with torch.cuda.stream(own_stream()):
        for mode in ("xor", "seal"):
            enet.set_seg_min(0)
            run_ops(enet, data1(), list(range(320)), tag_victim=None, ct_victim=None, ops=("seal",), want_seg=1,
                    tag="320 records before the plan's second trip")
            enet.set_seg_min(TILE)
            for which in sequence:
                run_sparse(enet, data[which], reverse, mode, f"{which} {'reversed' if reverse else 'in order'}")


# ------------------------------------------------------------------ 4. one-launch AEAD geometry
def uniform_case(enet, lens, hinted, seed):
    """Seal, open and tampered opens of a batch the hints call uniform (n x hinted bytes), AAD of 17
    bytes per record, twice on the stream (the arrival counters must be back at zero).  The
    tampered open flips one tag bit of record 0 and the last ciphertext byte (in the last tile) of
    the last record; a one-record batch takes the two flips in two opens."""
    n = len(lens)
    d = batch_data.__wrapped__(tuple(lens), seed, 0, "mod7", aad_lens=(17,), xor=False)
    kw = dict(hints=dict(total_bytes_hint=n * hinted, max_len_hint=hinted), want_seg=1,
              want_route=dict(), tag=f"{n} x {hinted}")
    last = (n - 1, lens[n - 1] - 1)
    for rep in range(2):
        if n > 1:
            run_ops(enet, d, None, tag_victim=0, ct_victim=last, ops=("seal", "open", "tamper"), **kw)
        else:
            run_ops(enet, d, None, tag_victim=0, ct_victim=None, ops=("seal", "open", "tamper"), **kw)
            run_ops(enet, d, None, tag_victim=None, ct_victim=last, ops=("tamper",), **kw)


@pytest.mark.parametrize("L", [40_000, 65_536, 131_072 - 5, 16 * 65536, 16 * 65536 + 1])
def test_uniform_aead_arrival_groups(enet, L):
    """T = 1 (ragged and whole: no combine, nw_t == 0), 2, 16 (16 groups of one member) and 17
    tiles (group 0 has two members, the others one): ng = min(T, 16), members = ceil((T - g) / ng)."""
    T = tiles_of(L)
    assert T == {40_000: 1, 65_536: 1, 131_067: 2, 1 << 20: 16, (1 << 20) + 1: 17}[L] and lq_of(T) == 0
    ng = min(T, 16)
    members = [(T - g + ng - 1) // ng for g in range(ng)]
    assert sum(members) == T and members == {1: [1], 2: [1, 1], 16: [1] * 16, 17: [2] + [1] * 15}[T]
    enet.set_seg_min(4096)
    uniform_case(enet, [L] * 3, L, 810000 + T)


LQ_CASES = {257: (257 * TILE, 0), 258: (258 * TILE, 1), 513: (513 * TILE, 1), 514: (514 * TILE, 2),
            2050: (2049 * TILE + 33, 4)}


@pytest.mark.parametrize("T", list(LQ_CASES))
def test_uniform_aead_combine_tiles_per_lane(enet, T):
    """One record of T tiles: the last arriver's combine runs 2^lq right-aligned tiles per lane,
    lq = 0 up to 257 tiles, 1 up to 513, 2 at 514, 4 at 2 050 (the power wave's table entries
    12 + lq + b).  T = 2 050 (last tile 33 bytes) needs 65 600 bytes of partials, past the 64 KiB
    floor: the buffer grows behind the launches before it, and a 5 x 300 KiB batch then runs inside
    the grown one."""
    import torch
    L, lq = LQ_CASES[T]
    assert tiles_of(L) == T and lq_of(T) == lq
    enet.set_seg_min(-1)
    if T != 2050:
        assert 32 * T <= PARTIALS_FLOOR
        uniform_case(enet, [L], L, 820000 + T)
        return
    assert 32 * T == 65600 > PARTIALS_FLOOR and L % TILE == 33
    with torch.cuda.stream(own_stream()):
        uniform_case(enet, [300 << 10] * 5, 300 << 10, 820005)  # allocates the floor
        uniform_case(enet, [L], L, 820000 + T)
        uniform_case(enet, [300 << 10] * 5, 300 << 10, 820005)


def test_uniform_aead_lying_hint_beside_lq2(enet):
    """Two records hinted as 514 tiles each; the second is 70 000 bytes longer and is run whole by
    its tile-0 workgroup, beside a neighbour combined at lq = 2."""
    L = LQ_CASES[514][0]
    assert lq_of(tiles_of(L)) == 2 and tiles_of(L + 70_000) == 516
    enet.set_seg_min(-1)
    uniform_case(enet, [L, L + 70_000], L, 830000)


# ------------------------------------------------------------------ 5. two streams, two threads
ROUNDS = 20
GROW_ROUNDS = (5, 12)


class OnDevice:
    """A batch_data batch and its oracle values as device tensors, with outputs of its own."""

    def __init__(self, enet, d, hints=None):
        import torch
        dev = lambda a: torch.from_numpy(np.array(a)).cuda()
        self.enet, self.d = enet, d
        self.hints = hints or dict(total_bytes_hint=sum(d.lens), max_len_hint=max(d.lens))
        self.offs, self.keys, self.nonces, self.aad, self.aoff = (dev(x) for x in (d.offs, d.keys, d.nonces, d.aad, d.aoff))
        self.pt, self.ct, self.xo, self.tags = dev(d.pt), dev(d.ct), dev(d.xo), dev(d.tags)
        self.ctr = dev(d.ctr.view(np.int32))
        self.out = torch.empty_like(self.pt)
        self.back = torch.empty_like(self.pt)
        self.tags_out = torch.empty_like(self.tags)
        self.ok = torch.empty(d.n, dtype=torch.uint8, device="cuda")

    def batch(self, arena):
        return self.enet.Batch(arena, self.offs, self.keys, self.nonces, key_stride=self.d.key_stride, **self.hints)

    def seal_open(self, s, open_too=True):
        """Flags (device scalars): ciphertext, tags, plaintext or verdicts differ from the oracle's."""
        for t in (self.out, self.back, self.tags_out, self.ok):
            t.fill_(FILL)
        self.enet.aead_seal(self.batch(self.pt), self.out, self.tags_out, self.aad, self.aoff, stream=s)
        g = self.d.base  # the gap before the first record stays as prefilled
        bad = [(self.out[g:] != self.ct[g:]).any(), (self.tags_out != self.tags).any()]
        if open_too:
            self.enet.aead_open(self.batch(self.out), self.back, self.tags_out, self.ok, self.aad, self.aoff, stream=s)
            bad += [(self.back[g:] != self.pt[g:]).any(), (self.ok != 1).any()]
        return bad

    def xor(self, s):
        self.out.fill_(FILL)
        self.enet.chacha20_xor(self.batch(self.pt), self.out, self.ctr, stream=s)
        return [(self.out[self.d.base:] != self.xo[self.d.base:]).any()]


def test_two_streams_two_threads(enet):
    """Two threads, each with its own stream, data, outputs and (long_records.cpp) tile scratch, 20
    rounds each under set_seg_min(0): one-launch seal + open of 6 x 53 tiles, planned ChaCha20 of
    the ragged-tile shape of test_gpu_segments.py, one-launch seal + open of 5 x 300 KiB.  In rounds
    5 and 12 thread B also seals 1 x 33 MiB and the 4 300 records of test 1: the latter's plan
    scratch (3.8 MB, row 108) replaces B's 256 KiB one while A's launches are in flight.  Expected
    values are the oracle's, computed and uploaded before the threads start; a thread compares on
    its stream and synchronises it once per round.  No mismatch in any round on either thread."""
    import torch
    ragged = tuple(shapes()["ragged_tiles_forced"][0])
    assert seg_layout(len(ragged), max(ragged), sum(ragged), 0)["bytes"] <= PLAN_FLOOR < seg_layout(N1, max(LENS1), sum(LENS1), 0)["bytes"]
    enet.set_seg_min(0)
    cases = {}
    for k, name in enumerate("AB"):
        seed = 840000 + 1000 * k
        cases[name] = dict(
            h53=OnDevice(enet, batch_data.__wrapped__((H53,) * 6, seed, 0, "mod7", aad_lens=(17,), xor=False)),
            ragged=OnDevice(enet, batch_data.__wrapped__(ragged, seed + 1, 0, "wrap977")),
            k300=OnDevice(enet, batch_data.__wrapped__((300 << 10,) * 5, seed + 2, 0, "mod7", aad_lens=(17,), xor=False)))
    cases["B"]["big"] = OnDevice(enet, batch_data.__wrapped__((33 * MiB,), 842000, 0, "mod7", aad_lens=(17,), xor=False))
    cases["B"]["many"] = OnDevice(enet, data1())
    torch.cuda.synchronize()
    streams = {name: torch.cuda.Stream() for name in "AB"}
    assert streams["A"].cuda_stream != streams["B"].cuda_stream
    wrong, errors = [], []
    seg0 = enet.seg_batches()

    def work(name):
        try:
            c, s = cases[name], streams[name]
            with torch.cuda.stream(s):
                for r in range(ROUNDS):
                    bad = c["h53"].seal_open(s) + c["ragged"].xor(s) + c["k300"].seal_open(s)
                    if name == "B" and r in GROW_ROUNDS:
                        bad += c["big"].seal_open(s, open_too=False) + c["many"].seal_open(s, open_too=False)
                    flags = torch.stack(bad)
                    s.synchronize()
                    hit = flags.cpu().tolist()
                    if any(hit):
                        wrong.append((name, r, hit))
        except Exception as e:  # reported by the main thread
            errors.append((name, repr(e)))

    threads = [threading.Thread(target=work, args=(name,)) for name in "AB"]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert not wrong, f"(thread, round, flags) with bytes that differ from the oracle's: {wrong[:6]}"
    assert enet.seg_batches() - seg0 == 2 * ROUNDS * 5 + len(GROW_ROUNDS) * 2
