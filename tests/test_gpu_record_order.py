"""A caller's `order` and unknown hints on the cipher calls (enet_chacha20_xor_batch,
enet_aead_seal_batch, enet_aead_open_batch): every path an `order` or hints 0 / 0 can reach.

include/enet_crypto.h makes `order` "optional [count] record indices to process, in this order
(e.g. longest first, or one length class of a larger batch)"; the indices address the offsets, keys,
nonces, tags and verdicts of the FULL batch and may be >= count.  The cases:
  a. a permutation of a mixed batch on the per-lane record kernel, at every lane count;
  b. a uniform batch whose hints would take the streaming / lockstep kernels: with an order it
     must run per lane (those kernels address record g at in_offsets[0] + g L);
  c. a subset with high indices (31 of 96 records) on the record engine;
  d. a subset with high indices on the plan + tiles path (segments.hip), whose claim bytes are
     kept per position of the launch, then a second subset on the same stream;
  e. hints 0 / 0 ("unknown") under a forced tile threshold of 0, which must still write every
     record (a one-launch uniform route sized by those hints would hold no tile).
Every output arena (with a 256-byte guard on each side and the base_offset gap), the tags and the
verdicts are prefilled with 0x5A: named records must come out bit-exact as the CPU oracle's, and
every byte of a record the order does not name -- output range, 16 tag bytes, verdict -- and of
the guards must still be 0x5A.  A subset call's hints describe the named records (their sum and
their maximum).  References are computed once per batch and shared."""
import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

KINDS = ("PerLane", "RunStaged", "LineStaged", "Lockstep", "Stream")
GUARD = 256
FILL = 0x5A
# block, Poly1305-block and lane-run edges; the last is one byte short of 5 blocks for each of 16 lanes
EDGE_LENS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4096 + 44, 64 * 16 * 5 - 1)
AAD_LENS = (0, 1, 16, 17)


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
    print(f"\n[record order] module wall time {time.time() - t0:.1f} s")


@functools.lru_cache(maxsize=None)
def batch_data(lens, seed, base, ctr_kind, aad_lens=AAD_LENS, shared_key=False, refs=None, xor=True):
    """A batch of len(lens) records starting at `base` in its arena, and the oracle's seal
    (AAD lengths cycling through aad_lens: 0, 1, 16, 17), and ChaCha20 (per-record start counters)
    of every record, laid out like the arena.  Computed once per batch; nothing mutates it.
    shared_key: one key for the batch (key_stride 0).  refs: the records to compute the oracle's
    values for (a tuple; None = all: the others' ranges of ct / xo / tags stay zero, for batches too
    large to check in full).  xor = False leaves xo zero (AEAD-only batches of many MiB).
    batch_data.__wrapped__ builds a batch without keeping it."""
    n = len(lens)
    offs = (base + np.concatenate([[0], np.cumsum(lens)])).astype(np.int64)
    size = max(int(offs[-1]), 1)
    pt = np.zeros(size, dtype=np.uint8)
    pt[base:int(offs[-1])] = np.frombuffer(splitmix_bytes(seed, int(offs[-1]) - base), dtype=np.uint8)
    keys = splitmix_bytes(seed + 1, 32 * (1 if shared_key else n))
    nonces = splitmix_bytes(seed + 2, 12 * n)
    aoff = np.concatenate([[0], np.cumsum([aad_lens[i % len(aad_lens)] for i in range(n)])]).astype(np.int64)
    aad = splitmix_bytes(seed + 3, int(aoff[-1]))
    if ctr_kind == "mod7":  # the u32 wrap falls before one of the first seven blocks, or nowhere
        ctr = np.array([(-(i % 7)) & 0xFFFFFFFF for i in range(n)], dtype=np.uint32)
    else:                   # up to 4096 blocks short of the wrap: inside the long records
        ctr = np.array([0xFFFFFFFF - (i * 977) % 4096 for i in range(n)], dtype=np.uint32)
    ct, xo = np.zeros_like(pt), np.zeros_like(pt)
    tags = np.zeros(16 * n, dtype=np.uint8)
    for i in (range(n) if refs is None else refs):
        k = keys[:32] if shared_key else keys[32 * i:32 * i + 32]
        nn = nonces[12 * i:12 * i + 12]
        m = pt[offs[i]:offs[i + 1]].tobytes()
        c, t = oracle.aead_seal(k, nn, m, aad[aoff[i]:aoff[i + 1]])
        ct[offs[i]:offs[i + 1]] = np.frombuffer(c, dtype=np.uint8)
        tags[16 * i:16 * i + 16] = np.frombuffer(t, dtype=np.uint8)
        if xor:
            xo[offs[i]:offs[i + 1]] = np.frombuffer(oracle.chacha20_xor(k, nn, m, int(ctr[i])), dtype=np.uint8)
    for a in (offs, pt, aoff, ctr, ct, xo, tags):
        a.setflags(write=False)
    as_u8 = lambda b: np.frombuffer(b or b"\0", dtype=np.uint8)
    return SimpleNamespace(n=n, lens=lens, base=base, offs=offs, size=size, pt=pt, keys=as_u8(keys),
                           key_stride=0 if shared_key else 32, refs=refs, nonces=as_u8(nonces), aad=as_u8(aad), aoff=aoff, ctr=ctr, ct=ct, xo=xo, tags=tags)


class Guarded:
    """nbytes of device memory between two GUARD-byte guards, all of it FILL (or `data` inside)."""

    def __init__(self, nbytes, data=None):
        import torch
        self.big = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        self.view = self.big[GUARD:GUARD + nbytes]
        if data is not None:
            self.view.copy_(torch.from_numpy(np.array(data)))

    def host(self):
        h = self.big.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[-GUARD:] == FILL).all(), "guard bytes overwritten"
        return h[GUARD:-GUARD]


def only_named(full, bounds, named):
    """FILL everywhere except the named records' ranges [bounds[i], bounds[i+1]), taken from `full`."""
    e = np.full(full.shape, FILL, dtype=np.uint8)
    for i in named:
        e[bounds[i]:bounds[i + 1]] = full[bounds[i]:bounds[i + 1]]
    return e


def same(got, want, bounds, what):
    d = np.flatnonzero(got != want)
    if d.size:
        rec = int(np.searchsorted(bounds, d[0], side="right") - 1)
        raise AssertionError(f"{what}: first wrong byte {int(d[0])} (record {rec}): got {int(got[d[0]]):#x}, "
                             f"want {int(want[d[0]]):#x}; {d.size} bytes differ")


def run_ops(enet, d, order, *, tag_victim, ct_victim, aad_victim=None, hints=None, want_route=None, want_seg=None,
            ops=("xor", "seal", "open", "tamper"), tag=""):
    """The cipher calls over the records `order` names (None: all, in batch order) of batch d, each
    into prefilled outputs, each checked as the module text says.  tag_victim: a named record whose
    tag gets one bit flipped, ct_victim = (named record, byte of it to flip), aad_victim: a third
    named record whose first AAD byte is flipped, for the tampered open (None: no such flip).
    want_route / want_seg: what every call must add to record_route_counts() / seg_batches().
    Returns the outputs (host arrays) by name."""
    import torch
    assert d.refs is None, "run_ops compares every record"
    named = list(range(d.n)) if order is None else [int(i) for i in order]
    victims = [v for v in (tag_victim, ct_victim and ct_victim[0], aad_victim) if v is not None]
    assert len(set(named)) == len(named) and set(victims) <= set(named) and len(set(victims)) == len(victims)
    if hints is None:  # of the named records
        hints = dict(total_bytes_hint=sum(d.lens[i] for i in named), max_len_hint=max(d.lens[i] for i in named))
    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    toffs, keys, nonces, aad, aoff = dev(d.offs), dev(d.keys), dev(d.nonces), dev(d.aad), dev(d.aoff)
    tord = None if order is None else torch.tensor(named, dtype=torch.int32, device="cuda")
    batch = lambda arena: enet.Batch(arena, toffs, keys, nonces, key_stride=d.key_stride, order=tord,
                                     count=None if order is None else len(named), **hints)
    b16, b1 = 16 * np.arange(d.n + 1), np.arange(d.n + 1)

    def launch(fn, *a):
        r0, s0 = enet.record_route_counts(), enet.seg_batches()
        fn(*a)
        r1, s1 = enet.record_route_counts(), enet.seg_batches()
        delta = {k: r1[k] - r0[k] for k in KINDS}
        if want_route is not None:
            assert delta == dict(dict.fromkeys(KINDS, 0), **want_route), (tag, fn.__name__, delta, want_route)
        if want_seg is not None:
            assert s1 - s0 == want_seg, (tag, fn.__name__, "seg_batches moved by", s1 - s0)

    res = {}
    pt_in, ct_in = dev(d.pt), dev(d.ct)
    if "xor" in ops:
        out = Guarded(d.size)
        launch(enet.chacha20_xor, batch(pt_in), out.view, dev(d.ctr.view(np.int32)))
        res["xor"] = out.host()
        same(res["xor"], only_named(d.xo, d.offs, named), d.offs, f"{tag} chacha20 xor")
    if "seal" in ops:
        out, tags = Guarded(d.size), Guarded(16 * d.n)
        launch(enet.aead_seal, batch(pt_in), out.view, tags.view, aad, aoff)
        res["seal"], res["seal_tags"] = out.host(), tags.host()
        same(res["seal"], only_named(d.ct, d.offs, named), d.offs, f"{tag} seal ciphertext")
        same(res["seal_tags"], only_named(d.tags, b16, named), b16, f"{tag} seal tags")
    ones = np.ones(d.n, dtype=np.uint8)
    if "open" in ops:
        out, ok = Guarded(d.size), Guarded(d.n)
        launch(enet.aead_open, batch(ct_in), out.view, dev(d.tags), ok.view, aad, aoff)
        res["open"], res["open_ok"] = out.host(), ok.host()
        same(res["open_ok"], only_named(ones, b1, named), b1, f"{tag} open verdicts")
        same(res["open"], only_named(d.pt, d.offs, named), d.offs, f"{tag} open plaintext")
    if "tamper" in ops:
        assert victims
        bad_ct, bad_tags, bad_aad = ct_in.clone(), dev(d.tags), aad.clone()
        if tag_victim is not None:
            bad_tags[16 * tag_victim + 5] ^= 0x08
        if ct_victim is not None:
            v, pos = ct_victim
            assert 0 <= pos < d.lens[v]
            bad_ct[int(d.offs[v]) + pos] ^= 0x20
        if aad_victim is not None:
            assert d.aoff[aad_victim + 1] > d.aoff[aad_victim]
            bad_aad[int(d.aoff[aad_victim])] ^= 0x01
        out, ok = Guarded(d.size), Guarded(d.n)
        launch(enet.aead_open, batch(bad_ct), out.view, bad_tags, ok.view, bad_aad, aoff)
        want_pt, want_ok = d.pt.copy(), ones.copy()
        for f in victims:  # no verdict, no plaintext
            want_pt[d.offs[f]:d.offs[f + 1]] = 0
            want_ok[f] = 0
        res["tamper"], res["tamper_ok"] = out.host(), ok.host()
        same(res["tamper_ok"], only_named(want_ok, b1, named), b1, f"{tag} tampered open verdicts")
        same(res["tamper"], only_named(want_pt, d.offs, named), d.offs, f"{tag} tampered open plaintext")
    return res


# ------------------------------------------------------------------ a. permuted order, per lane
N_A = 40
LENS_A = (EDGE_LENS * 3)[:N_A]


@pytest.mark.parametrize("how", ["longest_first", "reversed"])
@pytest.mark.parametrize("P", [1, 2, 4, 8, 16])
def test_permuted_order_on_the_record_engine(enet, P, how):
    """40 records of the edge lengths, base_offset 3, processed longest first (stable argsort,
    reversed) or in reverse: every launch hands exactly 40 records to the per-lane kernel; ChaCha20
    with start counters 2^32 - i mod 7 (the u32 wrap inside the records), seal with AAD, open, and an
    open with a flipped tag bit on one record and a flipped ciphertext byte in the last partial
    block of another (those two: ok = 0 and zeros; all others ok = 1 and plaintext).  The same calls
    without an order give the same bytes."""
    d = batch_data(LENS_A, 710000, 3, "mod7")
    if how == "longest_first":
        order = np.argsort(np.array(LENS_A), kind="stable")[::-1].copy()
    else:
        order = np.arange(N_A)[::-1].copy()
    enet.set_seg_min(-1)
    enet.set_staging(-1)
    enet.set_lanes_per_record(P)
    v = 14  # 4096 + 44 bytes: the last block holds 44
    assert LENS_A[v] % 64 == 44
    kw = dict(tag_victim=21, ct_victim=(v, LENS_A[v] - 3), want_route={"PerLane": N_A}, want_seg=0)
    got = run_ops(enet, d, order, tag=f"P {P} {how}", **kw)
    plain = run_ops(enet, d, None, tag=f"P {P} no order", **kw)
    for k in got:
        assert np.array_equal(got[k], plain[k]), (P, how, k, "differs from the call without an order")


# ------------------------------------------------------------------ b. uniform hints and an order
@pytest.mark.parametrize("staging", [1, 5])
@pytest.mark.parametrize("P", [1, 4, 16])
def test_uniform_hints_with_an_order_run_per_lane(enet, P, staging):
    """L = 128 P 2 bytes, n = 512 / P + 3 records, truthful uniform hints: without an order the
    whole 512-lane workgroup is the streaming kernel's under staging 1 (the lockstep kernel's under
    staging 5) and 3 records run per lane.  Those kernels take record g from in_offsets[0] + g L:
    with an order (reversed) all n records must go to the per-lane kernel and nothing elsewhere;
    seal, open and ChaCha20 bit-exact."""
    L, per = 128 * P * 2, 512 // P
    n = per + 3
    d = batch_data((L,) * n, 720000 + P, 0, "mod7")
    hints = dict(total_bytes_hint=n * L, max_len_hint=L)
    enet.set_seg_min(-1)
    enet.set_lanes_per_record(P)
    enet.set_staging(staging)
    kw = dict(tag_victim=1, ct_victim=(n - 2, L - 1), hints=hints, want_seg=0)
    staged = "Stream" if staging == 1 else "Lockstep"
    run_ops(enet, d, None, want_route={staged: per, "PerLane": 3}, tag=f"P {P} staging {staging} no order", **kw)
    run_ops(enet, d, np.arange(n)[::-1], want_route={"PerLane": n}, tag=f"P {P} staging {staging} reversed", **kw)
    enet.set_staging(-1)


# ------------------------------------------------------------------ c. subset, record engine
N_C = 96
LENS_C = EDGE_LENS * 6


def subset_c():
    """31 of the 96 records, in no monotone order, N-1 and N-2 among them."""
    perm = np.argsort(np.frombuffer(splitmix_bytes(730001, 4 * N_C), "<u4"), kind="stable").tolist()
    pick = [i for i in perm if i not in (N_C - 1, N_C - 2)][:29]
    pick.insert(1, N_C - 1)
    pick.insert(6, N_C - 2)
    return pick


@pytest.mark.parametrize("P", [1, 4])
def test_subset_with_high_indices_on_the_record_engine(enet, P):
    """count = 31 of N = 96 records with the tiles switched off: counters, keys, nonces, AAD, tags
    and verdicts are taken at the record's index (up to 95), not at its position (below 31), and the
    65 records the order leaves out are not touched."""
    order = subset_c()
    assert len(order) == 31 and len(set(order)) == 31 and {N_C - 1, N_C - 2} <= set(order)
    assert sum(i >= 31 for i in order) >= 5
    steps = np.sign(np.diff(order))
    assert (steps > 0).any() and (steps < 0).any(), "the order must not be monotone"
    d = batch_data(LENS_C, 730000, 3, "mod7")
    enet.set_seg_min(enet.SEG_NEVER)
    enet.set_staging(-1)
    enet.set_lanes_per_record(P)
    tv = N_C - 1                                   # 5119 bytes
    cv = max((i for i in order if i != tv), key=lambda i: LENS_C[i])
    assert LENS_C[cv] > 64
    run_ops(enet, d, order, tag_victim=tv, ct_victim=(cv, LENS_C[cv] // 2), want_route={"PerLane": 31},
            want_seg=0, ops=("xor", "seal", "tamper"), tag=f"subset P {P}")
    enet.set_seg_min(-1)


# ------------------------------------------------------------------ d. subset, plan + tiles
N_D = 1024
LONG_D = {600: 65553, 777: 131072, 900: 196607, 1023: 200000}
LENS_D = tuple(LONG_D.get(i, 40) for i in range(N_D))


def test_subset_with_high_indices_on_plan_and_tiles(enet):
    """N = 1024 records of 40 bytes, except 65 553, 131 072, 196 607 and 200 000 bytes at indices 600,
    777, 900 and 1023; the order names indices 512 .. 1023, longest first; count = 512; threshold
    64 KiB (set_seg_min(65536)).  The call's scratch (long_route.hpp seg_layout, pinned as layout
    row 101 of tests/cpp/route_table.cpp), from the hints of the named records:
        total = 508 * 40 + 65 553 + 131 072 + 196 607 + 200 000 = 613 552, max 200 000
        ecap  = min(512, 613 552 / 65 536 + 1) = 10 entries of sizeof(SegEntry) = 864 bytes
        tcap  = 613 552 / 65 536 + ecap + 1 = 20 tiles
        o_cl  = 256 + 10 * 864 = 8 896                  claim bytes, count = 512 of them
        o_part = roundup256(8 896 + 512) = 9 472        partials, 32 bytes per tile
    The four long records claim 2 + 2 + 3 + 4 = 11 tiles, so the partials in use are bytes
    [9 472, 9 824).  The claim bytes used to be indexed by RECORD: claimed[i] for i = 576 .. 927 lay
    at 8 896 + i inside those partials (claimed[1023] at 9 919, behind them).  The tile kernels
    overwrote them with Poly1305 sums, the record kernel read the sums as skip flags, and under seal /
    open a 40-byte record there was skipped (left at 0x5A) or a claimed one run twice.  Indexed by
    position (seg_claim_slot) the bytes in use are [8 896, 9 408), whatever the order names.
    Checked here: ChaCha20 with counters that wrap inside each long record, seal with AAD, open, and
    an open with the 200 000-byte record's tag and a middle byte of the 196 607-byte record
    flipped (both zeroed with ok = 0, every other named record intact); each call is one more
    seg_batches().  Then a second subset of the same batch on the same stream, indices 0 .. 511,
    all short: claim bytes the first calls set for positions 0 .. 3 must not survive into it."""
    d = batch_data(LENS_D, 740000, 3, "wrap977")
    named = list(range(512, N_D))
    order = [named[k] for k in np.argsort(np.array([LENS_D[i] for i in named]), kind="stable")[::-1]]
    assert order[:4] == [1023, 900, 777, 600] and len(order) == 512
    assert sum(LENS_D[i] for i in order) == 613552
    assert sum((L + 65535) // 65536 for L in LONG_D.values()) == 11
    for i, L in LONG_D.items():  # the u32 counter wraps inside each long record
        assert 0 < (1 << 32) - int(d.ctr[i]) < (L + 63) // 64
    enet.set_lanes_per_record(0)
    enet.set_staging(-1)
    enet.set_seg_min(65536)
    run_ops(enet, d, order, tag_victim=1023, ct_victim=(900, LENS_D[900] // 2), want_route={"PerLane": 512},
            want_seg=1, tag="tiles subset 512..1023")
    second = list(range(512))[::-1]
    run_ops(enet, d, second, tag_victim=3, ct_victim=(500, 39), want_route={"PerLane": 512}, want_seg=1,
            tag="tiles subset 511..0")
    enet.set_seg_min(-1)


# ------------------------------------------------------------------ e. unknown hints, forced tiles
LENS_E = (0, 1, 100, 65537, 200000)


@pytest.mark.parametrize("seg_min", [0, -1], ids=["forced_tiles", "record_engine_control"])
def test_unknown_hints_write_every_record(enet, seg_min):
    """total_bytes_hint = max_len_hint = 0 means "unknown" (enet_crypto.h).  Under set_seg_min(0)
    such a batch used to count as uniform of length 0 and took a one-launch route of no tiles: success
    returned, nothing written.  It is planned now (capacities from the hints: 5 entries, 6 tiles; a
    record past them stays with the record engine): every record bit-exact, and no byte, tag or
    verdict of it left at 0x5A.  With the automatic threshold the same hints take the record engine."""
    d = batch_data(LENS_E, 750000, 3, "wrap977")
    enet.set_lanes_per_record(0)
    enet.set_staging(-1)
    enet.set_seg_min(seg_min)
    res = run_ops(enet, d, None, tag_victim=3, ct_victim=(4, 199_999), hints=dict(total_bytes_hint=0, max_len_hint=0),
                  want_seg=1 if seg_min == 0 else 0, tag=f"hints 0/0 seg_min {seg_min}")
    for k in ("seal_tags", "open_ok", "tamper_ok"):
        width = 16 if k == "seal_tags" else 1
        for i in range(d.n):
            assert not (res[k][width * i:width * (i + 1)] == FILL).all(), (k, "record", i, "never written")
    for k in ("xor", "seal", "open"):
        for i in (3, 4):  # 64 KiB + 1 and 200 000 bytes: no 16-byte piece left at the prefill
            body = res[k][d.offs[i]:d.offs[i + 1]]
            pieces = body[:len(body) // 16 * 16].reshape(-1, 16)
            assert not (pieces == FILL).all(axis=1).any(), (k, "record", i, "has unwritten bytes")
    enet.set_seg_min(-1)
