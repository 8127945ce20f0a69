"""Every lane count of the uniform record kernels, with the kernel each batch ran on confirmed.

launch_one (csrc/records.hip) picks between five kernels -- streaming, lockstep run-staged, plain
run-staged, line-staged and per-lane -- by csrc/record_route.hpp.  Each case here first checks the
routing counter (enet_record_route_counts): the launch must have handed full * per_wg records to the
intended kind and the rest to the per-lane kernel.  Only then the bytes: seal, open and reference-mode
ChaCha20 of every record bit-exact against the CPU oracle.

Shapes: P lanes per record in {1, 2, 4, 8, 16}; L = 64 P B - r with B (blocks per lane) in
{2, 4, 5, 6} and r in {0, 1, 44}; n = full (512 / P) + 3 records, full = max(2, ceil((P B + 1) /
(512 / P))).  Under staging 1, r = 0 with B = 2, 4, 6 is the streaming kernel at 1, 2 and 3 stages
(prologue DMA + final stores only; no stage with both a previous and a next one; one steady-state
stage), one lane with r = 44 is line-staged, the rest lockstep.  Staging 5 and 4 run the same
lengths on the lockstep and the 256-thread staged kernel (0 to 3 staged stages, then an odd whole
block and / or a partial block per lane); staging 0 is the per-lane baseline.
ChaCha20 start counters are (2^32 - i mod (P B + 1)) mod 2^32 for record i, so that inside the
full workgroups the u32 wrap falls before every block of a record, lane boundaries and both
blocks of a stage included, and after the last one."""
import functools
import math
import time
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

LANES = [1, 2, 4, 8, 16]
STAGINGS = [1, 4, 5, 0]
BS = [2, 4, 5, 6]
RS = [0, 1, 44]
KINDS = ("PerLane", "RunStaged", "LineStaged", "Lockstep", "Stream")
GUARD = 256
FILL = 0x5A


@pytest.fixture(scope="module")
def enet():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ephemeralnet_amd as E
    E.lib()
    E.set_seg_min(-1)
    t0 = time.time()
    yield E
    E.set_lanes_per_record(0)
    E.set_staging(-1)
    print(f"\n[uniform matrix] module wall time {time.time() - t0:.1f} s")


def shape(P, B, r):
    per = 512 // P
    full = max(2, math.ceil((P * B + 1) / per))
    return 64 * P * B - r, full * per + 3, full


def expected_route(staging, P, B, r, n):
    """(kind, records in whole workgroups, records left per lane), from the kernels' requirements:
    the streaming kernel needs L % (128 P) == 0, line staging one lane and L % 64 != 0, L % 4 == 0;
    the lockstep and streaming kernels hold 512 lanes per workgroup, the others 256."""
    if staging == 0:
        return "PerLane", 0, n
    if staging == 4:
        kind, per = "RunStaged", 256 // P
    elif staging == 5:
        kind, per = "Lockstep", 512 // P
    elif r == 0 and B % 2 == 0:
        kind, per = "Stream", 512 // P
    elif P == 1 and r == 44:
        kind, per = "LineStaged", 256
    else:
        kind, per = "Lockstep", 512 // P
    return kind, (n // per) * per, n % per


@functools.lru_cache(maxsize=None)
def case_data(P, B, r, shared_key=False, lying=False):
    """Inputs and oracle outputs of one shape, computed once and shared by every staging."""
    L, n, full = shape(P, B, r)
    lens = [L] * n
    if lying:  # two records of the second 512-lane workgroup; the lengths still sum to n L
        per = 512 // P
        lens[per + 3] -= 64
        lens[per + 10] += 64
    seed = 500000 + 10000 * P + 100 * B + r + (7 if shared_key else 0) + (13 if lying else 0)
    return make_case(P, B, L, tuple(lens), seed, shared_key)


def make_case(P, B, L, lens, seed, shared_key=False):
    """n = len(lens) records under the hints (n L, L); B = blocks per lane of an L-byte record."""
    n, full = len(lens), len(lens) // (512 // P)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pt = splitmix_bytes(seed, int(offs[-1]))
    keys = splitmix_bytes(seed + 1, 32 if shared_key else 32 * n)
    nonces = splitmix_bytes(seed + 2, 12 * n)
    alens = [[0, 1, 16, 17][i % 4] for i in range(n)]
    aoff = np.concatenate([[0], np.cumsum(alens)]).astype(np.int64)
    aad = splitmix_bytes(seed + 3, int(aoff[-1]))
    ctr = np.array([(-(i % (P * B + 1))) & 0xFFFFFFFF for i in range(n)], dtype=np.uint32)
    ct, tags, xo = [], [], []
    for i in range(n):
        k = keys[:32] if shared_key else keys[32 * i:32 * i + 32]
        nn = nonces[12 * i:12 * i + 12]
        m = pt[offs[i]:offs[i + 1]]
        c, t = oracle.aead_seal(k, nn, m, aad[aoff[i]:aoff[i + 1]])
        ct.append(c)
        tags.append(t)
        xo.append(oracle.chacha20_xor(k, nn, m, int(ctr[i])))
    as_u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
    return SimpleNamespace(P=P, B=B, L=L, n=n, full=full, lens=lens, offs=offs, pt=as_u8(pt), keys=as_u8(keys),
                           nonces=as_u8(nonces), aad=as_u8(aad), aoff=aoff, ctr=ctr, ct=as_u8(b"".join(ct)),
                           tags=as_u8(b"".join(tags)), xo=as_u8(b"".join(xo)), key_stride=0 if shared_key else 32)


def first_bad(got, want, offs):
    """Index of the first record whose bytes differ (for the assertion message)."""
    d = np.flatnonzero(got != want)
    return None if d.size == 0 else int(np.searchsorted(offs, d[0], side="right") - 1)


class Arena:
    """A device arena of nbytes at GUARD + shift inside an allocation filled with FILL."""

    def __init__(self, nbytes, shift=0, data=None):
        import torch
        self.big = torch.full((nbytes + 2 * GUARD + shift,), FILL, dtype=torch.uint8, device="cuda")
        self.lo, self.hi = GUARD + shift, GUARD + shift + nbytes
        self.view = self.big[self.lo:self.hi]
        if data is not None:
            self.view.copy_(data if torch.is_tensor(data) else torch.from_numpy(np.array(data)))

    def host(self):
        h = self.big.cpu().numpy()
        assert (h[:self.lo] == FILL).all() and (h[self.hi:] == FILL).all(), "guard bytes overwritten"
        return h[self.lo:self.hi]


def run_case(enet, d, staging, want, ishift=0, oshift=0, victims=None):
    """One shape on one staging variant: `want` = (kind, records in whole workgroups, rest);
    victims = {record: byte to flip} for the tampered open (default: three records of the first two
    512-lane workgroups)."""
    import torch
    P, n, L, offs = d.P, d.n, d.L, d.offs
    total = int(offs[-1])
    enet.set_lanes_per_record(P)
    enet.set_staging(staging)
    want_delta = dict.fromkeys(KINDS, 0)
    want_delta[want[0]] += want[1]
    want_delta["PerLane"] += want[2]
    tag = (staging, P, L, n)

    def routed(fn, *a):
        """Run one batch call; its launches must be the intended kernel's, checked before any byte."""
        before = enet.record_route_counts()
        fn(*a)
        after = enet.record_route_counts()
        delta = {k: after[k] - before[k] for k in KINDS}
        assert delta == want_delta, (tag, fn.__name__, delta, want_delta)

    dev = lambda a: torch.from_numpy(np.array(a)).cuda()
    toffs, keys, nonces = dev(offs), dev(d.keys), dev(d.nonces)
    aad, aoff = dev(d.aad), dev(d.aoff)
    hints = dict(key_stride=d.key_stride, total_bytes_hint=n * L, max_len_hint=L)
    batch = lambda arena: enet.Batch(arena, toffs, keys, nonces, **hints)

    # ---- seal into a fresh guarded arena
    src = Arena(total, ishift, d.pt)
    out = Arena(total, oshift)
    tags = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
    routed(enet.aead_seal, batch(src.view), out.view, tags, aad, aoff)
    got = out.host()
    assert np.array_equal(got, d.ct), (tag, "seal ciphertext, record", first_bad(got, d.ct, offs))
    th = tags.cpu().numpy()
    assert np.array_equal(th, d.tags), (tag, "seal tag, record", first_bad(th, d.tags, 16 * np.arange(n + 1)))
    # ---- in place
    inp = Arena(total, ishift, d.pt)
    tags_ip = torch.zeros_like(tags)
    routed(enet.aead_seal, batch(inp.view), inp.view, tags_ip, aad, aoff)
    got = inp.host()
    assert np.array_equal(got, d.ct), (tag, "in-place seal, record", first_bad(got, d.ct, offs))
    assert np.array_equal(tags_ip.cpu().numpy(), d.tags), (tag, "in-place tags")
    # ---- open round trip
    back = Arena(total, ishift)
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    routed(enet.aead_open, batch(out.view), back.view, tags, ok, aad, aoff)
    okh = ok.cpu().numpy()
    assert okh.tolist() == [1] * n, (tag, "open verdicts", np.flatnonzero(okh != 1)[:8])
    got = back.host()
    assert np.array_equal(got, d.pt), (tag, "open plaintext, record", first_bad(got, d.pt, offs))
    # ---- tamper: first / middle / last byte of three records of the whole workgroups, one AAD byte
    per = 512 // P
    if victims is None:
        victims = {1: 0, per + 2: d.lens[per + 2] // 2, 2 * per - 2: d.lens[2 * per - 2] - 1}
    aad_victim = 5
    bad = Arena(total, oshift, out.view).view
    for v, pos in victims.items():
        bad[int(offs[v]) + pos] ^= 0x04
    bad_aad = aad.clone()
    assert d.aoff[aad_victim + 1] > d.aoff[aad_victim]
    bad_aad[int(d.aoff[aad_victim])] ^= 0x10
    failed = sorted(list(victims) + [aad_victim])
    back = Arena(total, ishift)
    ok.fill_(7)
    routed(enet.aead_open, batch(bad), back.view, tags, ok, bad_aad, aoff)
    okh = ok.cpu().numpy()
    assert np.flatnonzero(okh == 0).tolist() == failed and int(okh.sum()) == n - len(failed), (tag, okh)
    wantpt = d.pt.copy()
    for v in failed:
        wantpt[offs[v]:offs[v + 1]] = 0
    got = back.host()
    assert np.array_equal(got, wantpt), (tag, "tampered open, record", first_bad(got, wantpt, offs))
    # ---- reference-mode ChaCha20 with the start counters at the u32 wrap
    if d.n >= 2 * per:  # (every matrix shape)
        wraps = {int(-int(c)) & 0xFFFFFFFF for c in d.ctr[:d.full * per]}
        assert wraps >= set(range(P * d.B + 1)), "the full workgroups miss a wrap position"
    xo = Arena(total, oshift)
    routed(enet.chacha20_xor, batch(src.view), xo.view, torch.from_numpy(d.ctr.view(np.int32)).cuda())
    got = xo.host()
    assert np.array_equal(got, d.xo), (tag, "chacha20 xor, record", first_bad(got, d.xo, offs))
    print(f"[uniform matrix] staging {staging} P {P:2d} L {L:5d} n {n:4d}: {want[0]} {want[1]} + per-lane {want[2]} ok")


@pytest.mark.parametrize("P", LANES)
@pytest.mark.parametrize("staging", STAGINGS)
def test_uniform_matrix(enet, staging, P):
    """Every length of the matrix on one staging variant and lane count (see the module text)."""
    for B in BS:
        for r in RS:
            d = case_data(P, B, r)
            assert d.n * d.L <= 1 << 20
            want = expected_route(staging, P, B, r, d.n)
            assert want[2] == (d.n if staging == 0 else 3)
            run_case(enet, d, staging, want)
    enet.set_staging(-1)


@pytest.mark.parametrize("P", LANES)
def test_uniform_matrix_shared_key(enet, P):
    """One key for the whole batch (key_stride 0): the 3-stage streaming shape, and B = 5, r = 44
    on the lockstep (one lane: line-staged) and the plain staged kernels."""
    for staging, B, r in [(1, 6, 0), (1, 5, 44), (4, 5, 44)]:
        d = case_data(P, B, r, shared_key=True)
        run_case(enet, d, staging, expected_route(staging, P, B, r, d.n))
    enet.set_staging(-1)


@pytest.mark.parametrize("P", LANES)
def test_stream_shapes_shifted_arenas(enet, P):
    """The streaming shapes (1, 2 and 3 stages) with the input arena 4 and the output arena 12
    bytes off alignment: the LDS DMAs and whole-run stores then move unaligned 16-byte pieces."""
    for B in (2, 4, 6):
        d = case_data(P, B, 0)
        want = expected_route(1, P, B, 0, d.n)
        assert want[0] == "Stream"
        run_case(enet, d, 1, want, ishift=4, oshift=12)
    enet.set_staging(-1)


@pytest.mark.parametrize("P", LANES)
def test_stream_lying_hints(enet, P):
    """The 3-stage streaming shape with hints that still sum to n L while two records of the second
    workgroup are 64 bytes shorter / longer: the launch is the streaming kernel's all the same (the
    counter says Stream), and that workgroup must notice and run per lane inside the kernel --
    every byte as the oracle's."""
    d = case_data(P, 6, 0, lying=True)
    assert int(d.offs[-1]) == d.n * d.L and max(d.lens) == d.L + 64
    want = expected_route(1, P, 6, 0, d.n)
    assert want[0] == "Stream" and want[1] == d.full * (512 // P)
    run_case(enet, d, 1, want)
    enet.set_staging(-1)


def test_line_staged_records_of_256_lines(enet):
    """Line staging (one lane, L % 64 != 0, L % 4 == 0) is routed for every L < 2^24; a record of
    L >= 32 641 bytes spans 256 or more aligned 128-byte lines whatever its phase.  One full
    256-record workgroup of 32 644-byte records plus 3: every byte as the oracle's.  (The kernel kept
    a record's line count in 8 bits and left the first and last line of such records unwritten.)"""
    L, n = 32644, 259
    d = make_case(1, (L + 63) // 64, L, (L,) * n, 900001)
    run_case(enet, d, 1, ("LineStaged", 256, 3), victims={1: 0, 130: L // 2, 254: L - 1})
    enet.set_staging(-1)
