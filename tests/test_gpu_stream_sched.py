"""The streaming kernel's stage hand-off and the Poly1305 accumulator carried across stages.

tests/test_gpu_uniform_matrix.py walks every kernel and lane count; this file stays on the streaming
kernel (csrc/stream.hip) and on what a change to how its waves are scheduled, or to where the
Poly1305 of a stage is issued, can break: a stage read before it landed or stored before it was
written, and the accumulator h of open and seal carried from one stage's blocks into the next.
Everything is compared with the CPU oracle byte for byte: ciphertext, tags, verdicts, opened
plaintext.

Shapes: P lanes per record in {1, 2, 4, 8, 16}; n = 512 / P records (one workgroup) and 1 024 / P
(two); L = 128 P (one stage), 256 P (two) and 384 P (three, an odd count); a key and a nonce per
record.  AAD of 0, 1, 16 and 17 bytes on the two-stage shape.  Tamper: one bit of the first, a
middle and the last record of a workgroup, in turn in the ciphertext's first stage, its last stage,
the tag and the AAD.  Determinism: the C2 shape's one-workgroup slice (256 x 4 KiB, two lanes)
sealed and opened twice on one stream and twice on two streams."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import oracle
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

LANES = [1, 2, 4, 8, 16]
STAGES = [1, 2, 3]
WGS = [1, 2]
AADS = [0, 1, 16, 17]


@pytest.fixture(scope="module")
def enet():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ephemeralnet_amd as E
    E.lib()
    E.set_seg_min(-1)
    E.set_staging(-1)
    yield E
    E.set_lanes_per_record(0)


@functools.lru_cache(maxsize=None)
def case(P, stages, wgs, alen, L=None):
    """Inputs and the oracle's outputs of one shape, computed once."""
    L = L or 128 * P * stages
    n = wgs * 512 // P
    seed = 7100000 + 10000 * P + 1000 * stages + 100 * wgs + alen + (L if L != 128 * P * stages else 0)
    pt = splitmix_bytes(seed, n * L)
    keys = splitmix_bytes(seed + 1, 32 * n)
    nonces = splitmix_bytes(seed + 2, 12 * n)
    aad = splitmix_bytes(seed + 3, alen * n)
    ct, tags = [], []
    for i in range(n):
        c, t = oracle.aead_seal(keys[32 * i:32 * i + 32], nonces[12 * i:12 * i + 12], pt[L * i:L * i + L],
                                aad[alen * i:alen * i + alen])
        ct.append(c)
        tags.append(t)
    u8 = lambda b: np.frombuffer(b, dtype=np.uint8)
    return SimpleNamespace(P=P, L=L, n=n, alen=alen, pt=u8(pt), keys=u8(keys), nonces=u8(nonces), aad=u8(aad),
                           ct=u8(b"".join(ct)), tags=u8(b"".join(tags)),
                           offs=np.arange(n + 1, dtype=np.int64) * L, aoff=np.arange(n + 1, dtype=np.int64) * alen)


class Dev:
    """One case's inputs on the device."""

    def __init__(self, enet, d):
        import torch
        up = lambda a: torch.from_numpy(np.array(a)).cuda()
        self.enet, self.d = enet, d
        self.offs, self.keys, self.nonces = up(d.offs), up(d.keys), up(d.nonces)
        # (a zero-length AAD arena still gets a valid pointer)
        self.aad = up(d.aad) if d.alen else torch.zeros(16, dtype=torch.uint8, device="cuda")
        self.aoff = up(d.aoff)
        self.pt, self.ct, self.tags = up(d.pt), up(d.ct), up(d.tags)

    def batch(self, arena):
        d = self.d
        return self.enet.Batch(arena, self.offs, self.keys, self.nonces, total_bytes_hint=d.n * d.L, max_len_hint=d.L)

    def streamed(self, fn, *a, **kw):
        """Run one call; every record must have gone to the streaming kernel."""
        before = self.enet.record_route_counts()
        fn(*a, **kw)
        after = self.enet.record_route_counts()
        delta = {k: after[k] - before[k] for k in after}
        assert delta["Stream"] == self.d.n and sum(delta.values()) == self.d.n, delta

    def seal(self, src=None, aad=None, stream=None):
        import torch
        out = torch.full_like(self.pt, 0xA5)
        tags = torch.zeros(16 * self.d.n, dtype=torch.uint8, device="cuda")
        self.streamed(self.enet.aead_seal, self.batch(self.pt if src is None else src), out, tags,
                      self.aad if aad is None else aad, self.aoff, stream=stream)
        return out, tags

    def open(self, ct=None, tags=None, aad=None, stream=None):
        import torch
        out = torch.full_like(self.pt, 0xA5)
        ok = torch.full((self.d.n,), 7, dtype=torch.uint8, device="cuda")
        self.streamed(self.enet.aead_open, self.batch(self.ct if ct is None else ct), out,
                      self.tags if tags is None else tags, ok, self.aad if aad is None else aad, self.aoff,
                      stream=stream)
        return out, ok


def first_bad(got, want, width):
    d = np.flatnonzero(got != want)
    return None if d.size == 0 else int(d[0]) // width


def check_round_trip(enet, d):
    enet.set_lanes_per_record(d.P)
    g = Dev(enet, d)
    tag = (d.P, d.L, d.n, d.alen)
    ct, tags = g.seal()
    cth, th = ct.cpu().numpy(), tags.cpu().numpy()
    assert np.array_equal(cth, d.ct), (tag, "ciphertext, record", first_bad(cth, d.ct, d.L))
    assert np.array_equal(th, d.tags), (tag, "tag, record", first_bad(th, d.tags, 16))
    back, ok = g.open()
    okh, bh = ok.cpu().numpy(), back.cpu().numpy()
    assert okh.tolist() == [1] * d.n, (tag, "verdicts", np.flatnonzero(okh != 1)[:8])
    assert np.array_equal(bh, d.pt), (tag, "opened plaintext, record", first_bad(bh, d.pt, d.L))


@pytest.mark.parametrize("P", LANES)
def test_stages_and_workgroups(enet, P):
    """One, two and three stages in one and in two workgroups, no AAD."""
    for wgs in WGS:
        for stages in STAGES:
            check_round_trip(enet, case(P, stages, wgs, 0))


@pytest.mark.parametrize("P", LANES)
def test_aad_lengths_two_stages(enet, P):
    """The two-stage shape with 0, 1, 16 and 17 bytes of AAD per record (absorbed by lane 0 before
    the first stage; the length block by the last lane after the last)."""
    for alen in AADS:
        check_round_trip(enet, case(P, 2, 2, alen))


@pytest.mark.parametrize("P", LANES)
def test_tamper_one_record(enet, P):
    """Three stages, two workgroups, 17 bytes of AAD.  One flipped bit per open call: in the first,
    a middle and the last record of the second workgroup, in the first stage of the record's last
    lane, the last stage of its first lane, the tag and the AAD.  That record alone fails and comes
    back zeroed; every other record, its neighbours included, is exact."""
    d = case(P, 3, 2, 17)
    enet.set_lanes_per_record(P)
    g = Dev(enet, d)
    per = 512 // P
    run = d.L // P  # bytes per lane, three stages of 128
    spots = {"first stage": (P - 1) * run + 5, "last stage": 2 * 128 + 7}
    for v in (per, per + per // 2, 2 * per - 1):
        for where in ("first stage", "last stage", "tag", "aad"):
            ct, tags, aad = g.ct, g.tags, g.aad
            if where == "tag":
                tags = g.tags.clone()
                tags[16 * v + 9] ^= 0x20
            elif where == "aad":
                aad = g.aad.clone()
                aad[d.alen * v + 16] ^= 0x01
            else:
                ct = g.ct.clone()
                ct[d.L * v + spots[where]] ^= 0x80
            back, ok = g.open(ct, tags, aad)
            okh, bh = ok.cpu().numpy(), back.cpu().numpy()
            tag = (P, v, where)
            assert np.flatnonzero(okh != 1).tolist() == [v] and okh[v] == 0, (tag, np.flatnonzero(okh != 1)[:8])
            want = d.pt.copy()
            want[d.L * v:d.L * (v + 1)] = 0
            assert np.array_equal(bh, want), (tag, "opened plaintext, record", first_bad(bh, want, d.L))


def test_c2_slice_deterministic(enet):
    """256 records x 4 KiB on two lanes (one workgroup of the C2 shape, 16 stages): two seals and
    two opens back to back on one stream, then two of each on two streams at once; all four
    results identical, and the oracle's."""
    import torch
    d = case(2, 16, 1, 0, L=4096)
    assert d.n == 256 and d.L == 4096
    enet.set_lanes_per_record(2)
    g = Dev(enet, d)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    sealed = [g.seal(), g.seal()]
    opened = [g.open(), g.open()]
    for s in (s1, s2):
        with torch.cuda.stream(s):
            sealed.append(g.seal(stream=s))
    for s in (s1, s2):
        with torch.cuda.stream(s):
            opened.append(g.open(stream=s))
    torch.cuda.synchronize()
    for i, (ct, tags) in enumerate(sealed):
        cth, th = ct.cpu().numpy(), tags.cpu().numpy()
        assert np.array_equal(cth, d.ct), ("seal", i, "ciphertext, record", first_bad(cth, d.ct, d.L))
        assert np.array_equal(th, d.tags), ("seal", i, "tag, record", first_bad(th, d.tags, 16))
    for i, (back, ok) in enumerate(opened):
        okh, bh = ok.cpu().numpy(), back.cpu().numpy()
        assert okh.tolist() == [1] * d.n, ("open", i, np.flatnonzero(okh != 1)[:8])
        assert np.array_equal(bh, d.pt), ("open", i, "plaintext, record", first_bad(bh, d.pt, d.L))
