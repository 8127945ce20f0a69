"""The streaming kernel's lane map and what the lanes of a record hand each other.

Lane j of every record of a workgroup sits in wave group j (csrc/stream_map.hpp), and one lane per
record, its leader, makes the Poly1305 key and the tag: the leader's r goes to the record's other
lanes, their scaled limbs come back to it, and open's verdict goes out again for the tamper
zeroing, all through LDS under the record's index in the workgroup.  A value exchanged under the
wrong index, or a run moved for the wrong owner, gives another record's bytes, tag or verdict; every
record here has its own key and nonce, and everything is compared with the CPU oracle byte for
byte, after the routing counter has said Stream.

Shapes: P lanes per record in {2, 4, 8, 16}; n = 512 / P records (one workgroup) and 1 024 / P
(two); L = 128 P (one stage) and 256 P (two); AAD of 0 and 17 bytes.  Tamper (P = 2, 4): one
ciphertext bit inside the range of each record-lane in turn, in the first and in the last record of
the second workgroup.  One key for the whole batch, reference-mode ChaCha20 with start counters at
the u32 wrap, and hints that lie (one workgroup falls back to the per-lane path inside the kernel)
run through the uniform matrix's checker on the same two lengths."""
import numpy as np
import pytest

from test_gpu_stream_sched import Dev, case, check_round_trip, first_bad
from test_gpu_uniform_matrix import make_case, run_case

pytestmark = pytest.mark.gpu

LANES = [2, 4, 8, 16]


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
    E.set_staging(-1)


@pytest.mark.parametrize("P", LANES)
def test_round_trip_per_record_keys(enet, P):
    """One and two workgroups, one and two stages, no AAD and 17 bytes of it: ciphertext, tags,
    verdicts and opened plaintext of every record."""
    for wgs in (1, 2):
        for stages in (1, 2):
            for alen in (0, 17):
                check_round_trip(enet, case(P, stages, wgs, alen))


@pytest.mark.parametrize("P", [2, 4])
def test_tamper_each_record_lane(enet, P):
    """Two stages, two workgroups, 17 bytes of AAD.  One flipped ciphertext bit per open call, inside
    the bytes of record-lane j = 0 .. P-1 in turn (first stage for even j, second for odd), in the
    first and in the last record of the second workgroup.  That record alone fails, its whole
    length comes back zeroed, and every other record, its neighbours included, is exact."""
    d = case(P, 2, 2, 17)
    enet.set_lanes_per_record(P)
    g = Dev(enet, d)
    per = 512 // P
    run = d.L // P  # bytes per record-lane: two stages of 128
    assert run == 256
    for v in (per, 2 * per - 1):
        for j in range(P):
            ct = g.ct.clone()
            ct[d.L * v + j * run + 128 * (j & 1) + 3 + j] ^= 0x10
            back, ok = g.open(ct)
            okh, bh = ok.cpu().numpy(), back.cpu().numpy()
            tag = (P, v, j)
            assert np.flatnonzero(okh != 1).tolist() == [v] and okh[v] == 0, (tag, np.flatnonzero(okh != 1)[:8])
            want = d.pt.copy()
            want[d.L * v:d.L * (v + 1)] = 0
            assert np.array_equal(bh, want), (tag, "opened plaintext, record", first_bad(bh, want, d.L))


def matrix_case(P, B, shared_key=False, lying=False):
    """Three workgroups and 3 records more, L = 64 P B, under the uniform matrix's checker (seal,
    in-place seal, open, tampered open, ChaCha20 with start counters (2^32 - i mod (P B + 1)): the
    u32 wrap falls before every block of a record and after the last)."""
    per = 512 // P
    L = 64 * P * B
    lens = [L] * (3 * per + 3)
    if lying:  # two records of the second workgroup; the lengths still sum to n L
        lens[per + 3] -= 64
        lens[per + 10] += 64
    seed = 7300000 + 10000 * P + 100 * B + (7 if shared_key else 0) + (13 if lying else 0)
    d = make_case(P, B, L, tuple(lens), seed, shared_key)
    return d, ("Stream", 3 * per, 3)


@pytest.mark.parametrize("P", LANES)
def test_shared_key_and_wrapping_counters(enet, P):
    """One key for the whole batch (key_stride 0), one and two stages; the run includes
    reference-mode ChaCha20 with per-record start counters around the u32 wrap."""
    for B in (2, 4):
        d, want = matrix_case(P, B, shared_key=True)
        assert d.key_stride == 0
        run_case(enet, d, 1, want)
    enet.set_staging(-1)


@pytest.mark.parametrize("P", LANES)
def test_lying_hints_fall_back(enet, P):
    """Hints that still sum to n L while two records of the second workgroup are 64 bytes shorter /
    longer: the launch is the streaming kernel's (the counter says Stream), that workgroup runs per
    lane inside it under its own lane map, the other two under the streaming one."""
    for B in (2, 4):
        d, want = matrix_case(P, B, lying=True)
        assert int(d.offs[-1]) == d.n * d.L and max(d.lens) == d.L + 64
        run_case(enet, d, 1, want)
    enet.set_staging(-1)
