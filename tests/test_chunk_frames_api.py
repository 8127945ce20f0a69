"""CPU tests of the chunk transfer frames' boundary: the test helper's 42-byte Chunk header against
the compiled reference's golden frames, and the argument checks of enet_chunk_frame_*_batch, which
hold whatever the device state (no GPU is touched)."""
import ctypes as C

import pytest

import oracle
from chunk_frame_ref import chunk_header, chunk_message, wire_frame


def test_header_helper_matches_golden_chunk_frames(golden):
    """tests/golden/golden.json["frames"] holds four "chunk" vectors of the compiled reference
    (data lengths 0, 1, 1400, 4096; ttl 3600; version 4): signed = header || data || HMAC, body =
    the session frame body.  The helper's header and the oracle's frame body reproduce them."""
    chunks = [f for f in golden["frames"] if f["kind"] == "chunk"]
    assert len(chunks) == 4
    seen = []
    for f in chunks:
        signed, key, nonce = bytes.fromhex(f["signed"]), bytes.fromhex(f["key"]), bytes.fromhex(f["nonce"])
        m = signed[:-32]
        L = len(m) - 42
        seen.append(L)
        chunk_id, data = m[10:42], m[42:]
        assert signed[:42 + L] == chunk_header(4, 3600, chunk_id, L) + data
        assert m == chunk_message(4, 3600, chunk_id, data)
        assert oracle.frame_seal(key, nonce, m).hex() == f["body"]
        assert wire_frame(key, nonce, m)[16:].hex() == f["body"]
    assert sorted(seen) == [0, 1, 1400, 4096]


@pytest.fixture(scope="module")
def L():
    from ephemeralnet_amd import build as B
    B.build(verbose=False)
    import ephemeralnet_amd as E
    return E.lib()


def test_invalid_arguments_rejected_without_gpu(L):
    import ephemeralnet_amd as E
    buf = (C.c_uint8 * 256)()
    r = E._Records()
    r.count = 3
    r.in_offsets = r.out_offsets = r.in_ = r.out = r.keys = C.addressof(buf)
    r.key_stride = 32
    p = C.addressof(buf)
    good = [None, 0, None, p, p, p, p, None, None, p, None]  # session, sessions, mid, ids, keys, nonces, hashes, data_out, ttl_out, status, stream
    assert L.enet_chunk_frame_open_batch(None, *good) == -1
    assert b"NULL" in L.enet_last_error()
    for hole in (3, 4, 5, 6, 9):  # chunk_ids, chunk_keys, chunk_nonces, chunk_hashes, status
        args = list(good)
        args[hole] = None
        assert L.enet_chunk_frame_open_batch(C.byref(r), *args) == -1, hole
        assert b"chunk_frame_open" in L.enet_last_error()
        r0 = E._Records()  # ... also for an empty batch
        assert L.enet_chunk_frame_open_batch(C.byref(r0), *args) == -1, hole
    # a session list without its midstates
    args = list(good)
    args[0], args[1] = p, 4
    assert L.enet_chunk_frame_open_batch(C.byref(r), *args) == -1
    # seal: NULL descriptor, NULL arenas, NULL chunk_ids / ttl
    assert L.enet_chunk_frame_seal_batch(None, None, 0, None, p, p, None, None) == -1
    r.nonces = C.addressof(buf)
    assert L.enet_chunk_frame_seal_batch(C.byref(r), None, 0, None, None, p, None, None) == -1
    assert L.enet_chunk_frame_seal_batch(C.byref(r), None, 0, None, p, None, None, None) == -1
    assert L.enet_chunk_frame_seal_batch(C.byref(r), p, 0, p, p, p, None, None) == -1  # no sessions
    bad = E._Records()
    bad.count = 3
    assert L.enet_chunk_frame_seal_batch(C.byref(bad), None, 0, None, p, p, None, None) == -1
    # empty batches are no-ops
    r0 = E._Records()
    assert L.enet_chunk_frame_seal_batch(C.byref(r0), None, 0, None, None, None, None, None) == 0
    assert L.enet_chunk_frame_open_batch(C.byref(r0), *good) == 0
    assert L.enet_abi_version() == (1 << 16) | 4
