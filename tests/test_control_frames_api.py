"""CPU tests of the Request / Acknowledge frames' boundary: the test helper
(tests/control_frame_ref.py) in both directions against the compiled reference's golden vectors
(tests/golden/control_frames.json: encode_signed outputs, decode_signed verdicts and fields, frame
bodies), and the argument checks of enet_control_frame_*_batch / enet_frame_classify_batch, which
hold whatever the device state (no GPU is touched)."""
import ctypes as C
import json
import os

import pytest

import oracle
from control_frame_ref import (ACK, ACK_LEN, FK_ACK, FK_BAD, FK_OTHER, FK_REQUEST, FRAME, HEADER, OK, REQ_LEN, REQUEST,
                               clamp_version, classify, control_message, open_expect, parse_control, seal_expect,
                               wire_of)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "control_frames.json")) as f:
        return json.load(f)


def check_decoded(m: bytes, d: dict, name: str):
    """The helper's parse against the reference's decode_signed verdict and fields."""
    got = parse_control(m)
    as_control = d["decodes"] and d.get("type") in (REQUEST, ACK)
    assert (got is not None) == as_control, name
    if got is None:
        return None
    (v, t, acc, cid, pid), trailing = got
    assert (v, t, acc, cid.hex(), pid.hex()) == (d["version"], d["type"], d["accepted"], d["chunk_id"], d["peer_id"]), name
    return got


def test_helper_encodes_what_the_reference_encodes(gold):
    """encode_signed of Request and Acknowledge for versions 0..5 as given (clamped to 1..4) and both
    accepted values: the helper's message and the oracle's HMAC."""
    assert sorted({c["version_in"] for c in gold["cases"]}) == [0, 1, 2, 3, 4, 5]
    assert {(c["kind"], c["accepted"]) for c in gold["cases"]} == {(REQUEST, 0), (ACK, 0), (ACK, 1)}
    for c in gold["cases"]:
        key, cid, pid = (bytes.fromhex(c[k]) for k in ("key", "chunk_id", "peer_id"))
        m = control_message(c["kind"], cid, pid, bool(c["accepted"]), c["version_in"])
        assert len(m) == (REQ_LEN if c["kind"] == REQUEST else ACK_LEN), c["name"]
        assert m[0] == clamp_version(c["version_in"]) and m[1] == c["kind"]
        assert (m + oracle.hmac_sha256(key, m)).hex() == c["signed"], c["name"]
        got = check_decoded(m, c["decoded"], c["name"])
        assert got is not None and got[1] == 0


def test_helper_decodes_what_the_reference_decodes(gold):
    """decode_signed's verdict on bytes encode cannot make: other types, version bytes 0 and 5, one
    byte short, one byte long (the reference ACCEPTS the trailing byte; the fused open reports HEADER),
    an accepted byte of 2 (read as != 0), a flipped MAC bit."""
    names = " | ".join(m["name"] for m in gold["mutations"])
    for want in ("type 0x00", "type 0x05", "type 0x06", "type 0xff", "version byte 0", "version byte 5", "one byte short",
                 "one byte long", "accepted byte 2", "flipped MAC bit"):
        assert want in names
    nonce = bytes(range(12))
    for mu in gold["mutations"]:
        key, signed, d = bytes.fromhex(mu["key"]), bytes.fromhex(mu["signed"]), mu["decoded"]
        m, mac = signed[:-32], signed[-32:]
        frame = wire_of(nonce, oracle.chacha20_xor(key, nonce, signed))
        status = open_expect(frame, key)[0]
        if not oracle.hmac_sha256_verify(key, m, mac):
            assert not d["decodes"] and status == FRAME, mu["name"]
            continue
        got = check_decoded(m, d, mu["name"])
        if "one byte long" in mu["name"] or "type 0x02" in mu["name"]:
            # decode's only length check is remaining < needed (Message.cpp:136, 162)
            assert d["decodes"] and got is not None and got[1] == 1 and status == HEADER, mu["name"]
        elif "accepted byte 2" in mu["name"]:
            assert d["accepted"] == 1 and got[0][2] == 1 and status == OK, mu["name"]
            assert open_expect(frame, key)[3][:3] == bytes([4, ACK, 1])
        else:
            assert got is None and status == HEADER, mu["name"]


def test_helper_frames_are_the_reference_frames(gold):
    """ChaCha20::apply over the signed message from counter 0 is the frame body; the helper opens
    it, classifies it, and expects exactly it from the seal."""
    by = {c["name"]: c for c in gold["cases"]}
    assert {by[f["case"]]["kind"] for f in gold["frames"]} == {REQUEST, ACK}
    for f in gold["frames"]:
        c = by[f["case"]]
        key, nonce, signed = bytes.fromhex(f["key"]), bytes.fromhex(f["nonce"]), bytes.fromhex(f["signed"])
        cid, pid = bytes.fromhex(c["chunk_id"]), bytes.fromhex(c["peer_id"])
        assert oracle.chacha20_xor(key, nonce, signed).hex() == f["body"]
        frame = wire_of(nonce, bytes.fromhex(f["body"]))
        assert len(frame) == (114 if c["kind"] == REQUEST else 115)
        assert seal_expect(c["kind"], key, nonce, cid, pid, bool(c["accepted"]), c["version_in"], len(frame)) == (OK, frame)
        v = clamp_version(c["version_in"])
        assert open_expect(frame, key, pid) == (OK, cid, pid, bytes([v, c["kind"], c["accepted"], 1]))
        assert open_expect(frame, key, cid)[3][3] == 0 and open_expect(frame, key)[3][3] == 0
        assert classify(frame, key) == (FK_REQUEST if c["kind"] == REQUEST else FK_ACK)
        assert classify(frame, None) == FK_BAD and classify(frame[:-1], key) == FK_BAD
        assert classify(frame[:47], key) == FK_BAD
        bad = bytearray(frame)
        bad[-1] ^= 1  # triage authenticates nothing; the open does
        assert classify(bytes(bad), key) == classify(frame, key) and open_expect(bytes(bad), key)[0] == FRAME
        other = bytes(a ^ b for a, b in zip(key, bytes([1]) + bytes(31)))
        assert open_expect(frame, other)[0] == FRAME
        assert seal_expect(c["kind"], key, nonce, cid, pid, False, 4, len(frame) + 1) == (FRAME, bytes(len(frame) + 1))
        assert seal_expect(3, key, nonce, cid, pid, False, 4, len(frame)) == (HEADER, bytes(len(frame)))
    empty = wire_of(bytes(12), bytes(32))
    assert classify(empty, bytes(32)) == FK_OTHER


@pytest.fixture(scope="module")
def L():
    from ephemeralnet_amd import build as B
    B.build(verbose=False)
    import ephemeralnet_amd as E
    return E.lib()


def test_invalid_arguments_rejected_without_gpu(L):
    import ephemeralnet_amd as E
    buf = (C.c_uint64 * 64)()
    p = C.addressof(buf)
    r = E._Records()
    r.count = 3
    r.out_offsets = r.out = r.keys = r.nonces = p
    r.key_stride = 32
    seal, opn, cls = L.enet_control_frame_seal_batch, L.enet_control_frame_open_batch, L.enet_frame_classify_batch
    # seal(r, session, sessions, mid, kinds, chunk_ids, peer_id, accepted, accept_zero, versions, status, stream)
    assert seal(None, None, 0, None, p, p, p, None, 0, None, p, None) == -1
    for hole in range(4):
        a = [p, p, p, p]
        a[hole] = None
        assert seal(C.byref(r), None, 0, None, a[0], a[1], a[2], None, 0, None, a[3], None) == -1, hole
        assert b"control_frame_seal" in L.enet_last_error()
    assert seal(C.byref(r), None, 0, None, p, p + 2, p, None, 0, None, p, None) == -1
    assert b"misaligned" in L.enet_last_error()
    assert seal(C.byref(r), None, 0, None, p, p, p + 1, None, 0, None, p, None) == -1
    assert seal(C.byref(r), p, 0, p, p, p, p, None, 0, None, p, None) == -1   # a session list, no sessions
    assert seal(C.byref(r), p, 4, None, p, p, p, None, 0, None, p, None) == -1  # ... without its midstates
    assert seal(C.byref(r), p + 2, 4, p, p, p, p, None, 0, None, p, None) == -1
    for hole in ("out", "out_offsets", "keys", "nonces"):
        keep = getattr(r, hole)
        setattr(r, hole, None)
        assert seal(C.byref(r), None, 0, None, p, p, p, None, 0, None, p, None) == -1, hole
        setattr(r, hole, keep)
    # open(r, session, sessions, mid, sender_ids, chunk_ids_out, peer_ids_out, info, status, stream)
    ro = E._Records()
    ro.count = 3
    ro.in_offsets = ro.in_ = ro.keys = p  # no out side, no nonces
    ro.key_stride = 32
    assert opn(None, None, 0, None, None, p, None, p, p, None) == -1
    for hole in range(3):
        a = [p, p, p]
        a[hole] = None
        assert opn(C.byref(ro), None, 0, None, None, a[0], None, a[1], a[2], None) == -1, hole
        assert b"control_frame_open" in L.enet_last_error()
    for bad in range(4):
        a = [p, p, p, p]
        a[bad] = p + 2
        assert opn(C.byref(ro), None, 0, None, a[0], a[1], a[2], a[3], p, None) == -1, bad
        assert b"misaligned" in L.enet_last_error()
    assert opn(C.byref(ro), p, 0, p, None, p, None, p, p, None) == -1
    assert opn(C.byref(ro), p, 4, None, None, p, None, p, p, None) == -1
    # classify(r, session, sessions, kind, lists, counts, stream)
    assert cls(None, None, 0, p, p, p, None) == -1
    for hole in range(3):
        a = [p, p, p]
        a[hole] = None
        assert cls(C.byref(ro), None, 0, a[0], a[1], a[2], None) == -1, hole
        assert b"frame_classify" in L.enet_last_error()
    assert cls(C.byref(ro), None, 0, p, p + 2, p, None) == -1
    assert cls(C.byref(ro), None, 0, p, p, p + 2, None) == -1
    assert b"misaligned" in L.enet_last_error()
    assert cls(C.byref(ro), p, 0, p, p, p, None) == -1
    assert cls(C.byref(ro), p + 1, 4, p, p, p, None) == -1
    for hole in ("in_", "in_offsets", "keys"):
        keep = getattr(ro, hole)
        setattr(ro, hole, None)
        assert opn(C.byref(ro), None, 0, None, None, p, None, p, p, None) == -1, hole
        assert cls(C.byref(ro), None, 0, p, p, p, None) == -1, hole
        setattr(ro, hole, keep)
    # empty batches are no-ops
    r0 = E._Records()
    assert seal(C.byref(r0), None, 0, None, None, None, None, None, 0, None, None, None) == 0
    assert opn(C.byref(r0), None, 0, None, None, None, None, None, None, None) == 0
    assert cls(C.byref(r0), None, 0, None, None, None, None) == 0
    assert L.enet_abi_version() == (1 << 16) | 4
