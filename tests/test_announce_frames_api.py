"""CPU tests of the announce frames' boundary: the test helper (tests/announce_frame_ref.py) in
both directions against the compiled reference's golden vectors (tests/golden/announce_frames.json:
encode_signed outputs, decode_signed verdicts and fields, frame bodies, PoW digests), and the
argument checks of enet_announce_frame_*_batch, which hold whatever the device state (no GPU is
touched)."""
import ctypes as C
import json
import os

import pytest

import oracle
from announce_frame_ref import (HEADER, NO_MANIFEST, OK, POW, SENDER, FRAME, Announce, admit, announce_message,
                                clamp_version, message_len, parse_announce, wire_frame)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unhx(s: str) -> bytes:
    return b"" if s == "-" else bytes.fromhex(s)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "announce_frames.json")) as f:
        return json.load(f)


def case_announce(c) -> Announce:
    return Announce(chunk_id=bytes.fromhex(c["chunk_id"]), peer_id=bytes.fromhex(c["peer_id"]), endpoint=unhx(c["endpoint"]),
                    uri=unhx(c["uri"]), shards=unhx(c["shards"]), ttl=c["ttl"], version=c["version_in"],
                    work_nonce=c["work_nonce"])


def check_decoded(m: bytes, d: dict, name: str):
    """The helper's parse against the reference's decode_signed verdict and fields."""
    got = parse_announce(m)
    as_announce = d["decodes"] and d.get("type") == 1
    assert (got is not None) == as_announce, name
    if got is None:
        return None
    a, trailing = got
    assert (a.version, a.ttl, a.chunk_id.hex(), a.peer_id.hex(), a.endpoint, a.uri, a.shards, a.work_nonce) == (
        d["version"], d["ttl"], d["chunk_id"], d["peer_id"], unhx(d["endpoint"]), unhx(d["uri"]), unhx(d["shards"]),
        d["work_nonce"]), name
    return a, trailing


def test_helper_encodes_what_the_reference_encodes(gold):
    """encode_signed for versions 0..5 as given (clamped to 1..4; the nonce only for version 4), E / U
    / A including 0 and the default manifest's URI: the helper's message and the oracle's HMAC."""
    assert sorted({c["version_in"] for c in gold["cases"]}) == [0, 1, 2, 3, 4, 5]
    shapes = {(len(unhx(c["endpoint"])), len(unhx(c["uri"])), len(unhx(c["shards"]))) for c in gold["cases"]}
    assert {(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)} <= shapes
    assert any(unhx(c["uri"]).decode(errors="replace") == gold["manifest"]["uri"] for c in gold["cases"])
    for c in gold["cases"]:
        a, key = case_announce(c), bytes.fromhex(c["key"])
        m = announce_message(a)
        assert len(m) == message_len(a), c["name"]
        assert m[0] == clamp_version(c["version_in"]) and m[1] == 1
        assert (m + oracle.hmac_sha256(key, m)).hex() == c["signed"], c["name"]


def test_helper_decodes_what_the_reference_decodes(gold):
    """Every decode_signed verdict of the file: the encoded cases (a v3 announce made by encode
    does NOT decode: encode leaves the nonce out, decode expects it) and the mutations (v3 with a
    hand-appended nonce decodes; trailing bytes decode; a cut at every length check does not; a wrong
    type byte is no Announce; versions 0 / 5 / 255 do not decode)."""
    for c in gold["cases"]:
        signed, key = bytes.fromhex(c["signed"]), bytes.fromhex(c["key"])
        assert oracle.hmac_sha256_verify(key, signed[:-32], signed[-32:])
        got = check_decoded(signed[:-32], c["decoded"], c["name"])
        v = clamp_version(c["version_in"])
        assert (got is not None) == (v != 3), c["name"]
        if got:
            a, trailing = got
            assert trailing == 0 and a.work_nonce == (c["work_nonce"] if v == 4 else 0)
    seen = {}
    for mu in gold["mutations"]:
        signed, key = bytes.fromhex(mu["signed"]), bytes.fromhex(mu["key"])
        d = mu["decoded"]
        mac_ok = len(signed) >= 32 and oracle.hmac_sha256_verify(key, signed[:-32], signed[-32:])
        if not mac_ok:
            assert not d["decodes"], mu["name"]
            seen[mu["name"]] = None
            continue
        seen[mu["name"]] = check_decoded(signed[:-32], d, mu["name"])
    assert seen["v3 with a hand-appended nonce"][0].work_nonce == 0x0102030405060708
    assert seen["v4 with a trailing byte"][1] == 1 and seen["v4 with eight trailing bytes"][1] == 8
    assert seen["v1 with a trailing byte"][1] == 1
    assert seen["empty v4 cut to 90"][1] == 0  # 90 bytes is the whole of an announce without fields
    for name, got in seen.items():
        if name == "empty v4 cut to 90":
            continue
        if "cut to" in name or name.startswith("version byte") or "type" in name or name in (
                "E one too large", "31 bytes in all", "a flipped MAC bit"):
            assert got is None, name
    assert seen["U one too small"][1] == 1  # the nonce moves one byte down, one byte is left over


def test_frames_and_pow_digests(gold):
    """Frame bodies under fixed nonces (the reference's ChaCha20::apply over encode_signed) are the
    oracle's frame_seal of the helper's message; the PoW digests (Node.cpp:155-173 through the
    reference's Sha256) are the oracle's over the helper's prefix."""
    by = {c["name"]: c for c in gold["cases"]}
    for f in gold["frames"]:
        key, nonce, signed = bytes.fromhex(f["key"]), bytes.fromhex(f["nonce"]), bytes.fromhex(f["signed"])
        m = announce_message(case_announce(by[f["case"]]))
        assert m == signed[:-32]
        assert oracle.frame_seal(key, nonce, m).hex() == f["body"]
        assert wire_frame(key, nonce, m)[16:].hex() == f["body"]
        assert wire_frame(key, nonce, m)[:16] == nonce + (len(m) + 32).to_bytes(4, "big")
    assert len(gold["announce_pow"]) >= 8
    for p in gold["announce_pow"]:
        a = case_announce(by[p["case"]])
        d = oracle.pow_digest(a.prefix(), p["nonce"])
        assert d.hex() == p["digest"], p["case"]
        assert oracle.leading_zero_bits(d) == p["leading_zero_bits"]
        assert len(a.prefix()) == 112 + a.flen


def test_admission_order_of_the_helper(gold):
    """admit() on the golden frames: OK with the parsed fields, and each later check on its own."""
    by = {c["name"]: c for c in gold["cases"]}
    f = next(f for f in gold["frames"] if f["case"] == "encode v4 E14 U37 A3")
    c = by[f["case"]]
    key, nonce = bytes.fromhex(f["key"]), bytes.fromhex(f["nonce"])
    frame = nonce + (len(f["body"]) // 2).to_bytes(4, "big") + bytes.fromhex(f["body"])
    peer = bytes.fromhex(c["peer_id"])
    st, m, info = admit(frame, key, peer, 0)
    assert st == OK and m.hex() == c["signed"][:-64]
    assert info == [4, c["ttl"], 14, 37, 3, c["work_nonce"] & 0xFFFFFFFF, c["work_nonce"] >> 32, 0]
    assert admit(frame[:-1], key, peer, 0)[0] == FRAME
    assert admit(frame, key, bytes(32), 0)[0] == SENDER
    assert admit(frame, key, peer, 40)[0] == POW
    a = case_announce(by["encode v4 E1 U0 A0"])
    k2 = bytes.fromhex(by["encode v4 E1 U0 A0"]["key"])
    assert admit(wire_frame(k2, nonce, announce_message(a)), k2, a.peer_id, 0)[0] == NO_MANIFEST
    v3 = next(f for f in gold["frames"] if f["case"].startswith("encode v3"))
    fr3 = bytes.fromhex(v3["nonce"]) + (len(v3["body"]) // 2).to_bytes(4, "big") + bytes.fromhex(v3["body"])
    assert admit(fr3, bytes.fromhex(v3["key"]), bytes.fromhex(by[v3["case"]]["peer_id"]), 0)[0] == HEADER


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
    f = E._AnnounceFields()
    f.manifests = f.endpoints = 3
    for name in ("chunk_ids", "uris", "uri_offsets", "endpoint_bytes", "endpoint_offsets", "shards", "shard_offsets",
                 "peer_id", "ttl"):
        setattr(f, name, p)
    seal, opn = L.enet_announce_frame_seal_batch, L.enet_announce_frame_open_batch
    # seal(r, session, sessions, mid, f, difficulty, max_attempts, work_nonce, status, stream)
    assert seal(None, None, 0, None, C.byref(f), 6, 10, p, p, None) == -1
    assert seal(C.byref(r), None, 0, None, None, 6, 10, p, p, None) == -1
    assert b"announce_frame_seal" in L.enet_last_error()
    assert seal(C.byref(r), None, 0, None, C.byref(f), 6, 10, None, p, None) == -1
    assert seal(C.byref(r), None, 0, None, C.byref(f), 6, 10, p, None, None) == -1
    assert seal(C.byref(r), None, 0, None, C.byref(f), 256, 10, p, p, None) == -1
    assert b"difficulty" in L.enet_last_error()
    assert seal(C.byref(r), None, 0, None, C.byref(f), 6, 10, p + 4, p, None) == -1
    assert b"misaligned" in L.enet_last_error()
    assert seal(C.byref(r), p, 0, p, C.byref(f), 6, 10, p, p, None) == -1   # a session list, no sessions
    assert seal(C.byref(r), p, 4, None, C.byref(f), 6, 10, p, p, None) == -1  # ... without its midstates
    for name in ("chunk_ids", "uris", "uri_offsets", "endpoint_bytes", "endpoint_offsets", "shards", "shard_offsets",
                 "peer_id", "ttl"):
        setattr(f, name, None)
        assert seal(C.byref(r), None, 0, None, C.byref(f), 6, 10, p, p, None) == -1, name
        assert b"announce_frame_seal" in L.enet_last_error()
        setattr(f, name, p)
    f.ttl = p + 2
    assert seal(C.byref(r), None, 0, None, C.byref(f), 6, 10, p, p, None) == -1
    f.ttl = p
    for hole in ("out", "out_offsets", "keys", "nonces"):
        keep = getattr(r, hole)
        setattr(r, hole, None)
        assert seal(C.byref(r), None, 0, None, C.byref(f), 6, 10, p, p, None) == -1, hole
        setattr(r, hole, keep)
    # open(r, session, sessions, mid, peer_ids, difficulty, info, status, stream)
    r.in_offsets = r.in_ = p
    assert opn(None, None, 0, None, p, 6, p, p, None) == -1
    assert opn(C.byref(r), None, 0, None, None, 6, p, p, None) == -1
    assert b"announce_frame_open" in L.enet_last_error()
    assert opn(C.byref(r), None, 0, None, p, 6, None, p, None) == -1
    assert opn(C.byref(r), None, 0, None, p, 6, p, None, None) == -1
    assert opn(C.byref(r), None, 0, None, p, 256, p, p, None) == -1
    assert opn(C.byref(r), None, 0, None, p, 6, p + 2, p, None) == -1
    assert b"misaligned" in L.enet_last_error()
    assert opn(C.byref(r), p, 0, p, p, 6, p, p, None) == -1
    r.in_ = None
    assert opn(C.byref(r), None, 0, None, p, 6, p, p, None) == -1
    # empty batches are no-ops
    r0 = E._Records()
    assert seal(C.byref(r0), None, 0, None, None, 6, 10, None, None, None) == 0
    assert opn(C.byref(r0), None, 0, None, None, 6, None, None, None) == 0
    assert L.enet_abi_version() == (1 << 16) | 4
