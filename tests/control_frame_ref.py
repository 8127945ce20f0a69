"""Test helper for the Request / Acknowledge frames and the frame triage: the two messages as
protocol::encode writes them and protocol::decode reads them (src/protocol/Message.cpp:236-252,
134-143, 160-170), the frames the oracle module makes of them (encode_signed, Message.cpp:305-311;
SessionManager::send, SessionManager.cpp:362-387), the OK / FRAME / HEADER verdict of
enet_control_frame_open_batch and enet_frame_classify_batch's kinds.  Pinned against the compiled
reference's golden vectors (tests/golden/control_frames.json) by tests/test_control_frames_api.py."""
from __future__ import annotations

import oracle

REQUEST, ACK = 2, 4
REQ_LEN, ACK_LEN = 66, 67
OVERHEAD = 16 + 32  # wire header, MAC
OK, FRAME, HEADER = 0, 1, 2
FK_BAD, FK_ANNOUNCE, FK_REQUEST, FK_CHUNK, FK_ACK, FK_OTHER = 0, 1, 2, 3, 4, 5


def clamp_version(v: int) -> int:
    """clamp_version (Message.cpp:17-25)."""
    return min(max(v, 1), 4)


def control_message(kind: int, chunk_id: bytes, peer_id: bytes, accepted: bool = False, version: int = 4,
                    raw_version: bool = False) -> bytes:
    """encode (Message.cpp:236-252): the version clamped (raw_version: as given, for frames encode
    cannot make)."""
    assert kind in (REQUEST, ACK) and len(chunk_id) == 32 and len(peer_id) == 32
    v = version if raw_version else clamp_version(version)
    head = bytes([v, kind]) + (bytes([1 if accepted else 0]) if kind == ACK else b"")
    return head + chunk_id + peer_id


def parse_control(m: bytes):
    """decode (Message.cpp:268-303) for a Request or Acknowledge: None when it does not decode as
    one, else ((version, type, accepted, chunk_id, peer_id), bytes after the payload)."""
    if len(m) < 2 or not 1 <= m[0] <= 4 or m[1] not in (REQUEST, ACK):
        return None
    v, t, rest = m[0], m[1], m[2:]
    if t == REQUEST:
        if len(rest) < 64:
            return None
        return (v, t, 0, rest[:32], rest[32:64]), len(rest) - 64
    if len(rest) < 65:
        return None
    return (v, t, 1 if rest[0] != 0 else 0, rest[1:33], rest[33:65]), len(rest) - 65


def wire_of(nonce: bytes, body: bytes) -> bytes:
    """nonce(12) || BE32(|body|) || body (SessionManager.cpp:376-387)."""
    return nonce + len(body).to_bytes(4, "big") + body


def wire_frame(key: bytes, nonce: bytes, message: bytes) -> bytes:
    return wire_of(nonce, oracle.frame_seal(key, nonce, message))


def control_frame(key: bytes, nonce: bytes, kind: int, chunk_id: bytes, peer_id: bytes, accepted: bool = False,
                  version: int = 4) -> bytes:
    return wire_frame(key, nonce, control_message(kind, chunk_id, peer_id, accepted, version))


def seal_expect(kind: int, key, nonce: bytes, chunk_id: bytes, peer_id: bytes, accepted: bool, version: int,
                out_len: int):
    """What enet_control_frame_seal_batch owes for one record -> (status, the slot's bytes).  key
    None: the session index lies outside the table."""
    if kind not in (REQUEST, ACK):
        return HEADER, bytes(out_len)
    if key is None or out_len != (REQ_LEN if kind == REQUEST else ACK_LEN) + OVERHEAD:
        return FRAME, bytes(out_len)
    return OK, control_frame(key, nonce, kind, chunk_id, peer_id, accepted, version)


def open_message(frame: bytes, key):
    """The general open (enet_wire_open_batch) -> the message, or None for ok = 0."""
    if key is None or len(frame) < OVERHEAD or int.from_bytes(frame[12:16], "big") != len(frame) - 16:
        return None
    ok, m = oracle.frame_open(key, frame[:12], frame[16:])
    return m if ok else None


def open_expect(frame: bytes, key, sender=None):
    """What enet_control_frame_open_batch owes for one frame -> (status, chunk_id, peer_id, info).
    Bytes after the payload are HEADER (the call's one documented difference from decode)."""
    none = (bytes(32), bytes(32), bytes(4))
    m = open_message(frame, key)
    if m is None:
        return (FRAME,) + none
    parsed = parse_control(m)
    if parsed is None or parsed[1] != 0:
        return (HEADER,) + none
    v, t, acc, cid, pid = parsed[0]
    return OK, cid, pid, bytes([v, t, acc, 1 if sender is not None and sender == pid else 0])


def classify(frame: bytes, key) -> int:
    """enet_frame_classify_batch's kind for one frame: the first keystream block only, nothing
    authenticated."""
    if key is None or len(frame) < OVERHEAD or int.from_bytes(frame[12:16], "big") != len(frame) - 16:
        return FK_BAD
    lm = len(frame) - OVERHEAD
    if lm < 2:
        return FK_OTHER
    head = oracle.chacha20_xor(key, frame[:12], frame[16:18])
    v, t = head[0], head[1]
    if not 1 <= v <= 4:
        return FK_OTHER
    fits = {1: lm >= 82 + (8 if v >= 3 else 0), REQUEST: lm == REQ_LEN, 3: lm >= 42, ACK: lm == ACK_LEN}
    return t if fits.get(t, False) else FK_OTHER
