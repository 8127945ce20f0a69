"""Test helper for the announce frames: the `Announce` message as protocol::encode writes it and
protocol::decode reads it (src/protocol/Message.cpp:215-235, 75-121, 268-303), the frames the
oracle module makes of it, the proof of work through the oracle's prefix / search / check, and the
receiver's admission order (handle_transport_message / handle_announce, src/core/Node.cpp:2332-2357,
verify_announce_pow, :1144-1151).  Pinned against the compiled reference's golden vectors
(tests/golden/announce_frames.json) by tests/test_announce_frames_api.py."""
from __future__ import annotations

import dataclasses

import oracle

FIXED = 82            # version, type, BE32 ttl / E / U / A, chunk_id(32), peer_id(32)
OVERHEAD = 16 + 32    # wire header, MAC
ANNOUNCE = 0x01
OK, FRAME, HEADER, SENDER, NO_MANIFEST, POW = 0, 1, 2, 3, 4, 5
POW_NODE = 0
NODE_POW_ATTEMPTS = 500_000


def clamp_version(v: int) -> int:
    """clamp_version (Message.cpp:17-25)."""
    return min(max(v, 1), 4)


@dataclasses.dataclass
class Announce:
    chunk_id: bytes
    peer_id: bytes
    endpoint: bytes
    uri: bytes
    shards: bytes
    ttl: int = 3600
    version: int = 4
    work_nonce: int = 0

    @property
    def flen(self) -> int:
        return len(self.endpoint) + len(self.uri) + len(self.shards)

    def prefix(self) -> bytes:
        """announce_pow_digest's serialisation without the nonce (Node.cpp:155-168); the digest
        sees the ttl the wire carries."""
        return oracle.announce_pow_prefix(self.chunk_id, self.peer_id, self.endpoint, self.uri, self.shards,
                                          self.ttl & 0xFFFFFFFF)


def announce_message(a: Announce, type_byte: int = ANNOUNCE, raw_version: bool = False) -> bytes:
    """encode (Message.cpp:204-235): the version clamped (raw_version: as given, for frames encode
    cannot make); the nonce only when the version is 4."""
    assert len(a.chunk_id) == 32 and len(a.peer_id) == 32
    v = a.version if raw_version else clamp_version(a.version)
    m = bytes([v, type_byte]) + (a.ttl & 0xFFFFFFFF).to_bytes(4, "big")
    m += len(a.endpoint).to_bytes(4, "big") + len(a.uri).to_bytes(4, "big") + len(a.shards).to_bytes(4, "big")
    m += a.chunk_id + a.peer_id + a.endpoint + a.uri + a.shards
    if v >= 4:
        m += a.work_nonce.to_bytes(8, "big")
    return m


def message_len(a: Announce) -> int:
    return FIXED + a.flen + (8 if clamp_version(a.version) >= 4 else 0)


def parse_announce(m: bytes):
    """decode (Message.cpp:268-303) for an Announce: None when it does not decode as one, else
    (Announce, bytes after the payload).  decode expects the nonce for version >= 3."""
    if len(m) < 2 or not 1 <= m[0] <= 4 or m[1] != ANNOUNCE:
        return None
    v, rest = m[0], m[2:]
    extra = 8 if v >= 3 else 0
    if len(rest) < 16 + 64 + extra:
        return None
    ttl, E, U, A = (int.from_bytes(rest[4 * i:4 * i + 4], "big") for i in range(4))
    want = 16 + 64 + E + U + A + extra
    if len(rest) < want:
        return None
    at = 80
    a = Announce(chunk_id=rest[16:48], peer_id=rest[48:80], endpoint=rest[at:at + E], uri=rest[at + E:at + E + U],
                 shards=rest[at + E + U:at + E + U + A], ttl=ttl, version=v,
                 work_nonce=int.from_bytes(rest[want - 8:want], "big") if extra else 0)
    return a, len(rest) - want


def wire_of(nonce: bytes, body: bytes) -> bytes:
    """nonce(12) || BE32(|body|) || body (SessionManager.cpp:376-387)."""
    return nonce + len(body).to_bytes(4, "big") + body


def wire_frame(key: bytes, nonce: bytes, message: bytes) -> bytes:
    return wire_of(nonce, oracle.frame_seal(key, nonce, message))


def search_nonce(a: Announce, difficulty: int, max_attempts: int = NODE_POW_ATTEMPTS):
    """compute_announce_pow (Node.cpp:212-230) -> (found, nonce)."""
    if difficulty == 0:
        return True, 0
    found, nonce, _ = oracle.pow_search(a.prefix(), difficulty, POW_NODE, max_attempts)
    return found, (nonce if found else 0)


def pow_valid(a: Announce, difficulty: int) -> bool:
    """verify_announce_pow (Node.cpp:1144-1151): the wire version decides before the digest."""
    if difficulty == 0:
        return True
    if a.version < 3:
        return False
    return oracle.pow_check(a.prefix(), a.work_nonce, difficulty)


def seal_expect(a: Announce, key: bytes, nonce: bytes, difficulty: int, max_attempts: int = NODE_POW_ATTEMPTS,
                given_nonce: int = 0):
    """What enet_announce_frame_seal_batch owes for one record -> (status, frame or None, work_nonce).
    Only v4 records are searched; max_attempts == 0 passes given_nonce through."""
    v = clamp_version(a.version)
    found, wn = True, 0
    if v == 4:
        if max_attempts == 0:
            wn = given_nonce
        else:
            found, wn = search_nonce(a, difficulty, max_attempts)
    if not found:
        return POW, None, 0
    m = announce_message(dataclasses.replace(a, work_nonce=wn))
    return OK, wire_frame(key, nonce, m), wn


def admit(frame: bytes, key: bytes, peer: bytes, difficulty: int):
    """What enet_announce_frame_open_batch owes for one frame -> (status, message, info words).
    The checks in the reference's order; bytes after the payload are HEADER (the call's one
    documented difference from decode)."""
    none = (b"", [0] * 8)
    if len(frame) < OVERHEAD or int.from_bytes(frame[12:16], "big") != len(frame) - 16:
        return (FRAME,) + none
    ok, m = oracle.frame_open(key, frame[:12], frame[16:])
    if not ok:
        return (FRAME,) + none
    parsed = parse_announce(m)
    if parsed is None or parsed[1] != 0:
        return (HEADER,) + none
    a = parsed[0]
    if a.peer_id != peer:
        return (SENDER,) + none
    if not a.uri:
        return (NO_MANIFEST,) + none
    if not pow_valid(a, difficulty):
        return (POW,) + none
    info = [a.version, a.ttl, len(a.endpoint), len(a.uri), len(a.shards), a.work_nonce & 0xFFFFFFFF,
            a.work_nonce >> 32, 0]
    return OK, m, info
