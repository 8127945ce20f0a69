"""Test helper for the chunk transfer frames: the 42-byte `Chunk` message header
(protocol::encode, src/protocol/Message.cpp:204-246) and the frames the oracle module makes of it.
Pinned against the compiled reference's golden "chunk" frames by tests/test_chunk_frames_api.py."""
from __future__ import annotations

import oracle

HEADER = 42
OVERHEAD = 16 + HEADER + 32  # wire header, message header, MAC


def clamp_version(v: int) -> int:
    """clamp_version (Message.cpp:17-25)."""
    return min(max(v, 1), 4)


def chunk_header(version: int, ttl: int, chunk_id: bytes, data_len: int, type_byte: int = 0x03) -> bytes:
    """version(1) || 0x03 || BE32(ttl seconds) || BE32(|data|) || chunk_id(32); the version as given."""
    assert len(chunk_id) == 32
    return bytes([version, type_byte]) + ttl.to_bytes(4, "big") + data_len.to_bytes(4, "big") + chunk_id


def chunk_message(version: int, ttl: int, chunk_id: bytes, data: bytes) -> bytes:
    return chunk_header(clamp_version(version), ttl, chunk_id, len(data)) + data


def wire_of(nonce: bytes, body: bytes) -> bytes:
    """nonce(12) || BE32(|body|) || body (SessionManager.cpp:376-387)."""
    return nonce + len(body).to_bytes(4, "big") + body


def wire_frame(key: bytes, nonce: bytes, message: bytes) -> bytes:
    return wire_of(nonce, oracle.frame_seal(key, nonce, message))


def stored_data(chunk_key: bytes, chunk_nonce: bytes, chunk_id: bytes, plaintext: bytes) -> bytes:
    """encrypt_with_key (CryptoManager.cpp:38-46): ChaCha20 from LE32(chunk_id[0..3])."""
    return oracle.chacha20_xor(chunk_key, chunk_nonce, plaintext, oracle.derive_counter(chunk_id))
