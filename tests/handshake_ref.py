"""Pure-Python restatement of the reference's handshake chain (pow / hashlib / hmac only; nothing
here touches the library), the yardstick of the device session table's tests:

  validate_public, modexp, derive_shared_secret   src/network/KeyExchange.cpp:9-48
  handshake_pow_digest / handshake_pow_valid      src/core/Node.cpp:232-256
  make_handshake_material                         src/core/Node.cpp:61-75
  register_session_with_material, derive_key      src/network/KeyManager.cpp:32-46, 74-92
  perform_handshake's order of checks             src/core/Node.cpp:1872-1926

tests/golden/handshake.json (recorded from the compiled reference) pins it."""
import hashlib
import hmac

P = 2147483647          # KeyExchange::kPrime
G = 5                   # KeyExchange::kGenerator
HS_BAD_PUBLIC, HS_OK, HS_BAD_POW, HS_BAD_SLOT = 0, 1, 2, 3


def compute_public(private: int) -> int:
    return pow(G, private & 0xFFFFFFFF, P)


def validate_public(candidate: int) -> bool:
    return 1 < candidate < P


def shared_scalar(private: int, remote_public: int) -> int:
    # modexp: result starts at 1 % P, base is reduced first; exponent 0 -> 1, base 0 -> 0
    return pow((remote_public & 0xFFFFFFFF) % P, private & 0xFFFFFFFF, P)


def shared_secret(private: int, remote_public: int) -> bytes:
    return hashlib.sha256(shared_scalar(private, remote_public).to_bytes(4, "big")).digest()


def handshake_material(local_public: int, remote_public: int) -> bytes:
    lo, hi = sorted((local_public & 0xFFFFFFFF, remote_public & 0xFFFFFFFF))
    return lo.to_bytes(4, "big") + hi.to_bytes(4, "big")


def material_key(secret: bytes, material: bytes) -> bytes:
    return hmac.new(secret, material, hashlib.sha256).digest()


def derive_key(secret: bytes, counter: int, ticks: int) -> bytes:
    m = (counter & (2**64 - 1)).to_bytes(8, "big") + (ticks & (2**64 - 1)).to_bytes(8, "big")
    return hmac.new(secret, m, hashlib.sha256).digest()


def pow_message(initiator: bytes, responder: bytes, initiator_public: int, nonce: int) -> bytes:
    assert len(initiator) == 32 and len(responder) == 32
    be64 = lambda v: (v & (2**64 - 1)).to_bytes(8, "big")  # noqa: E731
    return be64(32) + initiator + be64(32) + responder + be64(initiator_public & 0xFFFFFFFF) + be64(nonce)


def pow_digest(initiator: bytes, responder: bytes, initiator_public: int, nonce: int) -> bytes:
    return hashlib.sha256(pow_message(initiator, responder, initiator_public, nonce)).digest()


def leading_zero_bits(digest: bytes) -> int:
    total = 0
    for b in digest:
        if b == 0:
            total += 8
            continue
        return total + (8 - b.bit_length())
    return total


def pow_valid(initiator: bytes, responder: bytes, initiator_public: int, nonce: int, difficulty: int) -> bool:
    if difficulty == 0:
        return True
    return leading_zero_bits(pow_digest(initiator, responder, initiator_public, nonce)) >= difficulty


def solve_pow(initiator: bytes, responder: bytes, initiator_public: int, difficulty: int, start: int = 0) -> int:
    nonce = start
    while not pow_valid(initiator, responder, initiator_public, nonce, difficulty):
        nonce = (nonce + 1) & (2**64 - 1)
    return nonce


def accept(peer_id: bytes, remote_public: int, work_nonce, slot: int, sessions: int, local_id: bytes,
           local_private: int, local_public: int, difficulty: int):
    """One record of the admission: (verdict, secret, key); secret and key are None unless
    accepted.  work_nonce may be None when difficulty == 0."""
    if not validate_public(remote_public & 0xFFFFFFFF):
        return HS_BAD_PUBLIC, None, None
    if difficulty != 0 and not pow_valid(peer_id, local_id, remote_public, work_nonce, difficulty):
        return HS_BAD_POW, None, None
    if slot >= sessions:
        return HS_BAD_SLOT, None, None
    secret = shared_secret(local_private, remote_public)
    return HS_OK, secret, material_key(secret, handshake_material(local_public, remote_public))


def rotate(live: int, secret: bytes, counter: int, last: int, now: int, interval: int):
    """rotate_if_needed on one slot: None when not due, else (counter, key)."""
    if not live or now - last < interval:
        return None
    c = (counter + 1) & (2**64 - 1)
    return c, derive_key(secret, c, now)
