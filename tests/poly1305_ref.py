"""Plain Poly1305 (RFC 8439 2.5, 2.8) in Python integers, and records crafted so that a chosen
Poly1305 accumulator takes a chosen value.

Test reference only: no limbs, no carries, nothing imported from the package.  p = 2^130 - 5, a
message is cut into 16-byte blocks, block i is c_i = LE(bytes) + 2^(8 len), and the accumulator
runs h <- (h + c_i) r mod p; the tag is (h + s) mod 2^128.  In the AEAD the message is
aad || pad || ct || pad || LE64 |aad| || LE64 |ct|, every block of it 16 bytes long, and the key
(r, s) is ChaCha20 block 0 of the record's (key, nonce): it cannot be chosen.  The ciphertext can
(on the seal side the plaintext is ct XOR keystream), and every accumulator is affine in any one
block, so for a given (key, nonce) one block m = (target - base) r^-k mod p puts an accumulator on
any target.  m must be a legal full block, 2^128 <= m < 2^129, which holds for about one nonce in
four: craft() walks a seeded nonce sequence until it does.

Scopes (Poly1305 block indices over the whole MAC stream, AAD blocks first, the length block last):
    ("final",)        the accumulator after the length block, H before + s
    ("prefix", i)     the accumulator after block i
    ("range", a, b)   the accumulator of blocks a..b started from zero: what one lane of a record
                      kernel, or one tile, holds after its own run of blocks
Each is the Horner value including the multiplication by r that follows its last block."""
from __future__ import annotations

import hashlib
import itertools
from dataclasses import dataclass

import oracle

P = (1 << 130) - 5
M128 = (1 << 128) - 1
CLAMP = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
CAP = 128                # nonces tried per crafted record
HEAVY_CAP = 1 << 16      # nonces searched for a heavy r


def key_rs(key32: bytes):
    """(clamped r, s) of a 32-byte one-time key."""
    return int.from_bytes(key32[:16], "little") & CLAMP, int.from_bytes(key32[16:32], "little")


def blocks(msg: bytes) -> list:
    """c_i of every 16-byte block of msg (the last one may be shorter)."""
    return [int.from_bytes(msg[i:i + 16], "little") + (1 << (8 * min(16, len(msg) - i)))
            for i in range(0, len(msg), 16)]


def horner(r: int, cs, h: int = 0) -> int:
    for c in cs:
        h = (h + c) * r % P
    return h


def poly1305(key32: bytes, msg: bytes) -> bytes:
    r, s = key_rs(key32)
    return ((horner(r, blocks(msg)) + s) & M128).to_bytes(16, "little")


def mac_data(aad: bytes, ct: bytes) -> bytes:
    pad = lambda b: b + bytes(-len(b) % 16)
    return pad(aad) + pad(ct) + len(aad).to_bytes(8, "little") + len(ct).to_bytes(8, "little")


def aead_tag(otk32: bytes, aad: bytes, ct: bytes) -> bytes:
    return poly1305(otk32, mac_data(aad, ct))


def one_time_key(key: bytes, nonce: bytes) -> bytes:
    return oracle.chacha20_block(key, nonce, 0)[:32]


def keystream_xor(key: bytes, nonce: bytes, data: bytes) -> bytes:
    """ct -> pt and pt -> ct (RFC 8439 2.8: data counter 1)."""
    return oracle.chacha20_xor(key, nonce, data, 1)


def seeded_bytes(seed: int, n: int) -> bytes:
    return hashlib.shake_128(b"poly1305 edges %d" % seed).digest(n) if n else b""


def nonce_seq(seed: int):
    """The seeded nonce sequence of one record: LE32(seed) || LE64(0, 1, 2, ...)."""
    for k in itertools.count():
        yield (seed & 0xFFFFFFFF).to_bytes(4, "little") + k.to_bytes(8, "little")


def counts(L: int, aad_len: int):
    """(AAD blocks, ciphertext blocks, blocks in all) of a record's MAC stream."""
    na, nct = (aad_len + 15) // 16, (L + 15) // 16
    return na, nct, na + nct + 1


def span(scope, N: int):
    """Block range (a, b) whose Horner value from zero the scope names."""
    if scope[0] == "final":
        return 0, N - 1
    if scope[0] == "prefix":
        return 0, scope[1]
    assert scope[0] == "range"
    return scope[1], scope[2]


def full_blocks(L: int, aad_len: int) -> list:
    """Stream indices of the blocks a record can give away: full 16-byte AAD / ciphertext blocks."""
    na = (aad_len + 15) // 16
    return list(range(aad_len // 16)) + [na + i for i in range(L // 16)]


class CraftError(RuntimeError):
    pass


@dataclass
class Crafted:
    key: bytes
    nonce: bytes
    aad: bytes
    ct: bytes
    otk: bytes
    attempts: int
    target: int = -1     # the value reached (-1: not crafted)
    scope: tuple = ()

    @property
    def pt(self) -> bytes:
        return keystream_xor(self.key, self.nonce, self.ct)

    @property
    def tag(self) -> bytes:
        return aead_tag(self.otk, self.aad, self.ct)


def _slot(na: int, aad_len: int, L: int, idx: int):
    """(in_aad, byte offset) of stream block idx, which must be a full AAD / ciphertext block."""
    if idx < na:
        assert 16 * idx + 16 <= aad_len, "the block is not a full AAD block"
        return True, 16 * idx
    assert 16 * (idx - na) + 16 <= L, "the block is not a full ciphertext block"
    return False, 16 * (idx - na)


NEXT_ONE = (1).to_bytes(16, "little")  # the block 01 00 .. 00


def craft(key: bytes, nonces, L: int, aad_len: int, free_block: int, target, scope, *, fill=0,
          then: bytes = None, cap: int = CAP) -> Crafted:
    """A record (nonce, aad, ct) of L ciphertext and aad_len AAD bytes under `key` whose accumulator
    `scope` equals `target` mod p.  target: an integer below p, or a function of the pad s giving one
    (None: this nonce cannot take the target; the next is tried).  free_block: the stream index of
    the full block that is solved for, inside the scope (a scope of that block alone cannot take
    the target 0).  fill: seed of the other bytes, or one byte
    value repeated.  then: 16 bytes put in the block after the scope's last one (a full block).
    Tries at most `cap` nonces of the sequence and raises CraftError after that.  Cost: one Horner
    pass over the scope's blocks per nonce tried, and one checking pass for the nonce accepted."""
    na, nct, N = counts(L, aad_len)
    a, b = span(scope, N)
    assert 0 <= a <= free_block <= b <= N - 1
    raw = bytes([fill[0]]) * (aad_len + L) if isinstance(fill, bytes) else seeded_bytes(fill, aad_len + L)
    aad, ct = bytearray(raw[:aad_len]), bytearray(raw[aad_len:])
    in_aad, at = _slot(na, aad_len, L, free_block)
    (aad if in_aad else ct)[at:at + 16] = bytes(16)
    if then is not None:
        assert len(then) == 16 and b + 1 != free_block
        t_aad, t_at = _slot(na, aad_len, L, b + 1)
        (aad if t_aad else ct)[t_at:t_at + 16] = then
    cs = blocks(mac_data(bytes(aad), bytes(ct)))
    assert len(cs) == N
    cs[free_block] = 0
    scoped = cs[a:b + 1]
    k = b - free_block + 1  # the free block is multiplied by r^k
    attempts = 0
    for nonce in itertools.islice(nonces, cap):
        attempts += 1
        otk = one_time_key(key, nonce)
        r, s = key_rs(otk)
        t = target(s) if callable(target) else target
        if t is None or r == 0:
            continue
        assert 0 <= t < P
        m = (t - horner(r, scoped)) * pow(r, -k, P) % P
        if not (1 << 128) <= m < (1 << 129):
            continue
        (aad if in_aad else ct)[at:at + 16] = (m - (1 << 128)).to_bytes(16, "little")
        rec = Crafted(key, nonce, bytes(aad), bytes(ct), otk, attempts, t, tuple(scope))
        assert horner(r, blocks(mac_data(rec.aad, rec.ct))[a:b + 1]) == t, "crafting is wrong"
        return rec
    raise CraftError(f"no nonce in {cap} puts {scope} on the target (L {L}, aad {aad_len})")


def plain(key: bytes, nonce: bytes, aad: bytes, ct: bytes) -> Crafted:
    """A record that is not crafted (extreme data, heavy r)."""
    return Crafted(key, nonce, aad, ct, one_time_key(key, nonce), 0)


HEAVY_BITS = 0x0E000000  # the top three bits the clamp leaves free in each 32-bit word of r


def heavy_nonce(key: bytes, nonces, cap: int = HEAVY_CAP):
    """(nonce, nonces tried): the first nonce of the sequence whose clamped r has the top three
    free bits of all four words set (about 2^-12 per nonce; CraftError after `cap`).  A stress of
    the kernels' column-sum headroom (radix 2^32: sums < 2^63; radix 2^26: < 2^58), not a boundary:
    the true maximum r = 0x0ffffffc0ffffffc0ffffffc0fffffff is one value among 2^124 and cannot be
    reached through ChaCha20."""
    for tried, nonce in enumerate(itertools.islice(nonces, cap), 1):
        r, _ = key_rs(one_time_key(key, nonce))
        if all((r >> (32 * w)) & HEAVY_BITS == HEAVY_BITS for w in range(4)):
            return nonce, tried
    raise CraftError(f"no heavy r in {cap} nonces")


# ------------------------------------------------------------------------------- target sets
# (name, value or function of the pad s).  The words only say why each is there.
def _minus_s(k):
    def f(s):
        t = (-s & M128) + (k << 128)
        return t if t < P else None
    return f


FINAL_TARGETS = (
    # the conditional subtraction of p, whichever representative the kernel holds
    [(f"{d}", d) for d in range(6)] + [("p-1", P - 1), ("p-5", P - 5), ("p-6", P - 6)]
    # the top two bits are dropped by the tag
    + [("2^128-1", M128)] + [(f"{k}*2^128", k << 128) for k in (1, 2, 3)]
    # repack boundaries, radix 2^26 and radix 2^32
    + [(f"2^{26 * j}-1", (1 << 26 * j) - 1) for j in (1, 2, 3, 4)]
    + [(f"2^{26 * j}", 1 << 26 * j) for j in (1, 2, 3, 4)]
    + [(f"2^{32 * j}-1", (1 << 32 * j) - 1) for j in (1, 2, 3)]
    + [(f"2^{32 * j}", 1 << 32 * j) for j in (1, 2, 3)]
    # h + s = 2^128 exactly: a zero tag with the carry running out of every word
    + [(f"-s+{k}*2^128", _minus_s(k)) for k in (0, 1, 2, 3)]
    # an all-ones tag
    + [("-s-1", lambda s: (-s - 1) & M128)]
    # the + s carry dies at word j
    + [(f"2^{32 * j}-s%2^{32 * j}", (lambda j: lambda s: (1 << 32 * j) - (s & ((1 << 32 * j) - 1)))(j))
       for j in (1, 2, 3)]
)

# Horner prefixes and lane / tile sums: the radix-2^32 and radix-2^26 states.  `then`: the block
# that follows the state (None: whatever the fill gives).
STATE_TARGETS = (
    # above 2^128 the radix-2^32 step's fold term is about 2^31, so these few are reached only
    # through the carry that ripples out of all four words
    [(f"{k}*2^128+{d}", (k << 128) + d, None) for k in (1, 2, 3) for d in (0, 1)]
    + [("0", 0, None)]
    # every 26-bit limb at its maximum going into the limb multiplication
    + [("p-1", P - 1, None)]
    # h + m = 2^128: the four-word add chain carries into the fifth
    + [("2^128-1 then 1", M128, NEXT_ONE)]
)
