"""Poly1305 at its edges, on the CPU: the big-integer reference (tests/poly1305_ref.py) against the
pinned tags, and the CPU oracle (oracle/enet_oracle.c, 44-bit limbs; what every GPU AEAD test
trusts) against the reference -- with the key given directly, where r and s are free, and through
the AEAD on records crafted so that the final accumulator, a Horner prefix or a block range's sum
lands on a boundary value.  Seeded random data never takes those branches (an accumulator in
[p, 2^130) is a 2^-128 event)."""
import functools
import time

import pytest

import oracle
import poly1305_ref as ref
from poly1305_ref import CLAMP, FINAL_TARGETS, M128, P, STATE_TARGETS
from util import splitmix_bytes

LENS = [0, 1, 15, 16, 17, 63, 64, 65, 100, 1500, 4096]
AADS = [0, 1, 16, 17]
KEY = bytes(range(32))


# ------------------------------------------------------------------ the reference against pinned tags
def test_reference_reproduces_pinned_tags(golden):
    for c in golden["poly1305"]:
        assert ref.poly1305(bytes.fromhex(c["key"]), bytes.fromhex(c["msg"])).hex() == c["tag"]
    v = golden["rfc8439_2_8_2"]
    k, n = bytes.fromhex(v["key"]), bytes.fromhex(v["nonce"])
    assert ref.keystream_xor(k, n, bytes.fromhex(v["pt"])).hex() == v["ct"]
    tag = ref.aead_tag(ref.one_time_key(k, n), bytes.fromhex(v["aad"]), bytes.fromhex(v["ct"]))
    assert tag.hex() == v["tag"] == "1ae10b594f09e26a7e902ecbd0600691"
    for c in golden["aead"]:
        k, n = bytes.fromhex(c["key"]), bytes.fromhex(c["nonce"])
        aad = splitmix_bytes(c["aad_seed"], c["aad_len"])
        ct = ref.keystream_xor(k, n, splitmix_bytes(c["pt_seed"], c["len"]))
        assert ref.aead_tag(ref.one_time_key(k, n), aad, ct).hex() == c["tag"]


# ------------------------------------------------------------------ the oracle, key given directly
R_RAW = [0, 1, 2, CLAMP, (1 << 124) - 4, M128]  # as key bytes: both sides clamp
SUMS = [("p-1", P - 1), ("p", P), ("p+4", P + 4), ("2^130-1", (1 << 130) - 1)]
LAST = [16, 1, 15]  # bytes of the last block


def message_reaching(r: int, want: int, last_len: int, seed: int) -> bytes:
    """Full blocks and a last block of last_len bytes such that the canonical accumulator plus the
    last block is exactly `want` (r != 0): the last block c takes seeded low bits, the accumulator
    before it must be want - c, and the last full block is solved for over one to three seeded
    blocks in front of it until it is a legal one (with r = 1 the full blocks simply add up, so how
    many can reach want - c depends on its size)."""
    hi = 1 << (8 * last_len)
    c = hi + int.from_bytes(ref.seeded_bytes(seed, last_len), "little") % hi
    if want - c >= P:  # (never for these sums: c > 4)
        raise AssertionError
    prev = want - c
    rinv = pow(r, -1, P)
    for k in range(ref.CAP):
        head = ref.seeded_bytes(1000 * seed + k, 16 * (1 + k % 3))
        c2 = (prev * rinv - ref.horner(r, ref.blocks(head))) % P
        if (1 << 128) <= c2 < (1 << 129):
            msg = head + (c2 - (1 << 128)).to_bytes(16, "little") + (c - hi).to_bytes(last_len, "little")
            cs = ref.blocks(msg)
            assert ref.horner(r, cs[:-1]) + cs[-1] == want
            return msg
    raise ref.CraftError("no seeded blocks give a legal last full one")


def test_oracle_direct_key_edges():
    cases = 0
    for ri, raw in enumerate(R_RAW):
        r = raw & CLAMP
        msgs = [b"", b"\x00", bytes(16), b"\xff" * 16, b"\xff" * 15, b"\xff" * 64, b"\xff" * 49]
        if r:
            msgs += [message_reaching(r, want, ll, 97 * ri + 7 * si + ll)
                     for si, (_, want) in enumerate(SUMS) for ll in LAST]
        for msg in msgs:
            H = ref.horner(r, ref.blocks(msg))
            for s in (0, M128, -H & M128, (-H - 1) & M128, ((1 << 64) - H) & M128):
                key = raw.to_bytes(16, "little") + s.to_bytes(16, "little")
                want = ref.poly1305(key, msg)
                assert want == ((H + s) & M128).to_bytes(16, "little")
                assert oracle.poly1305(key, msg) == want, (hex(raw), hex(s), msg.hex())
                cases += 1
    assert cases == 5 * (7 * len(R_RAW) + len(SUMS) * len(LAST) * (len(R_RAW) - 1))


# ------------------------------------------------------------------ the oracle through the AEAD
def positions(full):
    """First, middle and last of the full blocks a record can give away (deduplicated, in order)."""
    return sorted({full[0], full[len(full) // 2], full[-1]})


def crafted_cases():
    """(L, aad_len, free block, scope kind, target name, target, scope, then) for every shape that
    has a full block to give away: the final-H set on the whole stream; the state set on a prefix
    ending halfway between the free block and the end, and on a range around the free block.  A
    state target with a next block needs a full block right after the scope."""
    for L in LENS:
        for alen in AADS:
            full = ref.full_blocks(L, alen)
            if not full:
                assert L < 16 and alen < 16
                continue
            na, nct, N = ref.counts(L, alen)
            for f in positions(full):
                for name, t in FINAL_TARGETS:
                    yield L, alen, f, "final", name, t, ("final",), None
                for name, t, then in STATE_TARGETS:
                    # (at least two blocks in the scope: the free block alone cannot sum to 0)
                    if then is None:
                        ends = [max(1, f + (N - 1 - f) // 2)]
                    else:
                        ends = [i for i in range(max(1, f), N - 1) if i + 1 in full][:1]
                    for e in ends:
                        yield L, alen, f, "prefix", name, t, ("prefix", e), then
                        yield L, alen, f, "range", name, t, ("range", max(0, f - 2), e), then


@functools.lru_cache(maxsize=None)
def crafted_set():
    t0 = time.time()
    out = []
    for i, (L, alen, f, kind, name, t, scope, then) in enumerate(crafted_cases()):
        rec = ref.craft(KEY, ref.nonce_seq(i), L, alen, f, t, scope, fill=i, then=then)
        out.append((kind, name, L, alen, rec))
    print(f"\n[poly1305 edges] {len(out)} crafted records in {time.time() - t0:.1f} s")
    return out


def check_oracle(rec, what):
    pt = rec.pt
    want = rec.tag
    ct, tag = oracle.aead_seal(rec.key, rec.nonce, pt, rec.aad)
    assert ct == rec.ct and tag == want, (what, "seal", tag.hex(), want.hex())
    ok, back = oracle.aead_open(rec.key, rec.nonce, rec.ct, want, rec.aad)
    assert ok and back == pt, (what, "open")
    bad = bytes([want[0] ^ 1]) + want[1:]
    assert not oracle.aead_open(rec.key, rec.nonce, rec.ct, bad, rec.aad)[0], (what, "flipped tag opens")


def test_oracle_on_crafted_set():
    recs = crafted_set()
    names = {(kind, name) for kind, name, *_ in recs}
    assert names == {("final", n) for n, _ in FINAL_TARGETS} | \
        {(k, n) for k in ("prefix", "range") for n, _, _ in STATE_TARGETS}
    for kind, name, L, alen, rec in recs:
        check_oracle(rec, (kind, name, L, alen))


def test_crafted_final_values_are_what_they_say():
    """The crafting tool itself: the tag of a record crafted to final H is (H + s) mod 2^128, so the
    zero tag, the all-ones tag and the values at and around p come out as named."""
    seen = set()
    for kind, name, L, alen, rec in crafted_set():
        if kind != "final":
            continue
        s = ref.key_rs(rec.otk)[1]
        assert int.from_bytes(rec.tag, "little") == (rec.target + s) & M128
        if name.startswith("-s+"):
            assert rec.tag == bytes(16)
        if name == "-s-1":
            assert rec.tag == b"\xff" * 16
        seen.add(name)
    assert len(seen) == len(FINAL_TARGETS)


def test_oracle_on_extreme_data_and_heavy_r():
    """Ciphertext all 0xFF and all 0x00 at every length and AAD length (the shapes with no full
    block included), under an ordinary r and under a heavy one."""
    nonce, tried = ref.heavy_nonce(KEY, ref.nonce_seq(0xEA))
    print(f"\n[poly1305 edges] heavy r after {tried} nonces")
    assert tried <= ref.HEAVY_CAP
    for n in (ref.nonce_seq(1).__next__(), nonce):
        for L in LENS:
            for alen in AADS:
                for byte in (b"\xff", b"\x00"):
                    check_oracle(ref.plain(KEY, n, byte * alen, byte * L), (L, alen, byte))
                check_oracle(ref.plain(KEY, n, ref.seeded_bytes(L, alen), ref.seeded_bytes(alen, L)), (L, alen))


def test_attempts_stay_within_the_cap():
    """The only statistic: nonces tried per crafted record, by scope."""
    worst, total, count = {}, {}, {}
    for kind, name, L, alen, rec in crafted_set():
        worst[kind] = max(worst.get(kind, 0), rec.attempts)
        total[kind] = total.get(kind, 0) + rec.attempts
        count[kind] = count.get(kind, 0) + 1
    for kind in worst:
        print(f"\n[poly1305 edges] {kind}: {count[kind]} records, mean {total[kind] / count[kind]:.2f} "
              f"attempts, max {worst[kind]}")
        assert worst[kind] <= ref.CAP
    assert set(worst) == {"final", "prefix", "range"}


def test_craft_raises_when_the_cap_is_too_small():
    with pytest.raises(ref.CraftError):
        # target 0 on a final scope: one nonce in four works, so some seed fails on a single try
        for seed in range(64):
            ref.craft(KEY, ref.nonce_seq(seed), 64, 0, 0, 0, ("final",), cap=1)
