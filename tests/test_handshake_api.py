"""CPU tests of the device session table: the pure-Python restatement (tests/handshake_ref.py)
against every case the compiled reference recorded (tests/golden/handshake.json, made by
tools/gen_handshake_golden.py), and the C ABI's argument checks (no GPU is touched by a rejected
call or a no-op)."""
import ctypes as C
import hashlib
import json
import os

import pytest

import handshake_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 2147483647


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "handshake.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib_path():
    from ephemeralnet_amd import build as B
    return B.build(verbose=False)


def test_golden_covers_the_edge_cases(golden):
    cases = golden["cases"]
    assert golden["prime"] == H.P == P and golden["generator"] == H.G == 5
    assert len(cases) >= 16
    assert {0, 1, 2**32 - 1} <= {c["local_private"] for c in cases}
    assert {0, 1, 2, P - 1, P, P + 1, 2**32 - 1} <= {c["remote_public"] for c in cases}
    assert any(1 < c["scalar"] < 2**24 for c in cases)                       # a zero top byte in BE32(scalar)
    assert any(c["local_public"] == c["remote_public"] for c in cases)       # equal publics
    assert any(not c["remote_valid"] for c in cases) and any(c["remote_valid"] for c in cases)
    assert all(c["rotate_counter"] == 1 for c in cases)
    lzb = [p["leading_zero_bits"] for p in golden["handshake_pow"]]
    assert 0 in lzb and max(lzb) >= 12


def test_restatement_matches_every_golden_case(golden):
    for c in golden["cases"]:
        priv, remote = c["local_private"], c["remote_public"]
        assert H.compute_public(priv) == c["local_public"], c
        if c["remote_private"] is not None:
            assert H.compute_public(c["remote_private"]) == remote, c
            assert H.shared_secret(c["remote_private"], c["local_public"]).hex() == c["secret"], c
        assert H.validate_public(remote) == c["remote_valid"], c
        assert H.shared_scalar(priv, remote) == c["scalar"], c
        secret = H.shared_secret(priv, remote)
        assert secret.hex() == c["secret"], c
        material = H.handshake_material(c["local_public"], remote)
        assert material.hex() == c["material"], c
        assert H.material_key(secret, material).hex() == c["material_key"], c
        assert H.derive_key(secret, c["rotate_counter"], c["rotate_ticks"]).hex() == c["rotated_key"], c
        assert H.rotate(1, secret, 0, 0, c["rotate_ticks"], 10**9) == (1, bytes.fromhex(c["rotated_key"])), c
    for p in golden["handshake_pow"]:
        d = H.pow_digest(bytes.fromhex(p["initiator"]), bytes.fromhex(p["responder"]), p["public"], p["nonce"])
        assert d.hex() == p["digest"], p
        assert H.leading_zero_bits(d) == p["leading_zero_bits"], p
        for diff in (0, p["leading_zero_bits"], p["leading_zero_bits"] + 1):
            want = diff == 0 or diff <= p["leading_zero_bits"]
            assert H.pow_valid(bytes.fromhex(p["initiator"]), bytes.fromhex(p["responder"]), p["public"],
                               p["nonce"], diff) == want, p


def test_anchor_case(golden):
    """privates 123456789 / 987654321, worked from the formulas; the golden file rules."""
    c = next(x for x in golden["cases"] if (x["local_private"], x["remote_private"]) == (123456789, 987654321))
    assert (c["local_public"], c["remote_public"], c["scalar"]) == (1891294900, 1686535327, 753432501)
    assert c["secret"].startswith("d3334095") and c["secret"].endswith("c42a748b")
    assert c["material"] == "64867c9f70badeb4"
    assert c["material_key"].startswith("d147d9f2") and c["material_key"].endswith("8c2e3af8")
    assert hashlib.sha256((753432501).to_bytes(4, "big")).hexdigest() == c["secret"]


def test_restatement_admission_order():
    """perform_handshake's order: public, then PoW, then (the table's) slot."""
    peer, local = bytes(range(32)), bytes(range(32, 64))
    pub = H.compute_public(1234)
    bad_nonce = next(n for n in range(64) if not H.pow_valid(peer, local, pub, n, 8))
    good = H.solve_pow(peer, local, pub, 8)
    lp = H.compute_public(99)
    assert H.accept(peer, 1, good, 0, 4, local, 99, lp, 8)[0] == H.HS_BAD_PUBLIC
    assert H.accept(peer, P, None, 9, 4, local, 99, lp, 0)[0] == H.HS_BAD_PUBLIC     # before the slot check
    assert H.accept(peer, pub, bad_nonce, 9, 4, local, 99, lp, 8)[0] == H.HS_BAD_POW  # before the slot check
    assert H.accept(peer, pub, good, 4, 4, local, 99, lp, 8)[0] == H.HS_BAD_SLOT
    v, secret, key = H.accept(peer, pub, good, 3, 4, local, 99, lp, 8)
    assert v == H.HS_OK and secret == H.shared_secret(1234, lp)                       # both peers agree
    assert H.accept(peer, pub, None, 3, 4, local, 99, lp, 0) == (v, secret, key)      # difficulty 0: no nonce


def test_handshake_abi_rejects_bad_arguments_without_gpu(lib_path):
    """enet_handshake_accept_batch / enet_session_rotate_batch / enet_key_exchange_batch: a NULL
    required buffer, a misaligned row, difficulty > 255, difficulty != 0 without work_nonce and a
    negative interval return ENET_EINVAL with the function's short name first in
    enet_last_error(); n == 0 and sessions == 0 are no-ops."""
    import ephemeralnet_amd as E
    L = E.lib()
    assert L.enet_abi_version() == (1 << 16) | 4
    assert (E.ENET_HS_BAD_PUBLIC, E.ENET_HS_OK, E.ENET_HS_BAD_POW, E.ENET_HS_BAD_SLOT) == (0, 1, 2, 3)
    raw = (C.c_uint8 * 16384)()
    base = (C.addressof(raw) + 15) & ~15     # 16-byte aligned host memory: never dereferenced
    a = [base + 1024 * k for k in range(14)]

    def table(sessions=4, **over):
        t = E._SessionTable()
        t.sessions = sessions
        t.secrets, t.keys, t.mid, t.counters, t.last_rotation, t.live = a[0], a[1], a[2], a[3], a[4], a[5]
        for k, v in over.items():
            setattr(t, k, v)
        return t

    acc, rot, kx = L.enet_handshake_accept_batch, L.enet_session_rotate_batch, L.enet_key_exchange_batch
    peers, pubs, nonces, slots, lid, verdict = a[6], a[7], a[8], a[9], a[10], a[11]

    def accept(t=None, n=3, peer_ids=peers, remote=pubs, nonce=nonces, slot=slots, local_id=lid, difficulty=8,
               out=verdict):
        return acc(C.byref(t) if t is not None else None, n, peer_ids, remote, nonce, slot, local_id, 5, 3125,
                   difficulty, 1000, out, None)

    bad_tables = [dict(secrets=None), dict(keys=None), dict(mid=None), dict(counters=None), dict(last_rotation=None),
                  dict(live=None), dict(secrets=a[0] + 1), dict(keys=a[1] + 2), dict(mid=a[2] + 3),
                  dict(counters=a[3] + 4), dict(last_rotation=a[4] + 4)]
    for over in bad_tables:
        assert accept(table(**over)) == -1, over
        assert L.enet_last_error().startswith(b"handshake_accept"), over
        assert rot(C.byref(table(**over)), 10, 5, a[12], None) == -1, over
        assert L.enet_last_error().startswith(b"session_rotate"), over
    for kw in [dict(t=None), dict(remote=None), dict(out=None), dict(nonce=None), dict(peer_ids=None),
               dict(local_id=None), dict(difficulty=256), dict(difficulty=2**32 - 1),
               dict(peer_ids=peers + 1), dict(local_id=lid + 2), dict(remote=pubs + 1), dict(slot=slots + 2),
               dict(nonce=nonces + 4), dict(nonce=None, difficulty=255)]:
        kw.setdefault("t", table())
        assert accept(**kw) == -1, kw
        assert L.enet_last_error().startswith(b"handshake_accept"), kw
    assert rot(None, 10, 5, a[12], None) == -1 and L.enet_last_error().startswith(b"session_rotate")
    assert rot(C.byref(table()), 10, -1, a[12], None) == -1 and L.enet_last_error().startswith(b"session_rotate")
    assert rot(C.byref(table()), 10, -2**63, a[12], None) == -1
    assert rot(C.byref(table()), 10, 5, None, None) == -1 and L.enet_last_error().startswith(b"session_rotate")
    for args in [(3, None, pubs, a[12], a[13]), (3, a[6], None, a[12], a[13]),       # NULL privates; secrets without remotes
                 (3, a[6] + 1, pubs, a[12], a[13]), (3, a[6], pubs + 2, a[12], a[13]),
                 (3, a[6], pubs, a[12] + 3, a[13]), (3, a[6], pubs, a[12], a[13] + 1)]:
        assert kx(*args, None) == -1, args
        assert L.enet_last_error().startswith(b"key_exchange"), args
    # no-ops: nothing is launched, so no device is needed
    assert accept(table(), n=0) == 0
    assert accept(table(), n=0, remote=None, out=None, nonce=None) == 0
    assert accept(table(sessions=0, secrets=None, keys=None, mid=None, counters=None, last_rotation=None, live=None),
                  n=0) == 0
    assert rot(C.byref(table(sessions=0)), 10, 5, None, None) == 0
    assert rot(C.byref(table(sessions=0, secrets=None, keys=None, mid=None, counters=None, last_rotation=None,
                             live=None)), 10, 0, None, None) == 0
    assert kx(0, None, None, None, None, None) == 0
