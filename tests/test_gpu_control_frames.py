"""GPU parity of the Request / Acknowledge frames and the frame triage (control_frames.hip:
enet_control_frame_seal_batch / enet_control_frame_open_batch / enet_frame_classify_batch) against
the CPU oracle through tests/control_frame_ref.py.  Frames are packed back to back behind a 1-byte
or a 3-byte sentinel base, so the 114- and 115-byte records start at every alignment mod 4 and mod
16; the sentinels around the arenas and in the slots an `order` does not name stay untouched.
Bit-exact throughout."""
import dataclasses
import json
import os

import numpy as np
import pytest

import oracle
from announce_frame_ref import Announce, admit, announce_message, parse_announce
from chunk_frame_ref import chunk_message, stored_data
from control_frame_ref import (ACK, FK_BAD, FRAME, HEADER, OK, OVERHEAD, REQUEST, classify, control_frame, control_message,
                               open_expect, open_message, parse_control, seal_expect, wire_frame, wire_of)
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = 0xAA
SESSIONS = 5
RECS_PER_WG = 64  # kControlRecsPerWG
SIZES = (1, 63, 64, 65, 2 * RECS_PER_WG + 1, 257)


@pytest.fixture(scope="module")
def enet():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ephemeralnet_amd as E
    E.lib()
    return E


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def devb(b: bytes):
    return dev(np.frombuffer(b, np.uint8).copy())


def dev_u8(vals):
    return dev(np.array(vals, dtype=np.uint8))


def dev_u32(vals):
    return dev(np.array(vals, dtype=np.uint32).view(np.int32))


def host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def offsets_for(lens, base):
    return np.concatenate([[base], base + np.cumsum(lens)]).astype(np.int64)


def records_of(arena: bytes, offs):
    return [arena[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def frame_len(kind):
    return 114 if kind == REQUEST else 115


@dataclasses.dataclass
class World:
    n: int
    kinds: list
    versions: list  # as given: 0..5
    accepted: list
    cids: list
    local: bytes
    table: list
    sess: list
    fnonces: list

    def key(self, i):
        return self.table[self.sess[i]] if self.sess[i] < SESSIONS else None

    def frame(self, i, accepted=None):
        acc = self.accepted[i] if accepted is None else accepted[i]
        return control_frame(self.key(i), self.fnonces[i], self.kinds[i], self.cids[i], self.local, bool(acc),
                             self.versions[i])


def make_world(seed, n, runs=False) -> World:
    """Kinds alternating, or in runs of 1..9; versions 0..5; accepted 0 / 1 / 2 / 255."""
    if runs:
        kinds, k = [], 0
        while len(kinds) < n:
            kinds += [[REQUEST, ACK][k % 2]] * (1 + (5 * k) % 9)
            k += 1
        kinds = kinds[:n]
    else:
        kinds = [[REQUEST, ACK][i % 2] for i in range(n)]
    return World(n=n, kinds=kinds, versions=[(i // 2) % 6 for i in range(n)],
                 accepted=[[0, 1, 2, 255, 1, 0, 0][i % 7] for i in range(n)],
                 cids=[splitmix_bytes(seed + 100 + i, 32) for i in range(n)], local=splitmix_bytes(seed + 1, 32),
                 table=[splitmix_bytes(seed + 10 + s, 32) for s in range(SESSIONS)],
                 sess=[int(x) % SESSIONS for x in splitmix_bytes(seed + 2, n)],
                 fnonces=[splitmix_bytes(seed + 5000 + i, 12) for i in range(n)])


def keys_for(enet, table, sess, sessions):
    """-> (keys tensor, key_stride, the session keywords)"""
    import torch
    if not sessions:
        return devb(b"".join(table[s] if s < len(table) else bytes(32) for s in sess)), 32, {}
    mid = torch.zeros(16 * len(table), dtype=torch.int32, device="cuda")
    tbl = devb(b"".join(table))
    enet.hmac_midstates(tbl, len(table), mid)
    return tbl, 32, dict(session=dev_u32(sess), sessions=len(table), mid=mid)


def run_seal(enet, w, base=1, sessions=True, accepted="given", out_lens=None, kinds=None, order=None, versions=True):
    """-> dict(frames, status, edges)"""
    import torch
    kinds = w.kinds if kinds is None else kinds
    lens = out_lens or [frame_len(k) for k in kinds]
    ooffs = offsets_for(lens, base)
    out = torch.full((int(ooffs[-1]) + 7,), SENT, dtype=torch.uint8, device="cuda")
    keys, stride, kw = keys_for(enet, w.table, w.sess, sessions)
    b = enet.Batch(arena=None, offsets=dev(ooffs), keys=keys, nonces=devb(b"".join(w.fnonces)), key_stride=stride,
                   order=None if order is None else dev_u32(order), count=None if order is None else len(order))
    status = torch.full((w.n,), 0x77, dtype=torch.uint8, device="cuda")
    acc = None if accepted == "null" else dev_u8(w.accepted if accepted == "given" else [0 if a else 1 for a in w.accepted])
    enet.control_frame_seal(b, out, b.offsets, dev_u8(kinds), devb(b"".join(w.cids)), devb(w.local), status,
                            accepted=acc, accept_zero=accepted == "zero",
                            versions=dev_u8(w.versions) if versions else None, **kw)
    o, offs = host(out), ooffs.tolist()
    return dict(frames=records_of(o, offs), status=status.cpu().tolist(), edges=[o[:offs[0]], o[offs[-1]:]])


def run_open(enet, frames, table, sess, base=1, sessions=True, senders=None, peers_out=True, order=None):
    """-> dict(status, cid, pid, info); the input arena and its sentinels must come back unchanged"""
    import torch
    n = len(frames)
    ioffs = offsets_for([len(f) for f in frames], base)
    arena = devb(bytes([SENT]) * base + b"".join(frames) + bytes([SENT]) * 3)
    keys, stride, kw = keys_for(enet, table, sess, sessions)
    b = enet.Batch(arena=arena, offsets=dev(ioffs), keys=keys, nonces=None, key_stride=stride,
                   order=None if order is None else dev_u32(order), count=None if order is None else len(order))
    status = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    cid = torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda")
    pid = torch.full((n, 32), 0x5B, dtype=torch.uint8, device="cuda") if peers_out else None
    info = torch.full((n, 4), 0x5C, dtype=torch.uint8, device="cuda")
    enet.control_frame_open(b, cid, info, status, peer_ids_out=pid, sender_ids=None if senders is None else devb(b"".join(senders)),
                            **kw)
    assert host(arena) == bytes([SENT]) * base + b"".join(frames) + bytes([SENT]) * 3
    return dict(status=status.cpu().tolist(), cid=records_of(host(cid), list(range(0, 32 * n + 1, 32))),
                pid=records_of(host(pid), list(range(0, 32 * n + 1, 32))) if peers_out else None,
                info=records_of(host(info), list(range(0, 4 * n + 1, 4))))


def check_open(r, frames, keys, senders=None, named=None):
    for i, f in enumerate(frames):
        if named is not None and i not in named:
            assert (r["status"][i], r["cid"][i], r["pid"][i], r["info"][i]) == (
                0x77, bytes([0x5A]) * 32, bytes([0x5B]) * 32, bytes([0x5C]) * 4), i
            continue
        st, cid, pid, info = open_expect(f, keys[i], None if senders is None else senders[i])
        assert r["status"][i] == st, (i, r["status"][i], st)
        assert r["cid"][i] == cid and r["info"][i] == info, i
        if r["pid"] is not None:
            assert r["pid"][i] == pid, i


def assert_sentinels(edges):
    for e in edges:
        assert e == bytes([SENT]) * len(e)


@pytest.fixture(scope="module")
def big():
    w = make_world(930000, 257)
    return w, [w.frame(i) for i in range(w.n)]


# ------------------------------------------------------------------ seal
@pytest.mark.parametrize("n", SIZES)
def test_seal_matches_oracle(enet, n):
    """Alternating kinds and kinds in runs, versions 0..5, every accepted byte; the session table
    behind a 1-byte base and per-record keys behind a 3-byte base."""
    for runs, base, sessions in ((False, 1, True), (True, 3, False)):
        w = make_world(931000 + n, n, runs)
        r = run_seal(enet, w, base=base, sessions=sessions)
        assert r["status"] == [OK] * n
        assert r["frames"] == [w.frame(i) for i in range(n)]
        assert_sentinels(r["edges"])


def test_seal_accepted_forms(enet, big):
    w, frames = big
    r = run_seal(enet, w, accepted="null", versions=False)  # send_negative_ack; NULL versions = 4
    w4 = dataclasses.replace(w, versions=[4] * w.n)
    assert r["frames"] == [w4.frame(i, accepted=[0] * w.n) for i in range(w.n)]
    r = run_seal(enet, w, base=3, accepted="zero")  # the table holds the inverse sense
    assert r["frames"] == frames and r["status"] == [OK] * w.n


def test_seal_order_subset(enet, big):
    w, frames = big
    order = [200, 3, 64, 65, 0, 256, 130, 7]
    r = run_seal(enet, w, base=3, order=order)
    for i in range(w.n):
        if i in order:
            assert r["frames"][i] == frames[i] and r["status"][i] == OK, i
        else:
            assert r["frames"][i] == bytes([SENT]) * len(frames[i]) and r["status"][i] == 0x77, i
    assert_sentinels(r["edges"])


def test_seal_failures(enet):
    """Wrong slot size by +-1, a session outside the table, kinds 0 / 1 / 3 / 5: the status, and the
    whole slot zeroed; the neighbours are sealed."""
    w = make_world(932000, 70)
    kinds, lens = list(w.kinds), [frame_len(k) for k in w.kinds]
    lens[3] += 1; lens[4] -= 1; lens[40] -= 1; lens[41] += 1
    w.sess[10] = SESSIONS; w.sess[65] = 0xFFFFFFFF
    for i, k in ((20, 0), (21, 1), (22, 3), (23, 5), (69, 255)):
        kinds[i] = k
    lens[22] = 116  # no kind, no length to fit: HEADER whatever the slot
    r = run_seal(enet, w, base=1, out_lens=lens, kinds=kinds)
    want = [seal_expect(kinds[i], w.key(i), w.fnonces[i], w.cids[i], w.local, bool(w.accepted[i]), w.versions[i], lens[i])
            for i in range(w.n)]
    assert r["status"] == [s for s, _ in want]
    assert {FRAME, HEADER, OK} == set(r["status"]) and r["status"].count(FRAME) == 6 and r["status"].count(HEADER) == 5
    assert r["frames"] == [f for _, f in want]
    assert_sentinels(r["edges"])


# ------------------------------------------------------------------ open
@pytest.mark.parametrize("base,sessions", [(1, True), (3, False)])
def test_open_round_trip(enet, big, base, sessions):
    """The sealed frames, with sender ids matching, differing and absent."""
    w, frames = big
    keys = [w.key(i) for i in range(w.n)]
    senders = [w.local if i % 3 else w.cids[i] for i in range(w.n)]
    r = run_open(enet, frames, w.table, w.sess, base=base, sessions=sessions, senders=senders)
    check_open(r, frames, keys, senders)
    assert r["status"] == [OK] * w.n and {x[3] for x in r["info"]} == {0, 1}
    r = run_open(enet, frames[:65], w.table, w.sess[:65], base=base, sessions=sessions, peers_out=False)
    check_open(r, frames[:65], keys)
    assert {x[3] for x in r["info"]} == {0}


def test_open_golden_negatives(enet):
    with open(os.path.join(ROOT, "tests", "golden", "control_frames.json")) as f:
        gold = json.load(f)
    vec = gold["mutations"] + gold["cases"]
    table = [bytes.fromhex(v["key"]) for v in vec]
    nonces = [splitmix_bytes(933000 + i, 12) for i in range(len(vec))]
    frames = [wire_of(nonces[i], oracle.chacha20_xor(table[i], nonces[i], bytes.fromhex(v["signed"]))) for i, v in enumerate(vec)]
    r = run_open(enet, frames, table, list(range(len(vec))), base=3)
    check_open(r, frames, table)
    for i, v in enumerate(vec):
        d = v["decoded"]
        fused = d["decodes"] and d.get("type") in (REQUEST, ACK) and len(frames[i]) == frame_len(d["type"])
        assert (r["status"][i] == OK) == fused, v["name"]
        if fused:
            assert (r["info"][i][0], r["info"][i][1], r["info"][i][2], r["cid"][i].hex(), r["pid"][i].hex()) == (
                d["version"], d["type"], d["accepted"], d["chunk_id"], d["peer_id"]), v["name"]
    assert {OK, FRAME, HEADER} == set(r["status"])


def test_open_damaged_and_short_frames(enet, big):
    """A flipped bit in each of nonce, length, body and MAC; frames of 47 and 48 bytes and other odd
    lengths (a valid MAC over a message of the wrong length is HEADER, a broken one FRAME); a
    session outside the table; failed records zeroed."""
    w, good = big
    frames, sess = [], []
    for i in range(40):
        f = bytearray(good[i])
        at = [0, 11, 12, 15, 16, 17, 16 + 63, 16 + 64, 16 + 66, len(f) - 32, len(f) - 1][i % 11]
        f[at] ^= 1 << (i % 8)
        frames.append(bytes(f)); sess.append(w.sess[i])
    k0 = w.table[0]
    for L in (0, 1, 15, 16, 47):
        frames.append(splitmix_bytes(934000 + L, L)); sess.append(0)
    for lm in (0, 1, 2, 30, 63, 64, 65, 68, 80, 81, 95, 96, 127, 128, 129, 200, 1000):  # the row holds 128 bytes
        m = bytes([4, REQUEST if lm % 2 else ACK]) + splitmix_bytes(934100 + lm, max(lm - 2, 0)) if lm >= 2 else bytes(lm)
        f = wire_frame(k0, splitmix_bytes(934200 + lm, 12), m)
        frames.append(f); sess.append(0)
        bad = bytearray(f); bad[-1 - (lm % 32)] ^= 0x80
        frames.append(bytes(bad)); sess.append(0)
    frames += good[40:50]; sess += [SESSIONS, 0xFFFFFFFF] + w.sess[42:50]
    keys = [w.table[s] if s < SESSIONS else None for s in sess]
    for base, sessions in ((1, True), (3, True), (2, False)):
        if not sessions:  # per-record keys: no session index to be wrong
            keys = [k if k is not None else bytes(32) for k in keys]
        r = run_open(enet, frames, w.table, sess, base=base, sessions=sessions, senders=[w.local] * len(frames))
        check_open(r, frames, keys, [w.local] * len(frames))
        assert {OK, FRAME, HEADER} == set(r["status"])


def test_open_order_subset(enet, big):
    w, frames = big
    order = [256, 0, 5, 64, 63, 129, 77]
    r = run_open(enet, frames, w.table, w.sess, base=3, order=order)
    check_open(r, frames, [w.key(i) for i in range(w.n)], named=set(order))


# ------------------------------------------------------------------ chunk open -> ack seal
@dataclasses.dataclass
class Chunks:
    frames: list
    ids: list
    ckeys: list
    cnonces: list
    hashes: list
    pts: list


def make_chunks(seed, skeys, lens, versions=None) -> Chunks:
    c = Chunks([], [], [], [], [], [])
    for i, L in enumerate(lens):
        pt, cid = splitmix_bytes(seed + 10 * i, L), splitmix_bytes(seed + 10 * i + 1, 32)
        ck, cn = splitmix_bytes(seed + 10 * i + 2, 32), splitmix_bytes(seed + 10 * i + 3, 12)
        m = chunk_message(versions[i] if versions else 4, 3600 + i, cid, stored_data(ck, cn, cid, pt))
        c.frames.append(wire_frame(skeys[i], splitmix_bytes(seed + 10 * i + 4, 12), m))
        c.ids.append(cid); c.ckeys.append(ck); c.cnonces.append(cn); c.hashes.append(oracle.sha256(pt)); c.pts.append(pt)
    return c


def chunk_expect(frame, key, cid, ck, cn, h):
    """enet_chunk_frame_open_batch's status for one frame: the general open, then decode's view."""
    m = open_message(frame, key)
    if m is None:
        return 1
    if len(m) < 42 or not 1 <= m[0] <= 4 or m[1] != 3 or int.from_bytes(m[6:10], "big") != len(m) - 42:
        return 2
    if m[10:42] != cid:
        return 3
    pt = oracle.chacha20_xor(ck, cn, m[42:], oracle.derive_counter(cid))
    return 0 if oracle.sha256(pt) == h else 4


def test_chunk_open_status_feeds_ack_seal(enet):
    """handle_chunk (Node.cpp:2286-2317) on the device: chunk_frame_open, then control_frame_seal with
    accepted = status and accept_zero on the same stream, no host read in between."""
    import torch
    n = 9
    w = make_world(935000, n)
    w.kinds = [ACK] * n
    skeys = [w.key(i) for i in range(n)]
    c = make_chunks(935500, skeys, [100, 0, 1, 1458, 64, 333, 7, 200, 50])
    f = bytearray(c.frames[1]); f[-1] ^= 1; c.frames[1] = bytes(f)                     # FRAME
    m = bytearray(chunk_message(4, 1, c.ids[3], b"x" * 10)); m[1] = 5
    c.frames[3] = wire_frame(skeys[3], bytes(12), bytes(m))                           # HEADER
    c.ids[5] = splitmix_bytes(935900, 32)                                              # CHUNK_ID
    c.hashes[7] = splitmix_bytes(935901, 32)                                           # HASH
    want = [chunk_expect(c.frames[i], skeys[i], c.ids[i], c.ckeys[i], c.cnonces[i], c.hashes[i]) for i in range(n)]
    assert want == [0, 1, 0, 2, 0, 3, 0, 4, 0]
    keys, stride, kw = keys_for(enet, w.table, w.sess, True)
    ioffs = offsets_for([len(x) for x in c.frames], 1)
    ooffs = offsets_for([max(len(x) - 90, 0) for x in c.frames], 0)
    rx = enet.Batch(arena=devb(bytes(1) + b"".join(c.frames)), offsets=dev(ioffs), keys=keys, nonces=None, key_stride=stride)
    pt = torch.zeros(int(ooffs[-1]) + 1, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    aoffs = offsets_for([115] * n, 3)
    acks = torch.full((int(aoffs[-1]) + 5,), SENT, dtype=torch.uint8, device="cuda")
    tx = enet.Batch(arena=None, offsets=dev(aoffs), keys=keys, nonces=devb(b"".join(w.fnonces)), key_stride=stride)
    st_seal = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    d_ids, d_local = devb(b"".join(c.ids)), devb(w.local)
    d_args = [devb(b"".join(x)) for x in (c.ids, c.ckeys, c.cnonces, c.hashes)]
    d_kinds = dev_u8(w.kinds)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        enet.chunk_frame_open(rx, pt, dev(ooffs), *d_args, status, stream=s, **kw)
        enet.control_frame_seal(tx, acks, tx.offsets, d_kinds, d_ids, d_local, st_seal, accepted=status, accept_zero=True,
                                stream=s, **kw)
    s.synchronize()
    assert status.cpu().tolist() == want and st_seal.cpu().tolist() == [OK] * n
    o = host(acks)
    got = records_of(o, aoffs.tolist())
    assert got == [control_frame(skeys[i], w.fnonces[i], ACK, c.ids[i], w.local, want[i] == 0, 4) for i in range(n)]
    assert_sentinels([o[:3], o[int(aoffs[-1]):]])


# ------------------------------------------------------------------ classify
def mixed_batch(seed):
    """-> (frames, sess, table, local, chunks-by-index): ~300 frames of every kind and defect."""
    table = [splitmix_bytes(seed + s, 32) for s in range(SESSIONS)]
    local = splitmix_bytes(seed + 9, 32)
    frames, sess, chunk_at = [], [], {}
    state = [0]

    def add(make, s=None):
        k = state[0]; state[0] += 1
        s = k % SESSIONS if s is None else s
        frames.append(make(table[s % SESSIONS], splitmix_bytes(seed + 1000 + k, 12), k)); sess.append(s)
        return len(frames) - 1

    def raw(m):
        return lambda key, nonce, k: wire_frame(key, nonce, m)

    def announce(v, cut=0, pad=0):
        a = Announce(chunk_id=splitmix_bytes(seed + 20 + v, 32), peer_id=local, endpoint=b"", uri=b"u" if pad else b"",
                     shards=b"", version=v, work_nonce=7)
        m = announce_message(a)
        if v == 3:  # encode writes no nonce for v3, decode wants one: the class minimum is 90
            m += bytes(8)
        return m[:len(m) - cut]

    # Chunk frames: data of 0, 1 and 1458 bytes, versions 1..4
    lens = [0, 1, 1458] * 14 + [1458] * 160
    skeys = [table[k % SESSIONS] for k in range(len(lens))]
    c = make_chunks(seed + 50000, skeys, lens, versions=[1 + k % 4 for k in range(len(lens))])
    for k in range(len(lens)):
        chunk_at[add(lambda key, nonce, _k, k=k: c.frames[k], s=k % SESSIONS)] = k
    for v in (1, 2, 3, 4):
        add(raw(announce(v)))               # |m| at the class minimum (no manifest: NO_MANIFEST from the open)
        add(raw(announce(v, cut=1)))        # one below
        add(raw(announce(v, pad=1)))        # admitted by the open
    add(raw(announce(4, pad=1) + b"\x00"))  # in the class by its length, HEADER from the open
    for k in range(40):
        kind = [REQUEST, ACK][k % 2]
        m = control_message(kind, splitmix_bytes(seed + 300 + k, 32), local, k % 3 == 0, 1 + k % 4)
        add(raw(m))
        if k < 8:
            add(raw(m[:-1])); add(raw(m + b"\x5a"))
        if k < 2:
            for t in (0, 5, 6, 0xFF):
                add(raw(m[:1] + bytes([t]) + m[2:]))
            for v in (0, 5):
                add(raw(bytes([v]) + m[1:]))
            add(lambda key, nonce, _k, m=m: (lambda f: f[:12] + (len(f) - 15).to_bytes(4, "big") + f[16:])(wire_frame(key, nonce, m)))
            add(raw(m), s=SESSIONS + k)     # a session outside the table
    for L in (0, 15, 16, 47):
        add(lambda key, nonce, k, L=L: splitmix_bytes(seed + 400 + L, L))
    for L in (48, 49, 50):
        add(lambda key, nonce, k, L=L: wire_of(nonce, splitmix_bytes(seed + 400 + L, L - 16)))
    # a fixed shuffle, so that every workgroup's block is mixed
    perm = sorted(range(len(frames)), key=lambda i: splitmix_bytes(seed + 7000 + i, 4))
    frames, sess = [frames[i] for i in perm], [sess[i] for i in perm]
    chunk_at = {perm.index(i): k for i, k in chunk_at.items()}
    return frames, sess, table, local, c, chunk_at


def test_classify_routes_a_mixed_batch(enet):
    import torch
    frames, sess, table, local, c, chunk_at = mixed_batch(936000)
    n = len(frames)
    assert 280 <= n <= 340
    keys = [table[s] if s < SESSIONS else None for s in sess]
    want = [classify(f, k) for f, k in zip(frames, keys)]
    assert set(want) == {0, 1, 2, 3, 4, 5}
    # the completeness property on the helper itself: whatever a fused open would accept is in its class
    for i, f in enumerate(frames):
        m = open_message(f, keys[i])
        if m is None:
            continue
        pc, pa = parse_control(m), parse_announce(m)
        if pc is not None and pc[1] == 0:
            assert want[i] == pc[0][1], i
        if pa is not None and pa[1] == 0:
            assert want[i] == 1, i
        if len(m) >= 42 and 1 <= m[0] <= 4 and m[1] == 3 and int.from_bytes(m[6:10], "big") == len(m) - 42:
            assert want[i] == 3, i
    base = 3
    ioffs = offsets_for([len(f) for f in frames], base)
    arena = devb(bytes([SENT]) * base + b"".join(frames) + bytes([SENT]) * 3)
    tbl, stride, kw = keys_for(enet, table, sess, True)
    b = enet.Batch(arena=arena, offsets=dev(ioffs), keys=tbl, nonces=None, key_stride=stride)
    rows = None
    for fill in (0, 0x7FFFFFF1):  # the call zeroes counts itself
        kind = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
        lists = torch.full((5, n), -1, dtype=torch.int32, device="cuda")
        counts = torch.full((5,), fill, dtype=torch.int32, device="cuda")
        enet.frame_classify(b, kind, lists, counts, session=kw["session"], sessions=SESSIONS)
        assert kind.cpu().tolist() == want
        cn, ls = counts.cpu().tolist(), lists.cpu().tolist()
        assert cn == [want.count(k) for k in range(1, 6)]
        rows = [ls[k][:cn[k]] for k in range(5)]
        for k in range(5):
            assert sorted(rows[k]) == [i for i in range(n) if want[i] == k + 1], k
            assert ls[k][cn[k]:] == [-1] * (n - cn[k])
            for blk in range(0, n, 256):  # ascending inside each workgroup's block
                part = [i for i in rows[k] if blk <= i < blk + 256]
                assert part == sorted(part)
    assert sum(len(r) for r in rows) == n - want.count(FK_BAD)

    def sub(k):
        return dataclasses.replace(b, order=lists[k], count=len(rows[k]))

    # row 1: the announce open
    ooffs = offsets_for([max(len(f) - OVERHEAD, 0) for f in frames], 0)
    d_ooffs = dev(ooffs)
    msgs = torch.zeros(int(ooffs[-1]) + 1, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    info = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    enet.announce_frame_open(sub(0), msgs, d_ooffs, devb(local * n), 0, info, st, **kw)
    got, out = st.cpu().tolist(), records_of(host(msgs), ooffs.tolist())
    for i in rows[0]:
        s_, m_, _ = admit(frames[i], keys[i], local, 0)
        assert got[i] == s_ and (s_ != 0 or out[i] == m_), i
    assert 0 in [got[i] for i in rows[0]] and 2 in [got[i] for i in rows[0]]
    # rows 2 and 4: the control open
    st = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    cid = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    pid = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    inf = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    for k in (1, 3):
        enet.control_frame_open(sub(k), cid, inf, st, peer_ids_out=pid, **kw)
    got, gc, gp, gi = st.cpu().tolist(), host(cid), host(pid), host(inf)
    for i in rows[1] + rows[3]:
        assert (got[i], gc[32 * i:32 * i + 32], gp[32 * i:32 * i + 32], gi[4 * i:4 * i + 4]) == open_expect(frames[i], keys[i]), i
    assert {got[i] for i in rows[1] + rows[3]} == {OK}  # exact lengths and valid MACs: all fast-path
    # row 3: the chunk open
    dummy = bytes(32)
    ids = [c.ids[chunk_at[i]] if i in chunk_at else dummy for i in range(n)]
    cks = [c.ckeys[chunk_at[i]] if i in chunk_at else dummy for i in range(n)]
    cns = [c.cnonces[chunk_at[i]] if i in chunk_at else dummy[:12] for i in range(n)]
    hs = [c.hashes[chunk_at[i]] if i in chunk_at else dummy for i in range(n)]
    poffs = offsets_for([max(len(f) - 90, 0) for f in frames], 0)
    pt = torch.zeros(int(poffs[-1]) + 1, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    enet.chunk_frame_open(sub(2), pt, dev(poffs), *[devb(b"".join(x)) for x in (ids, cks, cns, hs)], st, **kw)
    got, out = st.cpu().tolist(), records_of(host(pt), poffs.tolist())
    for i in rows[2]:
        assert got[i] == chunk_expect(frames[i], keys[i], ids[i], cks[i], cns[i], hs[i]), i
        if got[i] == 0:
            assert out[i] == c.pts[chunk_at[i]], i
    assert sorted(rows[2]) == sorted(chunk_at)
    # row 5: the general open
    macs = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    ok = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    msgs.zero_()
    enet.wire_open_sessions(sub(4), msgs, d_ooffs, kw["session"], SESSIONS, kw["mid"], macs, ok)
    got, out = ok.cpu().tolist(), records_of(host(msgs), ooffs.tolist())
    for i in rows[4]:
        m = open_message(frames[i], keys[i])
        assert got[i] == (1 if m is not None else 0) and (m is None or out[i] == m), i
    # nothing outside the rows was touched by any open
    for i in range(n):
        if want[i] == FK_BAD:
            assert got[i] == 0x77
            assert open_message(frames[i], keys[i]) is None  # what every open rejects as FRAME


# ------------------------------------------------------------------ arguments
def test_invalid_arguments_and_empty_batches(enet, big):
    import torch
    w, frames = big
    n = 8
    keys, stride, kw = keys_for(enet, w.table, w.sess[:n], True)
    ooffs = dev(offsets_for([frame_len(k) for k in w.kinds[:n]], 0))
    out = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    b = enet.Batch(arena=None, offsets=ooffs, keys=keys, nonces=devb(b"".join(w.fnonces[:n])), key_stride=stride)
    ids, st = torch.zeros(32 * n + 4, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")
    kinds, local = dev_u8(w.kinds[:n]), torch.zeros(36, dtype=torch.uint8, device="cuda")
    E = enet.EnetError
    for bad in (dict(kinds=None), dict(chunk_ids=None), dict(peer_id=None), dict(status=None), dict(chunk_ids=ids[1:]),
                dict(peer_id=local[2:])):
        a = dict(kinds=kinds, chunk_ids=ids, peer_id=local, status=st)
        a.update(bad)
        with pytest.raises(E):
            enet.control_frame_seal(b, out, ooffs, a["kinds"], a["chunk_ids"], a["peer_id"], a["status"], **kw)
    with pytest.raises(E):
        enet.control_frame_seal(b, out, ooffs, kinds, ids, local, st, session=kw["session"], sessions=0, mid=kw["mid"])
    rx = enet.Batch(arena=out, offsets=ooffs, keys=keys, nonces=None, key_stride=stride)
    info = torch.zeros(4 * n + 4, dtype=torch.uint8, device="cuda")
    for bad in (dict(cid=None), dict(info=None), dict(st=None), dict(cid=ids[2:]), dict(info=info[1:]), dict(pid=ids[3:]),
                dict(snd=ids[1:])):
        a = dict(cid=ids, info=info, st=st, pid=None, snd=None)
        a.update(bad)
        with pytest.raises(E):
            enet.control_frame_open(rx, a["cid"], a["info"], a["st"], peer_ids_out=a["pid"], sender_ids=a["snd"], **kw)
    lists, counts = torch.zeros(5 * n + 1, dtype=torch.int32, device="cuda"), torch.zeros(6, dtype=torch.int32, device="cuda")
    l8, c8 = lists.view(torch.uint8), counts.view(torch.uint8)
    for bad in (dict(kind=None), dict(lists=None), dict(counts=None), dict(lists=l8[2:]), dict(counts=c8[1:])):
        a = dict(kind=st, lists=lists, counts=counts)
        a.update(bad)
        with pytest.raises(E):
            enet.frame_classify(rx, a["kind"], a["lists"], a["counts"], session=kw["session"], sessions=SESSIONS)
    # nothing was launched by any of these; count == 0 is a no-op
    assert host(out) == bytes(1024) and host(st) == bytes(n)
    counts.fill_(5)
    e = dataclasses.replace(rx, count=0)
    enet.control_frame_seal(dataclasses.replace(b, count=0), None, None, None, None, None, None)
    enet.control_frame_open(e, None, None, None)
    enet.frame_classify(e, None, None, None)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == [5] * 6
