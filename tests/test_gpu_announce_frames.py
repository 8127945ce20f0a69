"""GPU parity of the announce frames (announce_frames.hip, enet_announce_frame_seal_batch /
enet_announce_frame_open_batch) against the CPU oracle through tests/announce_frame_ref.py: the
gossip send -- proof-of-work search, Announce message and session wire frame gathered from shared
manifest / endpoint tables (Node::deliver_manifest, Node.cpp:2512-2661; compute_announce_pow,
:212-230) -- and the receive side -- frame open, header parse, sender, manifest and proof-of-work
checks in one pass (handle_announce, Node.cpp:2332-2357; verify_announce_pow, :1144-1151).
Expected bytes: oracle.frame_seal over the helper's message, oracle.pow_search / pow_check over
oracle.announce_pow_prefix.  Bit-exact throughout."""
import dataclasses

import numpy as np
import pytest

import handshake_ref as H
import oracle
from announce_frame_ref import (FIXED, FRAME, HEADER, NO_MANIFEST, NODE_POW_ATTEMPTS, OK, OVERHEAD, POW, SENDER, Announce,
                                admit, announce_message, clamp_version, parse_announce, seal_expect, wire_frame)
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

SENT = 0xAA
SESSIONS = 5
EDGE = (0, 1, 55, 56, 57, 63)           # residues mod 64 around SHA-256's padding boundary
GOLDEN_URI = 354                         # the default 3-of-5 manifest's URI (tests/golden/announce_frames.json)
URI_LENS = [1, 2, 3, 37, 62, 64, 65, GOLDEN_URI, 1290, 256 << 10, 0]
EP_LENS = [0, 1, 2, 3, 14, 21, 22, 23]


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


def dev_u32(vals):
    return dev(np.array(vals, dtype=np.uint32).view(np.int32))


def host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def offsets_for(lens, base):
    return np.concatenate([[base], base + np.cumsum(lens)]).astype(np.int64)


def records_of(arena: bytes, offs):
    return [arena[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


def arena_of(items, base):
    """(device arena with `base` sentinel bytes in front, device offsets)"""
    offs = offsets_for([len(x) for x in items], base)
    return devb(bytes([SENT]) * base + b"".join(items) + bytes([SENT]) * 3), dev(offs)


@dataclasses.dataclass
class World:
    """n announces over M shared manifests and Ep shared endpoints, the local id, the session keys."""
    n: int
    cids: list      # [M]
    uris: list      # [M]
    eps: list       # [Ep]
    midx: list      # [n]
    eidx: list      # [n]
    shards: list    # [n]
    ttl: list
    versions: list  # as given: 0..5
    local: bytes
    table: list
    sess: list
    fnonces: list

    def announce(self, i, **kw) -> Announce:
        a = Announce(chunk_id=self.cids[self.midx[i]], peer_id=self.local, endpoint=self.eps[self.eidx[i]],
                     uri=self.uris[self.midx[i]], shards=self.shards[i], ttl=self.ttl[i], version=self.versions[i])
        return dataclasses.replace(a, **kw)

    def key(self, i) -> bytes:
        return self.table[self.sess[i]]

    @property
    def skeys(self):
        return [self.table[s] for s in self.sess]


def finish_world(seed, cids, uris, eps, midx, eidx, alens) -> World:
    n = len(midx)
    return World(n=n, cids=cids, uris=uris, eps=eps, midx=midx, eidx=eidx,
                 shards=[splitmix_bytes(seed + 1000 + i, A) for i, A in enumerate(alens)],
                 ttl=[[3600, 0, 1, 0xFFFFFFFF][i % 4] for i in range(n)],
                 versions=[[4, 4, 0, 4, 1, 4, 2, 4, 3, 4, 5][i % 11] for i in range(n)],
                 local=splitmix_bytes(seed + 1, 32), table=[splitmix_bytes(seed + 10 + s, 32) for s in range(SESSIONS)],
                 sess=[int(x) % SESSIONS for x in splitmix_bytes(seed + 2, n)],
                 fnonces=[splitmix_bytes(seed + 5000 + i, 12) for i in range(n)])


def shared_world(seed) -> World:
    """~190 records over 11 manifests and 8 endpoints.  F = E + U + A runs over every residue mod 64
    that puts |m| = 90 + F or the PoW message's 120 + F on a padding edge, in three 64-byte rows
    (so |m| crosses 127..129 and 255..257), five times over with the endpoint, manifest and version
    rotating; then the realistic, the MTU-sized and the 256 KiB records."""
    cids = [splitmix_bytes(seed + 100 + k, 32) for k in range(len(URI_LENS))]
    uris = [splitmix_bytes(seed + 200 + k, U) for k, U in enumerate(URI_LENS)]
    eps = [splitmix_bytes(seed + 300 + k, E) for k, E in enumerate(EP_LENS)]
    res = sorted({(r - 90) % 64 for r in EDGE} | {(r - 120) % 64 for r in EDGE})
    midx, eidx, alens = [], [], []
    i = 0
    for rep in range(5):
        for row in range(3):
            for r in res:
                F = r + 64 * row
                ei = (i + rep) % len(EP_LENS)
                fit = [k for k, U in enumerate(URI_LENS) if 0 < U and EP_LENS[ei] + U <= F]
                if fit:
                    mi = fit[(i // 3 + rep) % len(fit)]
                else:
                    mi, ei = len(URI_LENS) - 1, 0  # no room for a URI: the empty one
                midx.append(mi); eidx.append(ei); alens.append(F - EP_LENS[ei] - URI_LENS[mi])
                i += 1
    for mi, ei, A in [(7, 5, 5), (7, 0, 0), (8, 4, 6), (9, 5, 3)]:  # realistic (twice), |m| = 1400, long
        midx.append(mi); eidx.append(ei); alens.append(A)
    w = finish_world(seed, cids, uris, eps, midx, eidx, alens)
    w.versions[-4:] = [4] * 4
    return w


def plain_world(seed, n=70) -> World:
    """Record i has manifest i and endpoint i (the NULL-index form), small fields."""
    ulens = [[37, 1, 64, GOLDEN_URI, 100][i % 5] + i % 3 for i in range(n)]
    elens = [EP_LENS[i % len(EP_LENS)] for i in range(n)]
    return finish_world(seed, [splitmix_bytes(seed + 100 + k, 32) for k in range(n)],
                        [splitmix_bytes(seed + 200 + k, U) for k, U in enumerate(ulens)],
                        [splitmix_bytes(seed + 400 + k, E) for k, E in enumerate(elens)],
                        list(range(n)), list(range(n)), [(7 * i) % 23 for i in range(n)])


class Expect:
    """The helper's verdicts for a world, computed once per (difficulty, attempts) and shared."""

    def __init__(self, w: World):
        self.w, self.memo = w, {}

    def sealed(self, difficulty, max_attempts=NODE_POW_ATTEMPTS):
        k = (difficulty, max_attempts)
        if k not in self.memo:
            w = self.w
            self.memo[k] = [seal_expect(w.announce(i), w.key(i), w.fnonces[i], difficulty, max_attempts)
                            for i in range(w.n)]
        return self.memo[k]


@pytest.fixture(scope="module")
def shared():
    w = shared_world(910000)
    return w, Expect(w)


@pytest.fixture(scope="module")
def plain():
    w = plain_world(920000)
    return w, Expect(w)


def session_args(enet, w, sess=None):
    import torch
    tbl = devb(b"".join(w.table))
    mid = torch.zeros(16 * SESSIONS, dtype=torch.int32, device="cuda")
    enet.hmac_midstates(tbl, SESSIONS, mid)
    return tbl, dict(session=dev_u32(w.sess if sess is None else sess), sessions=SESSIONS, mid=mid)


def key_batch(enet, w, items, base, sessions, sess, **batch_kw):
    b = enet.make_batch(items, w.skeys, w.fnonces, base_offset=base)
    kw = {}
    if sessions:
        tbl, kw = session_args(enet, w, sess)
        b = dataclasses.replace(b, keys=tbl)
    return dataclasses.replace(b, **batch_kw), kw


def run_seal(enet, w, difficulty, base=0, sessions=True, sess=None, max_attempts=NODE_POW_ATTEMPTS, given=None,
             out_lens=None, midx=None, eidx=None, null_index=False, **batch_kw):
    """-> dict(frames, status, nonce, edges)"""
    import torch
    b, kw = key_batch(enet, w, [b""] * w.n, 0, sessions, sess, **batch_kw)
    b = dataclasses.replace(b, arena=None)  # seal reads no input arena
    lens = out_lens or [len(announce_message(w.announce(i))) + OVERHEAD for i in range(w.n)]
    ooffs = offsets_for(lens, base + 1)
    out = torch.full((int(ooffs[-1]) + 7,), SENT, dtype=torch.uint8, device="cuda")
    uris, uoff = arena_of(w.uris, base)
    eps, eoff = arena_of(w.eps, base + 2)
    shards, soff = arena_of(w.shards, base + 1)
    f = enet.AnnounceFields(chunk_ids=devb(b"".join(w.cids)), uris=uris, uri_offsets=uoff, endpoint_bytes=eps,
                            endpoint_offsets=eoff, shards=shards, shard_offsets=soff,
                            peer_id=devb(bytes(base) + w.local)[base:], ttl=dev_u32(w.ttl),
                            manifest=None if null_index else dev_u32(w.midx if midx is None else midx),
                            endpoint=None if null_index else dev_u32(w.eidx if eidx is None else eidx),
                            versions=dev(np.array(w.versions, dtype=np.uint8)))
    nonce = dev(np.array(given if given is not None else [0x5A5A5A5A5A5A5A5A] * w.n, dtype=np.uint64).view(np.int64))
    status = torch.full((w.n,), 0x77, dtype=torch.uint8, device="cuda")
    enet.announce_frame_seal(b, out, dev(ooffs), f, difficulty, nonce, status, max_attempts=max_attempts, **kw)
    o = host(out)
    return dict(frames=records_of(o, ooffs.tolist()), status=status.cpu().tolist(),
                nonce=nonce.cpu().numpy().view(np.uint64).tolist(), edges=[o[:base + 1], o[int(ooffs[-1]):]])


def run_open(enet, w, frames, difficulty, base=0, sessions=True, sess=None, peers=None, out_lens=None, **batch_kw):
    """-> dict(out, status, info, edges)"""
    import torch
    b, kw = key_batch(enet, w, frames, base, sessions, sess, **batch_kw)
    b = dataclasses.replace(b, nonces=None)
    ooffs = offsets_for(out_lens or [max(len(f) - OVERHEAD, 0) for f in frames], base + 2)
    out = torch.full((int(ooffs[-1]) + 9,), SENT, dtype=torch.uint8, device="cuda")
    n = len(frames)
    status = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    info = torch.full((n, 8), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    enet.announce_frame_open(b, out, dev(ooffs), devb(b"".join(peers or [w.local] * n)), difficulty, info, status, **kw)
    o, offs = host(out), ooffs.tolist()
    return dict(out=records_of(o, offs), status=status.cpu().tolist(),
                info=info.cpu().numpy().view(np.uint32).tolist(), edges=[o[:offs[0]], o[offs[-1]:]])


def assert_sentinels(edges):
    for e in edges:
        assert e == bytes([SENT]) * len(e)


def check_open(w, r, frames, difficulty, peers=None, keys=None):
    """Every record against the helper's admission: status, message and info, zero on failure."""
    for i, f in enumerate(frames):
        st, m, info = admit(f, keys[i] if keys else w.key(i), (peers or [w.local] * len(frames))[i], difficulty)
        assert r["status"][i] == st, (i, r["status"][i], st)
        if st == OK:
            assert r["out"][i] == m and r["info"][i] == info, i
        else:
            assert r["out"][i] == bytes(len(r["out"][i])) and r["info"][i] == [0] * 8, i


def test_shapes_cover_the_edges(shared):
    """The shapes the other tests run (no GPU work): see shared_world."""
    w, _ = shared
    assert w.n >= 180 and w.n % 64 != 0 and max(w.midx) < len(w.uris) < w.n and max(w.eidx) < len(w.eps) < w.n
    v4 = [i for i in range(w.n) if clamp_version(w.versions[i]) == 4]
    F = {i: w.announce(i).flen for i in range(w.n)}
    E = {i: len(w.eps[w.eidx[i]]) for i in range(w.n)}
    U = {i: len(w.uris[w.midx[i]]) for i in range(w.n)}
    assert {(90 + F[i]) % 64 for i in v4} >= set(EDGE)
    assert {(120 + F[i]) % 64 for i in v4} >= set(EDGE)
    assert {90 + F[i] for i in v4} >= {127, 128, 129, 255, 256, 257}
    for pos in (E, {i: E[i] + U[i] for i in F}, F):
        assert {pos[i] % 4 for i in v4} == {0, 1, 2, 3}
    assert any(E[i] == 0 for i in v4) and any(F[i] - E[i] - U[i] == 0 for i in v4)
    assert any(U[i] == GOLDEN_URI for i in v4) and any(90 + F[i] == 1400 for i in v4) and any(U[i] == 256 << 10 for i in v4)
    assert sorted(set(w.versions)) == [0, 1, 2, 3, 4, 5] and set(w.ttl) == {0, 1, 3600, 0xFFFFFFFF}


@pytest.mark.parametrize("difficulty,sessions,base", [(0, True, 0), (1, False, 3), (6, True, 5), (10, False, 1)])
def test_seal_and_open_match_helper(enet, shared, difficulty, sessions, base):
    """One mixed batch over every length class (several 64-record workgroups, a partial last one, a
    256 KiB URI among short neighbours), shared manifests and endpoints through the index tables,
    arenas at odd byte offsets, versions 0..5, session table and per-record keys: the seal gives the
    helper's frame byte for byte and the oracle's first-found nonce; the open of those frames gives
    the helper's verdict (v3 frames as encode writes them never decode; v1 / v2 fail the proof of
    work at difficulty > 0; an empty URI is no manifest), message and parsed fields; nothing outside
    the records' ranges is written."""
    w, ex = shared
    want = ex.sealed(difficulty)
    assert all(st == OK for st, _, _ in want)
    r = run_seal(enet, w, difficulty, base, sessions)
    assert r["status"] == [0] * w.n
    for i, (_, frame, nonce) in enumerate(want):
        assert r["nonce"][i] == nonce, (i, w.versions[i])
        assert r["frames"][i] == frame, (i, len(frame))
    assert_sentinels(r["edges"])
    frames = [f for _, f, _ in want]
    o = run_open(enet, w, frames, difficulty, base, sessions)
    check_open(w, o, frames, difficulty)
    assert_sentinels(o["edges"])
    seen = set(o["status"])
    assert seen == ({OK, HEADER, NO_MANIFEST} if difficulty == 0 else {OK, HEADER, NO_MANIFEST, POW})


def test_null_index_form(enet, plain):
    """manifest == endpoint == NULL: record i takes manifest i and endpoint i."""
    w, ex = plain
    want = ex.sealed(6)
    r = run_seal(enet, w, 6, 2, null_index=True)
    assert r["status"] == [0] * w.n and r["nonce"] == [x[2] for x in want]
    assert r["frames"] == [x[1] for x in want]
    assert_sentinels(r["edges"])


def test_search_policy(enet, plain):
    """Nothing found within max_attempts = 3 at difficulty 16 (the oracle finds nothing either):
    ENET_AF_POW, a zeroed slot and nonce 0 for the v4 records, the v < 4 records sealed without a
    nonce.  max_attempts = 0 passes the caller's nonces through, whatever the difficulty."""
    w, ex = plain
    want = ex.sealed(16, 3)
    v4 = [clamp_version(v) == 4 for v in w.versions]
    assert [st for st, _, _ in want] == [POW if x else OK for x in v4]
    r = run_seal(enet, w, 16, 1, max_attempts=3)
    assert r["status"] == [st for st, _, _ in want]
    assert r["nonce"] == [0] * w.n
    for i, (st, frame, _) in enumerate(want):
        assert r["frames"][i] == (frame if st == OK else bytes(len(r["frames"][i]))), i
    assert_sentinels(r["edges"])
    given = [int.from_bytes(splitmix_bytes(930000 + i, 8), "little") for i in range(w.n)]
    for difficulty in (0, 10):
        r = run_seal(enet, w, difficulty, 0, sessions=False, max_attempts=0, given=given)
        assert r["status"] == [0] * w.n
        assert r["nonce"] == [g if x else 0 for g, x in zip(given, v4)]
        for i in range(w.n):
            assert r["frames"][i] == seal_expect(w.announce(i), w.key(i), w.fnonces[i], difficulty, 0, given[i])[1], i


def test_seal_bad_slots_fail_closed(enet, plain):
    """A slot one byte too long or too short, a manifest / endpoint index at and past its table, a
    session index at the table's size: ENET_AF_FRAME, the whole slot zero, nonce 0; the others are
    sealed; the sentinels around every range survive."""
    w, ex = plain
    want = ex.sealed(6)
    lens = [len(f) for _, f, _ in want]
    midx, eidx, sess = list(w.midx), list(w.eidx), list(w.sess)
    lens[3] += 1; lens[10] -= 1
    midx[17] = w.n; midx[24] = 0xFFFFFFFF
    eidx[31] = w.n; eidx[38] = 0x80000000
    sess[45] = SESSIONS
    bad = {3, 10, 17, 24, 31, 38, 45}
    r = run_seal(enet, w, 6, 3, sess=sess, out_lens=lens, midx=midx, eidx=eidx)
    for i, (_, frame, nonce) in enumerate(want):
        if i in bad:
            assert r["status"][i] == FRAME and r["frames"][i] == bytes(lens[i]) and r["nonce"][i] == 0, i
        else:
            assert r["status"][i] == OK and r["frames"][i] == frame and r["nonce"][i] == nonce, i
    assert_sentinels(r["edges"])


def test_every_open_status_fails_closed(enet):
    """One batch at difficulty 10, one offending record per case, each with exactly its status, a
    zeroed message and zeroed info; first-failure precedence where two checks fail; every other
    record status 0 with its bytes.  The same frames at difficulty 0 accept the wrong nonces."""
    w = plain_world(940000, 84)
    w.versions = [4] * w.n
    difficulty = 10
    anns = []
    for i in range(w.n):
        a = w.announce(i)
        found, nonce = True, 0
        if i % 2 == 0:  # the odd records carry nonce 0: no proof
            found, nonce, _ = oracle.pow_search(a.prefix(), difficulty, 0, NODE_POW_ATTEMPTS)
        assert found
        anns.append(dataclasses.replace(a, work_nonce=nonce))
    frames = [wire_frame(w.key(i), w.fnonces[i], announce_message(a)) for i, a in enumerate(anns)]
    peers, sess = [w.local] * w.n, list(w.sess)
    want = {i: POW for i in range(1, w.n, 2) if not oracle.pow_check(anns[i].prefix(), 0, difficulty)}
    flip = lambda b, at, bit=1: b[:at] + bytes([b[at] ^ bit]) + b[at + 1:]

    def resign(i, m, status):  # altered bytes under the record's own key and nonce: they authenticate
        frames[i] = wire_frame(w.key(i), w.fnonces[i], m)
        want[i] = status

    m = lambda i, **kw: announce_message(dataclasses.replace(anns[i], **kw))
    # FRAME
    frames[0] = flip(frames[0], len(frames[0]) - 1, 0x80); want[0] = FRAME     # a MAC bit
    frames[2] = flip(frames[2], 16 + 20); want[2] = FRAME                      # a body byte
    frames[4] = flip(frames[4], 15); want[4] = FRAME                           # the length field
    frames[6] = splitmix_bytes(7, 47); want[6] = FRAME                         # shorter than header + MAC
    sess[8] = SESSIONS; want[8] = FRAME                                        # the first index past the table
    # HEADER
    resign(10, m(10)[:1] + b"\x02" + m(10)[2:], HEADER)                        # wrong type
    resign(12, announce_message(dataclasses.replace(anns[12], version=3)), HEADER)  # v3 as encode writes it
    resign(14, m(14) + b"\x00", HEADER)                                        # a trailing byte
    resign(16, b"\x00" + m(16)[1:], HEADER)
    resign(18, b"\x05" + m(18)[1:], HEADER)
    resign(20, m(20)[:81], HEADER)                                             # 81 bytes
    resign(22, m(22)[:9] + bytes([m(22)[9] ^ 1]) + m(22)[10:], HEADER)         # E off by one
    resign(24, m(24)[:10] + b"\xff\xff\xff\xff" + m(24)[14:], HEADER)          # U = 2^32 - 1: the 64-bit sum
    # SENDER
    peers[26] = flip(w.local, 31); want[26] = SENDER
    resign(28, m(28, peer_id=splitmix_bytes(9, 32)), SENDER)
    # NO_MANIFEST
    a30 = dataclasses.replace(anns[30], uri=b"")
    _, n30, _ = oracle.pow_search(a30.prefix(), difficulty, 0, NODE_POW_ATTEMPTS)
    resign(30, announce_message(dataclasses.replace(a30, work_nonce=n30)), NO_MANIFEST)
    # POW
    for i, delta in ((32, 1), (34, -1)):                                       # the nonce off by one
        wrong = dataclasses.replace(anns[i], work_nonce=(anns[i].work_nonce + delta) % 2**64)
        if not oracle.pow_check(wrong.prefix(), wrong.work_nonce, difficulty):
            resign(i, announce_message(wrong), POW)
    resign(36, announce_message(dataclasses.replace(anns[36], version=2)), POW)  # v2 carries no nonce
    resign(38, announce_message(dataclasses.replace(anns[38], version=1)), POW)
    v3 = announce_message(dataclasses.replace(anns[40], version=3), raw_version=True)  # v3 with its nonce decodes
    resign(40, v3 + anns[40].work_nonce.to_bytes(8, "big"), OK)
    del want[40]
    # precedence: the first failed check in the reference's order
    frames[42] = flip(wire_frame(w.key(42), w.fnonces[42], m(42)[:1] + b"\x09" + m(42)[2:]), 16); want[42] = FRAME
    resign(44, m(44, peer_id=bytes(32))[:1] + b"\x03" + m(44, peer_id=bytes(32))[2:], HEADER)   # type and sender
    resign(46, m(46, peer_id=bytes(32), uri=b""), SENDER)                       # sender, manifest and proof
    resign(48, m(48, uri=b"", work_nonce=anns[48].work_nonce ^ 1), NO_MANIFEST)  # manifest and proof
    resign(50, m(50, version=2, peer_id=bytes(32)), SENDER)                     # sender and v2
    assert set(want.values()) == {FRAME, HEADER, SENDER, NO_MANIFEST, POW}
    assert sum(1 for i in (32, 34) if want.get(i) == POW) >= 1
    out_lens = [max(len(f) - OVERHEAD, 0) for f in frames]

    r = run_open(enet, w, frames, difficulty, 3, sess=sess, peers=peers, out_lens=out_lens)
    assert r["status"] == [want.get(i, OK) for i in range(w.n)]
    keys = [w.table[s] if s < SESSIONS else bytes(32) for s in sess]
    check_open(w, r, frames, difficulty, peers=peers, keys=keys)
    assert r["info"][40][0] == 3 and r["info"][40][5] | (r["info"][40][6] << 32) == anns[40].work_nonce
    assert_sentinels(r["edges"])
    # difficulty 0: no proof is asked for
    r0 = run_open(enet, w, frames, 0, 0, sess=sess, peers=peers, out_lens=out_lens)
    assert r0["status"] == [0 if want.get(i, OK) == POW else want.get(i, OK) for i in range(w.n)]
    check_open(w, r0, frames, 0, peers=peers, keys=keys)


def test_agrees_with_three_call_path(enet, plain):
    """The same frames through wire_open_sessions, a host parse and prefix build, then pow_check:
    the same messages and the same verdicts, also for a tampered frame, a wrong nonce and a v2
    announce.  The fused seal equals pow_search + wire_seal_sessions over the assembled messages."""
    import torch
    w, ex = plain
    difficulty, n = 6, w.n
    want = ex.sealed(difficulty)
    frames = [f for _, f, _ in want]
    frames[5] = frames[5][:40] + bytes([frames[5][40] ^ 4]) + frames[5][41:]
    a9 = dataclasses.replace(w.announce(9), work_nonce=want[9][2])
    assert clamp_version(a9.version) == 4
    k = 1
    while oracle.pow_check(a9.prefix(), a9.work_nonce ^ k, difficulty):
        k += 1
    frames[9] = wire_frame(w.key(9), w.fnonces[9], announce_message(dataclasses.replace(a9, work_nonce=a9.work_nonce ^ k)))
    fused = run_open(enet, w, frames, difficulty, 0)
    # three calls
    tbl, kw = session_args(enet, w)
    b = dataclasses.replace(enet.make_batch(frames, w.skeys, w.fnonces), keys=tbl, nonces=None)
    moffs = offsets_for([len(f) - 48 for f in frames], 0)
    msgs = torch.zeros(int(moffs[-1]) + 1, dtype=torch.uint8, device="cuda")
    macs = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    ok_w = torch.zeros(n, dtype=torch.uint8, device="cuda")
    enet.wire_open_sessions(b, msgs, dev(moffs), kw["session"], SESSIONS, kw["mid"], macs, ok_w)
    opened = records_of(host(msgs), moffs.tolist())
    parsed = [parse_announce(m) if ok else None for m, ok in zip(opened, ok_w.cpu().tolist())]
    pre = [p[0].prefix() if p else b"" for p in parsed]
    poffs = offsets_for([len(x) for x in pre], 0)
    ok_p = torch.zeros(n, dtype=torch.uint8, device="cuda")
    enet.pow_check(devb(b"".join(pre) + b"\0"), dev(poffs),
                   dev(np.array([p[0].work_nonce if p else 0 for p in parsed], dtype=np.uint64).view(np.int64)),
                   dev(np.full(n, difficulty, dtype=np.uint8)), ok_p)
    three, okp = [], ok_p.cpu().tolist()
    for i, p in enumerate(parsed):
        good = p is not None and p[1] == 0 and p[0].peer_id == w.local and len(p[0].uri) > 0
        three.append(bool(good and p[0].version >= 3 and okp[i]))
    assert [s == OK for s in fused["status"]] == three
    assert fused["status"][5] == FRAME and fused["status"][9] == POW
    assert any(three) and not all(three)
    for i in range(n):
        assert fused["out"][i] == (opened[i] if three[i] else bytes(len(opened[i]))), i
    # seal: pow_search over host-built prefixes, then wire_seal_sessions over host-built messages
    anns = [w.announce(i) for i in range(n)]
    pre = [a.prefix() for a in anns]
    nonces = torch.zeros(n, dtype=torch.int64, device="cuda")
    found = torch.zeros(n, dtype=torch.uint8, device="cuda")
    enet.pow_search(devb(b"".join(pre)), dev(offsets_for([len(x) for x in pre], 0)),
                    dev(np.full(n, difficulty, dtype=np.uint8)), enet.POW_NODE, NODE_POW_ATTEMPTS, nonces, found)
    got = nonces.cpu().numpy().view(np.uint64).tolist()
    ms = [announce_message(dataclasses.replace(a, work_nonce=got[i])) for i, a in enumerate(anns)]
    mb = dataclasses.replace(enet.make_batch(ms, w.skeys, w.fnonces), keys=tbl)
    foffs = offsets_for([len(m) + 48 for m in ms], 0)
    out = torch.zeros(int(foffs[-1]), dtype=torch.uint8, device="cuda")
    enet.wire_seal_sessions(mb, out, dev(foffs), kw["session"], SESSIONS, kw["mid"])
    r = run_seal(enet, w, difficulty, 0)
    assert found.cpu().tolist() == [1] * n and r["frames"] == records_of(host(out), foffs.tolist())


def test_order_and_hints(enet, shared):
    """A longest-first permutation and a subset `order` that names indices >= count give the bytes
    of the unordered call (records the subset does not name keep their sentinels); true, absent and
    lying hints (total = count * max on a mixed batch, i.e. "uniform") change nothing."""
    w, ex = shared
    difficulty, n = 6, w.n
    want = ex.sealed(difficulty)
    frames = [f for _, f, _ in want]
    by_len = np.argsort([-len(f) for f in frames], kind="stable").astype(np.int32)
    r = run_seal(enet, w, difficulty, 3, order=dev(by_len))
    assert r["frames"] == frames and r["nonce"] == [x[2] for x in want]
    o = run_open(enet, w, frames, difficulty, 3, order=dev(by_len))
    check_open(w, o, frames, difficulty)
    sub = np.arange(1, n, 3, dtype=np.int32)[::-1].copy()
    named = set(sub.tolist())
    assert max(named) >= len(sub)
    r = run_seal(enet, w, difficulty, 1, order=dev(sub), count=len(sub))
    o = run_open(enet, w, frames, difficulty, 1, order=dev(sub), count=len(sub))
    for i in range(n):
        if i in named:
            assert r["frames"][i] == frames[i] and r["nonce"][i] == want[i][2] and r["status"][i] == 0, i
            assert o["status"][i] == admit(frames[i], w.key(i), w.local, difficulty)[0], i
        else:
            assert r["frames"][i] == bytes([SENT]) * len(frames[i]) and r["status"][i] == 0x77, i
            assert r["nonce"][i] == 0x5A5A5A5A5A5A5A5A, i
            assert o["status"][i] == 0x77 and o["info"][i] == [0x5A5A5A5A] * 8, i
            assert o["out"][i] == bytes([SENT]) * len(o["out"][i]), i
    assert_sentinels(r["edges"] + o["edges"])
    mx = max(len(f) for f in frames)
    for hints in (dict(max_len_hint=mx, total_bytes_hint=sum(len(f) for f in frames)),
                  dict(max_len_hint=0, total_bytes_hint=0), dict(max_len_hint=mx, total_bytes_hint=n * mx),
                  dict(max_len_hint=64, total_bytes_hint=64 * n)):
        o = run_open(enet, w, frames, difficulty, 0, **hints)
        check_open(w, o, frames, difficulty)
        r = run_seal(enet, w, difficulty, 0, **hints)
        assert r["frames"] == frames


def test_one_stream_after_handshake(enet, plain):
    """handshake_accept -> announce_frame_seal -> announce_frame_open on one stream with no
    synchronisation in between: the session keys go from the handshake into the table and from
    there into both calls without leaving the device.  The frames are the helper's under the
    restatement's keys; they open with status 0."""
    import torch
    w, _ = plain
    n, S, difficulty = w.n, 16, 6
    local_private = 0x5EED1234
    local_public = H.compute_public(local_private)
    reqs = []
    for k in range(S):
        peer = splitmix_bytes(950000 + k, 32)
        pub = H.compute_public(int.from_bytes(splitmix_bytes(950100 + k, 4), "little"))
        assert H.validate_public(pub)
        reqs.append((peer, pub))
    keys = [H.accept(p, pub, 0, k, S, w.local, local_private, local_public, 0)[2] for k, (p, pub) in enumerate(reqs)]
    sess = [(3 * i) % S for i in range(n)]
    want = [seal_expect(w.announce(i), keys[sess[i]], w.fnonces[i], difficulty) for i in range(n)]
    frames = [f for _, f, _ in want]
    table = enet.SessionTable.empty(S)
    verdict = torch.zeros(S, dtype=torch.uint8, device="cuda")
    d_pubs = dev_u32([r[1] for r in reqs])
    d_lid = devb(w.local)
    b = dataclasses.replace(enet.make_batch([b""] * n, [bytes(32)] * n, w.fnonces), keys=table.keys, arena=None)
    foffs = dev(offsets_for([len(f) for f in frames], 0))
    moffs = dev(offsets_for([len(f) - OVERHEAD for f in frames], 0))
    out = torch.zeros(sum(len(f) for f in frames), dtype=torch.uint8, device="cuda")
    msgs = torch.zeros(sum(len(f) - OVERHEAD for f in frames), dtype=torch.uint8, device="cuda")
    uris, uoff = arena_of(w.uris, 1)
    eps, eoff = arena_of(w.eps, 0)
    shards, soff = arena_of(w.shards, 3)
    f = enet.AnnounceFields(chunk_ids=devb(b"".join(w.cids)), uris=uris, uri_offsets=uoff, endpoint_bytes=eps,
                            endpoint_offsets=eoff, shards=shards, shard_offsets=soff, peer_id=d_lid, ttl=dev_u32(w.ttl),
                            versions=dev(np.array(w.versions, dtype=np.uint8)))
    nonce = torch.zeros(n, dtype=torch.int64, device="cuda")
    st_seal = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    st_open = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    info = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    d_sess, d_peers = dev_u32(sess), devb(w.local * n)
    bo = dataclasses.replace(b, arena=out, offsets=foffs, nonces=None)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        enet.handshake_accept(table, None, d_pubs, None, None, d_lid, local_private, local_public, 0, 5_000_000_000,
                              verdict, stream=s)
        enet.announce_frame_seal(b, out, foffs, f, difficulty, nonce, st_seal, session=d_sess, sessions=S,
                                 mid=table.mid, stream=s)
        enet.announce_frame_open(bo, msgs, moffs, d_peers, difficulty, info, st_open, session=d_sess, sessions=S,
                                 mid=table.mid, stream=s)
    s.synchronize()
    assert verdict.cpu().tolist() == [H.HS_OK] * S
    assert st_seal.cpu().tolist() == [0] * n
    assert host(out) == b"".join(frames)
    assert st_open.cpu().tolist() == [admit(frames[i], keys[sess[i]], w.local, difficulty)[0] for i in range(n)]
    assert OK in st_open.cpu().tolist()
