"""GPU parity of the chunk transfer frames (chunk_frames.hip, enet_chunk_frame_seal_batch /
enet_chunk_frame_open_batch) against the CPU oracle: a stored chunk wrapped into a signed Chunk
message and a session wire frame in one pass (Node::dispatch_upload, Node.cpp:1254-1297), and the
receive side -- frame open, header checks, chunk decrypt, SHA-256 against the manifest -- in one
pass (SessionManager.cpp:760-822, Message.cpp:313-328 / 144-159, Node::receive_chunk,
Node.cpp:1615-1677).  Expected bytes: oracle.frame_seal over the helper's 42-byte header || data,
oracle.chacha20_xor from derive_counter(chunk_id), oracle.sha256.  Bit-exact throughout."""
import dataclasses

import numpy as np
import pytest

import oracle
from chunk_frame_ref import HEADER, OVERHEAD, chunk_header, chunk_message, clamp_version, stored_data, wire_frame
from util import splitmix_bytes

pytestmark = pytest.mark.gpu

SENT = 0xAA
# data lengths: empty; around the 22 / 42-byte carries; message 95..97 (tail + MAC crosses 128);
# the first chunk-keystream block boundary (message offset 106); message 127..129; 255..257;
# MTU, 4 KiB message, 4 KiB data; a 256 KiB message
SHORT = [0, 1, 21, 22, 23, 53, 54, 55, 63, 64, 65, 85, 86, 87, 213, 214, 215, 1458, 4054, 4096]
LONG = 262102
SESSIONS = 5


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


def host(t) -> bytes:
    return t.cpu().numpy().tobytes()


def offsets_for(lens, base):
    return np.concatenate([[base], base + np.cumsum(lens)]).astype(np.int64)


def records_of(arena: bytes, offs):
    return [arena[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]


@dataclasses.dataclass
class World:
    """n chunks with everything both sides know about them and the oracle's frames."""
    n: int
    pts: list
    data: list
    ids: list
    ckeys: list
    cnonces: list
    hashes: list
    ttl: list
    versions: list
    table: list
    sess: list
    fnonces: list
    frames: list

    @property
    def skeys(self):
        return [self.table[s] for s in self.sess]


def make_world(lens, seed) -> World:
    n = len(lens)
    pts = [splitmix_bytes(seed + i, L) for i, L in enumerate(lens)]
    ids = []
    for i in range(n):
        cid = splitmix_bytes(seed + 10000 + i, 32)
        if i % 7 == 3:
            cid = b"\xff\xff\xff\xff" + cid[4:]  # the chunk counter wraps after one block
        if i % 7 == 5:
            cid = b"\xfe\xff\xff\xff" + cid[4:]
        ids.append(cid)
    ckeys = [splitmix_bytes(seed + 20000 + i, 32) for i in range(n)]
    cnonces = [splitmix_bytes(seed + 30000 + i, 12) for i in range(n)]
    table = [splitmix_bytes(seed + 40000 + s, 32) for s in range(SESSIONS)]
    sess = [int(x) % SESSIONS for x in splitmix_bytes(seed + 50000, n)]
    fnonces = [splitmix_bytes(seed + 60000 + i, 12) for i in range(n)]
    ttl = [[3600, 0, 1, 0xFFFFFFFF, 0x01020304][i % 5] for i in range(n)]
    versions = [[1, 4, 0, 9, 2, 3][i % 6] for i in range(n)]
    data = [stored_data(ckeys[i], cnonces[i], ids[i], pts[i]) for i in range(n)]
    hashes = [oracle.sha256(p) for p in pts]
    frames = [wire_frame(table[sess[i]], fnonces[i], chunk_message(versions[i], ttl[i], ids[i], data[i]))
              for i in range(n)]
    return World(n, pts, data, ids, ckeys, cnonces, hashes, ttl, versions, table, sess, fnonces, frames)


@pytest.fixture(scope="module")
def ragged():
    lens = SHORT + [LONG]
    while len(lens) < 200:
        lens += SHORT
    return make_world(lens, 810000)


def session_args(enet, w, sess=None):
    import torch
    tbl = devb(b"".join(w.table))
    mid = torch.zeros(16 * SESSIONS, dtype=torch.int32, device="cuda")
    enet.hmac_midstates(tbl, SESSIONS, mid)
    st = dev(np.array(w.sess if sess is None else sess, dtype=np.uint32).view(np.int32))
    return tbl, dict(session=st, sessions=SESSIONS, mid=mid)


def run_seal(enet, w, base, sessions=True, out_lens=None, **batch_kw):
    """-> (frames, front sentinel, back sentinel)"""
    import torch
    b = enet.make_batch(w.data, w.skeys, w.fnonces, base_offset=base)
    kw = {}
    if sessions:
        tbl, kw = session_args(enet, w)
        b = dataclasses.replace(b, keys=tbl)
    b = dataclasses.replace(b, **batch_kw)
    ooffs = offsets_for(out_lens or [len(d) + OVERHEAD for d in w.data], base + 1)
    out = torch.full((int(ooffs[-1]) + 7,), SENT, dtype=torch.uint8, device="cuda")
    enet.chunk_frame_seal(b, out, dev(ooffs), devb(b"".join(w.ids)), dev(np.array(w.ttl, dtype=np.uint32).view(np.int32)),
                          versions=dev(np.array(w.versions, dtype=np.uint8)), **kw)
    o = host(out)
    return records_of(o, ooffs.tolist()), o[:base + 1], o[int(ooffs[-1]):]


def run_open(enet, w, frames, base, sessions=True, sess=None, ids=None, hashes=None, out_lens=None, data_out=True,
             **batch_kw):
    """-> dict(pt, data, status, ttl, and the sentinels around both output arenas)"""
    import torch
    b = enet.make_batch(frames, w.skeys, w.fnonces, base_offset=base)
    kw = {}
    if sessions:
        tbl, kw = session_args(enet, w, sess)
        b = dataclasses.replace(b, keys=tbl)
    b = dataclasses.replace(b, nonces=None, **batch_kw)
    ooffs = offsets_for(out_lens or [max(len(f) - OVERHEAD, 0) for f in frames], base + 2)
    size = int(ooffs[-1]) + 9
    pt = torch.full((size,), SENT, dtype=torch.uint8, device="cuda")
    ct = torch.full((size,), SENT, dtype=torch.uint8, device="cuda") if data_out else None
    n = len(frames)
    status = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    ttl = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    enet.chunk_frame_open(b, pt, dev(ooffs), devb(b"".join(ids or w.ids)), devb(b"".join(w.ckeys)),
                          devb(b"".join(w.cnonces)), devb(b"".join(hashes or w.hashes)), status, data_out=ct,
                          ttl_out=ttl, **kw)
    p, offs = host(pt), ooffs.tolist()
    res = dict(pt=records_of(p, offs), status=status.cpu().tolist(),
               ttl=ttl.cpu().numpy().view(np.uint32).tolist(), edges=[p[:offs[0]], p[offs[-1]:]])
    if data_out:
        c = host(ct)
        res["data"] = records_of(c, offs)
        res["edges"] += [c[:offs[0]], c[offs[-1]:]]
    return res


def assert_sentinels(edges):
    for e in edges:
        assert e == bytes([SENT]) * len(e)


@pytest.mark.parametrize("hinted", [True, False], ids=["long-frame-form", "short-frame-form"])
@pytest.mark.parametrize("sessions", [True, False], ids=["session-table", "per-record-keys"])
@pytest.mark.parametrize("base", [0, 3, 5])
def test_ragged_matrix(enet, ragged, base, sessions, hinted):
    """One mixed batch of 201 chunks over every length class (several 64-record workgroups, a
    partial last one, one 256 KiB message among short neighbours), arenas at byte offsets 0 / 3 / 5,
    chunk ids whose counter wraps, versions 1, 4, 0 (-> 1) and 9 (-> 4): the seal is the oracle's
    frame byte for byte; the open gives status 0, the plaintext, the stored ciphertext and the ttl;
    nothing outside the records' ranges is written.  The open kernel has two forms, chosen by
    max_len_hint (16 KiB and more: the long-frame form): the batch's true hints take the one,
    hints of 0 ("unknown") the other."""
    w = ragged
    assert w.n >= 200 and w.n % 64 != 0
    hints = {} if hinted else dict(max_len_hint=0, total_bytes_hint=0)
    got, front, back = run_seal(enet, w, base, sessions, **hints)
    for i in range(w.n):
        assert got[i] == w.frames[i], (i, len(w.data[i]))
    assert_sentinels([front, back])
    r = run_open(enet, w, w.frames, base, sessions, **hints)
    assert r["status"] == [0] * w.n
    for i in range(w.n):
        assert r["pt"][i] == w.pts[i], (i, len(w.pts[i]))
        assert r["data"][i] == w.data[i], (i, len(w.pts[i]))
    assert r["ttl"] == w.ttl
    assert_sentinels(r["edges"])


def test_agrees_with_two_call_path(enet, ragged):
    """The same frames through wire_open_sessions, then chunk_fetch over the data part of every
    opened message (a 2n-entry offsets table, message i = header record 2i + data record 2i+1,
    `order` naming the data records): the same plaintext and the same verdicts, also for a tampered
    frame and a wrong manifest hash.  The fused seal equals wire_seal_sessions over the assembled
    messages."""
    import torch
    w = ragged
    n = w.n
    frames = list(w.frames)
    frames[6] = frames[6][:40] + bytes([frames[6][40] ^ 4]) + frames[6][41:]
    hashes = list(w.hashes)
    hashes[17] = bytes([hashes[17][0] ^ 1]) + hashes[17][1:]
    fused = run_open(enet, w, frames, 0, hashes=hashes)
    # two calls
    tbl, kw = session_args(enet, w)
    b = dataclasses.replace(enet.make_batch(frames, w.skeys, w.fnonces), keys=tbl, nonces=None)
    mlens = [len(f) - 48 for f in frames]
    moffs = offsets_for(mlens, 0)
    msgs = torch.zeros(int(moffs[-1]) + 1, dtype=torch.uint8, device="cuda")
    macs = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    ok_w = torch.zeros(n, dtype=torch.uint8, device="cuda")
    enet.wire_open_sessions(b, msgs, dev(moffs), kw["session"], SESSIONS, kw["mid"], macs, ok_w)
    split = np.empty(2 * n + 1, dtype=np.int64)
    split[0::2] = moffs
    split[1::2] = moffs[:-1] + HEADER
    rows = lambda xs, k: devb(b"".join(bytes(k) + x for x in xs))  # record 2i+1 carries chunk i's entry
    fb = enet.Batch(arena=msgs, offsets=dev(split), keys=rows(w.ckeys, 32), nonces=rows(w.cnonces, 12),
                    order=dev(np.arange(1, 2 * n, 2, dtype=np.int32)), count=n)
    back = torch.zeros_like(msgs)
    ok_f = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    enet.chunk_fetch(fb, back, rows(w.ids, 32), rows(hashes, 32), ok_f)
    two_pt = records_of(host(back), split.tolist())[1::2]
    two_ok = [a & b for a, b in zip(ok_w.cpu().tolist(), ok_f.cpu().tolist()[1::2])]
    assert [int(s == 0) for s in fused["status"]] == two_ok
    assert [i for i in range(n) if not two_ok[i]] == [6, 17]
    assert fused["status"][6] == 1 and fused["status"][17] == 4
    for i in range(n):
        assert fused["pt"][i] == two_pt[i], i
    # seal: wire_seal_sessions over header || data
    ms = [chunk_message(w.versions[i], w.ttl[i], w.ids[i], w.data[i]) for i in range(n)]
    mb = dataclasses.replace(enet.make_batch(ms, w.skeys, w.fnonces), keys=tbl)
    foffs = offsets_for([len(m) + 48 for m in ms], 0)
    out = torch.zeros(int(foffs[-1]), dtype=torch.uint8, device="cuda")
    enet.wire_seal_sessions(mb, out, dev(foffs), kw["session"], SESSIONS, kw["mid"])
    got, _, _ = run_seal(enet, w, 0)
    assert got == records_of(host(out), foffs.tolist())


def test_every_status_fails_closed(enet):
    """One batch, one offending record per case; each gets exactly its status with zeroed
    plaintext, zeroed data_out and ttl 0, every other record status 0 and its bytes."""
    lens = [300, 0, 1, 86, 87, 129, 1458] * 12
    w = make_world(lens, 820000)
    n = w.n
    frames, sess, ids, hashes = list(w.frames), list(w.sess), list(w.ids), list(w.hashes)
    out_lens = [len(p) for p in w.pts]
    want = {}
    flip = lambda b, at, bit=1: b[:at] + bytes([b[at] ^ bit]) + b[at + 1:]
    key = lambda i: w.table[w.sess[i]]

    def resign(i, m, status):  # the altered message under the record's own key and nonce: it authenticates
        frames[i] = wire_frame(key(i), w.fnonces[i], m)
        out_lens[i] = max(len(m) - HEADER, 0)
        want[i] = status

    def header(i, **kw):
        a = dict(version=clamp_version(w.versions[i]), ttl=w.ttl[i], chunk_id=w.ids[i], data_len=len(w.data[i]))
        a.update(kw)
        return chunk_header(**a)

    # FRAME
    frames[7] = flip(frames[7], 16 + 60); want[7] = 1             # a body byte
    frames[14] = flip(frames[14], len(frames[14]) - 1, 0x80); want[14] = 1  # a MAC byte
    frames[21] = flip(frames[21], 15); want[21] = 1              # the length field
    frames[28] = splitmix_bytes(5, 47); out_lens[28] = 0; want[28] = 1  # shorter than header + MAC
    sess[35] = SESSIONS; want[35] = 1                            # the first index past the table
    # HEADER
    resign(42, header(42, version=0) + w.data[42], 2)
    resign(49, header(49, version=5) + w.data[49], 2)
    resign(56, header(56, type_byte=0x02) + w.data[56], 2)
    resign(63, header(63, data_len=301) + w.data[63], 2)
    resign(70, header(70, data_len=299) + w.data[70], 2)
    resign(77, header(77)[:41], 2)                               # a 41-byte message
    resign(6, header(6) + w.data[6] + bytes(range(8)), 2)        # 8 bytes after the data
    # CHUNK_ID
    ids[13] = flip(ids[13], 31); want[13] = 3
    # HASH
    hashes[20] = flip(hashes[20], 9, 0x10); want[20] = 4
    d = flip(w.data[27], 1000)
    frames[27] = wire_frame(key(27), w.fnonces[27], chunk_message(w.versions[27], w.ttl[27], w.ids[27], d)); want[27] = 4
    assert len(want) == 15 and all(len(w.data[i]) in (300, 1458) for i in want)

    r = run_open(enet, w, frames, 3, sess=sess, ids=ids, hashes=hashes, out_lens=out_lens)
    assert r["status"] == [want.get(i, 0) for i in range(n)]
    for i in range(n):
        if i in want:
            assert r["pt"][i] == bytes(out_lens[i]) and r["data"][i] == bytes(out_lens[i]) and r["ttl"][i] == 0, i
        else:
            assert r["pt"][i] == w.pts[i] and r["data"][i] == w.data[i] and r["ttl"][i] == w.ttl[i], i
    assert_sentinels(r["edges"])
    # seal: a slot of the wrong size or a session past the table is zeroed whole
    slens = [len(x) + OVERHEAD for x in w.data]
    slens[4] += 1
    got, front, back = run_seal(enet, w, 0, out_lens=slens)
    assert got[4] == bytes(slens[4])
    assert all(got[i] == w.frames[i] for i in range(n) if i != 4)
    assert_sentinels([front, back])


def test_order_and_hints(enet, ragged):
    """A longest-first permutation and a subset `order` give the bytes of the unordered call
    (records the subset does not name keep their sentinel); lying hints (total = count * max on a
    mixed batch, i.e. "uniform") change nothing."""
    w = ragged
    n = w.n
    by_len = np.argsort([-len(d) for d in w.data], kind="stable").astype(np.int32)
    r = run_open(enet, w, w.frames, 3, order=dev(by_len))
    assert r["status"] == [0] * n and r["pt"] == w.pts and r["data"] == w.data and r["ttl"] == w.ttl
    got, _, _ = run_seal(enet, w, 3, order=dev(by_len))
    assert got == w.frames
    sub = np.arange(0, n, 3, dtype=np.int32)[::-1].copy()
    named = set(sub.tolist())
    r = run_open(enet, w, w.frames, 3, order=dev(sub), count=len(sub))
    got, _, _ = run_seal(enet, w, 3, order=dev(sub), count=len(sub))
    for i in range(n):
        if i in named:
            assert r["status"][i] == 0 and r["pt"][i] == w.pts[i] and r["data"][i] == w.data[i] and r["ttl"][i] == w.ttl[i], i
            assert got[i] == w.frames[i], i
        else:
            assert r["status"][i] == 0x77 and r["ttl"][i] == 0x5A5A5A5A, i
            assert r["pt"][i] == bytes([SENT]) * len(w.pts[i]) and r["data"][i] == bytes([SENT]) * len(w.pts[i]), i
            assert got[i] == bytes([SENT]) * len(w.frames[i]), i
    assert_sentinels(r["edges"])
    mx = max(len(f) for f in w.frames)
    r = run_open(enet, w, w.frames, 0, max_len_hint=mx, total_bytes_hint=n * mx)
    assert r["status"] == [0] * n and r["pt"] == w.pts and r["data"] == w.data
    md = max(len(d) for d in w.data)
    got, _, _ = run_seal(enet, w, 0, max_len_hint=md, total_bytes_hint=n * md)
    assert got == w.frames


def test_one_stream_keys_stay_on_device(enet):
    """shamir_split -> shamir_combine writing into the tensor passed as chunk_keys ->
    chunk_frame_open, all on one stream with no synchronisation and no host copy in between."""
    import torch
    w = make_world([0, 1, 86, 300, 1458, 4096] * 22, 830000)
    n, t, sc = w.n, 3, 5
    secrets = devb(b"".join(w.ckeys)).reshape(n, 32)
    coeffs = devb(splitmix_bytes(831000, n * (t - 1) * 32)).reshape(n, t - 1, 32)
    shares = torch.zeros((n, sc, 32), dtype=torch.uint8, device="cuda")
    tbl, kw = session_args(enet, w)
    b = dataclasses.replace(enet.make_batch(w.frames, w.skeys, w.fnonces, base_offset=1), keys=tbl, nonces=None)
    ooffs = offsets_for([len(p) for p in w.pts], 2)
    d_ooffs, d_ids, d_cn, d_h = dev(ooffs), devb(b"".join(w.ids)), devb(b"".join(w.cnonces)), devb(b"".join(w.hashes))
    pt = torch.full((int(ooffs[-1]),), SENT, dtype=torch.uint8, device="cuda")
    keybuf = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    ok_c = torch.zeros(n, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    pick = torch.tensor([4, 1, 2], device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        enet.shamir_split(secrets, coeffs, t, sc, shares, stream=s)
        values = shares[:, pick, :].contiguous()
        indices = (pick + 1).to(torch.uint8).expand(n, t).contiguous()
        enet.shamir_combine(indices, values, t, keybuf, ok_c, stream=s)
        enet.chunk_frame_open(b, pt, d_ooffs, d_ids, keybuf, d_cn, d_h, status, stream=s, **kw)
    s.synchronize()
    assert ok_c.cpu().tolist() == [1] * n
    assert status.cpu().tolist() == [0] * n
    assert records_of(host(pt), ooffs.tolist()) == w.pts
