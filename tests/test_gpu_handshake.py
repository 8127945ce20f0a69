"""GPU tests of the device session table (handshake.hip; enet_handshake_accept_batch,
enet_session_rotate_batch, enet_key_exchange_batch): bit-exact against the pure-Python restatement
tests/handshake_ref.py, which tests/golden/handshake.json (the compiled reference's answers) pins.
Every record of every batch is compared; table slots a call must not write are compared byte for
byte with the sentinel pattern they were filled with.  The composition test runs accept ->
wire_seal_sessions -> rotate -> seal -> open on one stream with no synchronisation in between."""
import dataclasses
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import handshake_ref as H
from util import splitmix_array, splitmix_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = H.P
U32, U64 = 2**32 - 1, 2**64 - 1
KWG = 256   # enet::kWG, the workgroup size of the three kernels
LOCAL_PRIVATE = 0x5EED1234
EDGE_PUBLICS = [0, 1, 2, P - 1, P, P + 1, U32]


@pytest.fixture(scope="module")
def enet():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ephemeralnet_amd as E
    E.lib()
    return E


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "handshake.json")) as f:
        return json.load(f)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # a writable, contiguous copy


def dev_u32(vals):
    return dev(np.array(vals, np.uint32).view(np.int32))


def dev_u64(vals):
    return dev(np.array(vals, np.uint64).view(np.int64))


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def pool():
    """The local identity and 25 handshakes: (peer id, remote public, work nonce), the nonces solved
    by the restatement at difficulties 12, 8, 4, 1 in turn; entry 24 has the local node's own
    public (equal publics).  Computed once, never modified."""
    local_id = splitmix_bytes(70000, 32)
    local_public = H.compute_public(LOCAL_PRIVATE)
    entries = []
    for k in range(25):
        peer = splitmix_bytes(70100 + k, 32)
        priv = LOCAL_PRIVATE if k == 24 else int.from_bytes(splitmix_bytes(70200 + k, 4), "little")
        pub = H.compute_public(priv)
        assert H.validate_public(pub)
        diff = [12, 8, 4, 1][k % 4]
        nonce = H.solve_pow(peer, local_id, pub, diff, start=int.from_bytes(splitmix_bytes(70300 + k, 8), "little"))
        entries.append((peer, pub, nonce, diff))
    return {"local_id": local_id, "local_public": local_public, "entries": entries}


def requests_for(pool, n):
    """n requests: the pool in turn, with every edge public and off-by-one / garbage nonces mixed in."""
    reqs = []
    for i in range(n):
        peer, pub, nonce, _ = pool["entries"][i % len(pool["entries"])]
        if i % 11 == 5:
            pub = EDGE_PUBLICS[(i // 11) % len(EDGE_PUBLICS)]
        elif i % 7 == 3:
            nonce = (nonce + 1 + i) & U64
        elif i % 13 == 8:
            peer = splitmix_bytes(71000 + i, 32)   # another peer's proof
        reqs.append((peer, pub, nonce))
    return reqs


def sentinel_table(enet, S, seed):
    """A table whose every byte is a seeded pattern (some slots look live, some dead)."""
    t = enet.SessionTable.empty(S)
    t.secrets.copy_(dev(splitmix_array(seed, S * 32).reshape(S, 32)))
    t.keys.copy_(dev(splitmix_array(seed + 1, S * 32).reshape(S, 32)))
    t.mid.copy_(dev(splitmix_array(seed + 2, S * 64).view(np.int32).reshape(S, 16)))
    t.counters.copy_(dev(splitmix_array(seed + 3, S * 8).view(np.int64)))
    t.last_rotation.copy_(dev(splitmix_array(seed + 4, S * 8).view(np.int64)))
    t.live.copy_(dev(splitmix_array(seed + 5, S) % 3))
    return t


def table_host(t):
    return {f.name: host(getattr(t, f.name)).copy() for f in dataclasses.fields(t)}


def midstates_of(enet, keys):
    """enet_hmac_midstates of a [S,32] host key array (the layout the table's mid must have)."""
    import torch
    S = keys.shape[0]
    mid = torch.zeros((S, 16), dtype=torch.int32, device="cuda")
    enet.hmac_midstates(dev(keys), S, mid)
    return host(mid)


ACCEPT_CASES = [(n, kind, [12, 8, 4, 1, 0][idx % 5], idx)
                for idx, (n, kind) in enumerate(itertools.product([1, 63, 64, 65, KWG, KWG + 1, 1000],
                                                                  ["identity", "reversed", "sparse"]))]


@pytest.mark.parametrize("n,kind,difficulty,idx", ACCEPT_CASES)
def test_accept_matches_restatement(enet, pool, n, kind, difficulty, idx):
    """Verdicts, secrets, keys, midstates, counters, times and live flags of every record, with
    slots as identity (NULL, the table one slot short so the last record is out of range),
    reversed, or scattered into 1024 slots; one slot == S and one == 0xFFFFFFFF; difficulty 0
    with a NULL or a garbage nonce array.  Every slot not accepted keeps its sentinel bytes."""
    import torch
    reqs = requests_for(pool, n)
    strong = [e[:3] for e in pool["entries"] if e[3] == 12]   # proofs good at every difficulty used here
    if kind == "identity":
        S, slots = max(n - 1, 1), list(range(n))
        if n > 1:
            reqs[n - 1] = strong[1]    # a good handshake whose slot n - 1 is the first past the table
    elif kind == "reversed":
        S, slots = n, list(range(n))[::-1]
    else:
        S = 1024
        slots = [int(x) for x in np.random.default_rng(1000 + n).permutation(S)[:n]]
    if kind != "identity" and n >= 3:
        reqs[n // 2], reqs[0] = strong[2], strong[0]
        slots[n // 2] = S          # the first slot past the table
        slots[0] = U32
    now = 1_700_000_000_000 + 977 * idx
    expect = [H.accept(peer, pub, nonce, slots[i], S, pool["local_id"], LOCAL_PRIVATE, pool["local_public"], difficulty)
              for i, (peer, pub, nonce) in enumerate(reqs)]
    verdicts = [e[0] for e in expect]
    if n >= 63:   # the mix the case is meant to have (the restatement said so, nothing is assumed)
        assert {H.HS_OK, H.HS_BAD_PUBLIC, H.HS_BAD_SLOT} <= set(verdicts)
        assert (H.HS_BAD_POW in verdicts) == (difficulty != 0)

    table = sentinel_table(enet, S, 72000 + idx)
    want = table_host(table)
    for i, (v, secret, key) in enumerate(expect):
        if v == H.HS_OK:
            s = slots[i]
            want["secrets"][s] = np.frombuffer(secret, np.uint8)
            want["keys"][s] = np.frombuffer(key, np.uint8)
            want["counters"][s], want["last_rotation"][s], want["live"][s] = 0, now, 1
    accepted = np.array([slots[i] for i, e in enumerate(expect) if e[0] == H.HS_OK], np.int64)
    want["mid"][accepted] = midstates_of(enet, want["keys"])[accepted]

    d_peers = dev(np.frombuffer(b"".join(r[0] for r in reqs), np.uint8))
    d_pubs = dev_u32([r[1] for r in reqs])
    if difficulty == 0 and idx % 2 == 0:
        d_nonce = None                                           # as the reference: never looked at
    elif difficulty == 0:
        d_nonce = dev_u64([(0xDEAD0000 + 7919 * i) & U64 for i in range(n)])
    else:
        d_nonce = dev_u64([r[2] for r in reqs])
    d_slot = None if kind == "identity" else dev_u32(slots)
    d_lid = dev(np.frombuffer(pool["local_id"], np.uint8))
    verdict = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    enet.handshake_accept(table, d_peers, d_pubs, d_nonce, d_slot, d_lid, LOCAL_PRIVATE, pool["local_public"],
                          difficulty, now, verdict)
    torch.cuda.synchronize()
    assert host(verdict).tolist() == verdicts
    got = table_host(table)
    for name in want:
        assert np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("S", [1, 65, 257])
@pytest.mark.parametrize("interval", [10**9, 0])
def test_rotate_matches_restatement(enet, golden, S, interval):
    """Live and dead slots whose last rotation lies interval - 1, exactly interval and
    interval + 1 before now, counters 0, 2^32-1 and 2^64-1 (which wraps to 0); slot 0 is the golden
    file's rotation.  Slots that are not due keep every byte."""
    import torch
    g = golden["cases"][0]
    now = g["rotate_ticks"]
    table = sentinel_table(enet, S, 73000 + S)
    secrets = splitmix_array(73500 + S, S * 32).reshape(S, 32)
    secrets[0] = np.frombuffer(bytes.fromhex(g["secret"]), np.uint8)
    live = np.array([0 if (s % 5 == 4) else 1 + (s % 2) * 6 for s in range(S)], np.uint8)   # 1 and 7 are both live
    delta = [[interval, interval - 1, interval + 1][s % 3] for s in range(S)]
    last = np.array([now - d for d in delta], np.int64)
    counters = np.array([[0, U32, U64, 5][s % 4] for s in range(S)], np.uint64)
    table.secrets.copy_(dev(secrets))
    table.live.copy_(dev(live))
    table.last_rotation.copy_(dev(last))
    table.counters.copy_(dev(counters.view(np.int64)))
    want = table_host(table)
    want_rot = []
    for s in range(S):
        r = H.rotate(int(live[s]), secrets[s].tobytes(), int(counters[s]), int(last[s]), now, interval)
        want_rot.append(0 if r is None else 1)
        if r is not None:
            want["counters"][s] = np.array([r[0]], np.uint64).view(np.int64)[0]
            want["last_rotation"][s] = now
            want["keys"][s] = np.frombuffer(r[1], np.uint8)
    due = np.array([s for s in range(S) if want_rot[s]], np.int64)
    want["mid"][due] = midstates_of(enet, want["keys"])[due]
    assert want_rot[0] == 1 and want["keys"][0].tobytes().hex() == g["rotated_key"] and want["counters"][0] == 1
    if S > 1:
        assert 0 in want_rot and any(live[s] == 0 and delta[s] >= interval for s in range(S))
        assert any(counters[s] == U64 and want_rot[s] for s in range(S))     # the wrap is exercised
    rotated = torch.full((S,), 0xEE, dtype=torch.uint8, device="cuda")
    enet.session_rotate(table, now, interval, rotated)
    torch.cuda.synchronize()
    assert host(rotated).tolist() == want_rot
    got = table_host(table)
    for name in want:
        assert np.array_equal(got[name], want[name]), name


def test_key_exchange_matches_restatement(enet, golden):
    """The golden keypairs and 1000 seeded pairs: publics and secrets in one call, each output
    alone with the other pointer NULL, and both peers of a pair derive the same secret."""
    import torch
    privs = [c["local_private"] for c in golden["cases"]]
    remotes = [c["remote_public"] for c in golden["cases"]]
    a = splitmix_array(74000, 4000).view(np.uint32).tolist()
    b = splitmix_array(74001, 4000).view(np.uint32).tolist()
    a[:3], b[:3] = [0, 1, U32], [U32, 0, 1]
    privs += a
    remotes += [H.compute_public(x) for x in b]
    n = len(privs)
    want_pub = [H.compute_public(x) for x in privs]
    want_sec = b"".join(H.shared_secret(x, r) for x, r in zip(privs, remotes))
    for c, pub, k in zip(golden["cases"], want_pub, range(n)):     # the golden file rules
        assert pub == c["local_public"] and want_sec[32 * k:32 * k + 32].hex() == c["secret"]
    d_priv, d_rem = dev_u32(privs), dev_u32(remotes)

    def run(with_pub, with_sec):
        pub = torch.full((n,), -0x11111112, dtype=torch.int32, device="cuda") if with_pub else None
        sec = torch.full((n, 32), 0xEE, dtype=torch.uint8, device="cuda") if with_sec else None
        enet.key_exchange(d_priv, d_rem if with_sec else None, pub, sec)
        torch.cuda.synchronize()
        if with_pub:
            assert host(pub).view(np.uint32).tolist() == want_pub
        if with_sec:
            assert host(sec).tobytes() == want_sec

    run(True, True)
    run(True, False)
    run(False, True)
    # the other side: privates b against the device's publics of a
    pub_a = torch.zeros(len(a), dtype=torch.int32, device="cuda")
    sec_b = torch.zeros((len(a), 32), dtype=torch.uint8, device="cuda")
    enet.key_exchange(dev_u32(a), None, pub_a, None)
    enet.key_exchange(dev_u32(b), pub_a, None, sec_b)
    torch.cuda.synchronize()
    assert host(sec_b).tobytes() == want_sec[32 * len(golden["cases"]):]


def test_accept_seal_rotate_open_on_one_stream(enet, pool):
    """accept -> wire_seal_sessions straight from table.keys / table.mid -> rotate -> seal -> open,
    all queued on one stream with no synchronisation between the calls.  The first frames are
    byte-equal to wire_seal under per-frame keys from the restatement, the second ones to wire_seal
    under the rotated keys, they open, and a frame sealed before the rotation fails closed."""
    import torch
    S, n_req, n = 96, 80, 300
    difficulty = 4
    reqs = requests_for(pool, n_req)
    slots = [int(x) for x in np.random.default_rng(5).permutation(S)[:n_req]]
    now, now2 = 5_000_000_000, 9_000_000_123
    expect = [H.accept(p, pub, nonce, slots[i], S, pool["local_id"], LOCAL_PRIVATE, pool["local_public"], difficulty)
              for i, (p, pub, nonce) in enumerate(reqs)]
    secret_of = {slots[i]: e[1] for i, e in enumerate(expect) if e[0] == H.HS_OK}
    key_of = {slots[i]: e[2] for i, e in enumerate(expect) if e[0] == H.HS_OK}
    live = sorted(key_of)
    assert 10 < len(live) < n_req
    key2_of = {s: H.derive_key(secret_of[s], 1, now2) for s in live}
    rng = np.random.default_rng(6)
    sess = [live[int(x)] for x in rng.integers(0, len(live), n)]
    lens = [int(x) for x in rng.integers(0, 2000, n)]
    lens[:5] = [0, 1, 63, 64, 1500]
    msgs = [splitmix_bytes(75000 + i, L) for i, L in enumerate(lens)]
    nonces = [splitmix_bytes(76000 + i, 12) for i in range(n)]
    ooffs = torch.tensor(np.concatenate([[0], np.cumsum([L + 48 for L in lens])]).astype(np.int64)).cuda()
    poffs = torch.tensor(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).cuda()
    total_out, total_pt = int(ooffs[-1]), max(int(poffs[-1]), 1)

    def reference_frames(keys):
        b = enet.make_batch(msgs, keys, nonces)
        out = torch.zeros(total_out, dtype=torch.uint8, device="cuda")
        enet.wire_seal(b, out, ooffs)
        torch.cuda.synchronize()
        return host(out).tobytes()

    ref1 = reference_frames([key_of[s] for s in sess])
    ref2 = reference_frames([key2_of[s] for s in sess])
    assert ref1 != ref2

    table = enet.SessionTable.empty(S)
    d_peers = dev(np.frombuffer(b"".join(r[0] for r in reqs), np.uint8))
    d_pubs, d_nonce, d_slot = dev_u32([r[1] for r in reqs]), dev_u64([r[2] for r in reqs]), dev_u32(slots)
    d_lid = dev(np.frombuffer(pool["local_id"], np.uint8))
    d_sess = dev_u32(sess)
    verdict = torch.zeros(n_req, dtype=torch.uint8, device="cuda")
    rotated = torch.zeros(S, dtype=torch.uint8, device="cuda")
    b = dataclasses.replace(enet.make_batch(msgs, [bytes(32)] * n, nonces), keys=table.keys)
    out1 = torch.zeros(total_out, dtype=torch.uint8, device="cuda")
    out2 = torch.zeros(total_out, dtype=torch.uint8, device="cuda")
    pt2 = torch.full((total_pt,), 0xAA, dtype=torch.uint8, device="cuda")
    pt_old = torch.full((total_pt,), 0xAA, dtype=torch.uint8, device="cuda")
    macs = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    ok2 = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ok_old = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    bo2 = dataclasses.replace(b, arena=out2, offsets=ooffs, nonces=None,
                              total_bytes_hint=total_out, max_len_hint=max(lens) + 48)
    bo_old = dataclasses.replace(bo2, arena=out1)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        enet.handshake_accept(table, d_peers, d_pubs, d_nonce, d_slot, d_lid, LOCAL_PRIVATE, pool["local_public"],
                              difficulty, now, verdict, stream=s)
        enet.wire_seal_sessions(b, out1, ooffs, d_sess, S, table.mid, stream=s)
        enet.session_rotate(table, now2, 0, rotated, stream=s)
        enet.wire_seal_sessions(b, out2, ooffs, d_sess, S, table.mid, stream=s)
        enet.wire_open_sessions(bo2, pt2, poffs, d_sess, S, table.mid, macs, ok2, stream=s)
        enet.wire_open_sessions(bo_old, pt_old, poffs, d_sess, S, table.mid, macs, ok_old, stream=s)
    s.synchronize()
    assert host(verdict).tolist() == [e[0] for e in expect]
    assert host(rotated).tolist() == [1 if x in key_of else 0 for x in range(S)]
    assert host(out1).tobytes() == ref1
    assert host(out2).tobytes() == ref2
    assert host(ok2).tolist() == [1] * n and host(pt2).tobytes()[:sum(lens)] == b"".join(msgs)
    assert host(ok_old).tolist() == [0] * n and host(pt_old).tobytes()[:sum(lens)] == bytes(sum(lens))
    assert host(table.keys)[live].tobytes() == b"".join(key2_of[x] for x in live)
    assert host(table.counters)[live].tolist() == [1] * len(live)


def test_cpp_batch_forms_match_golden(enet, golden, pool, tmp_path):
    """crypto::batch::key_exchange and handshake_accept (tests/cpp/handshake_api_test.cpp, linked
    against the library the package loaded) on the golden cases, and an admission batch at
    difficulty 8 against the restatement."""
    lib = enet.LIB_PATH
    exe = str(tmp_path / "handshake_api_test")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "handshake_api_test.cpp"), "-o", exe,
                    "-L", os.path.dirname(lib), "-lenet_crypto", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    cases = golden["cases"]
    pairs = [f"{c['local_private']} {c['remote_public']}" for c in cases]
    text = [f"kx {len(cases)} secrets"] + pairs + [f"kx {len(cases)} nosecrets"] + pairs
    want = [f"{c['local_public']} {c['secret']}" for c in cases] + [f"{c['local_public']} -" for c in cases]
    zero = bytes(32).hex()
    lid = splitmix_bytes(77000, 32)
    for c in cases:   # difficulty 0: one request per call, the call's local key is the case's
        text += [f"accept {lid.hex()} {c['local_private']} 0 {c['rotate_ticks']} 1",
                 f"{splitmix_bytes(77001, 32).hex()} {c['remote_public']} 12345"]
        want.append(f"1 {c['secret']} {c['material_key']}" if c["remote_valid"] else f"0 {zero} {zero}")
    reqs = requests_for(pool, 300)
    text.append(f"accept {pool['local_id'].hex()} {LOCAL_PRIVATE} 8 42 {len(reqs)}")
    for i, (peer, pub, nonce) in enumerate(reqs):
        text.append(f"{peer.hex()} {pub} {nonce}")
        v, secret, key = H.accept(peer, pub, nonce, i, len(reqs), pool["local_id"], LOCAL_PRIVATE,
                                  pool["local_public"], 8)
        want.append(f"{v} {secret.hex() if secret else zero} {key.hex() if key else zero}")
    assert {w[0] for w in want[-len(reqs):]} == {"0", "1", "2"}
    res = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert res.stdout.splitlines() == want
