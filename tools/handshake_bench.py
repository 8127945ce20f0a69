"""Timings of the device session table (profiles/handshake_bench.json): 65 536 handshakes
admitted at difficulty 12 (every proof valid: the nonces are found by pow_search first, so each
record runs all nine compressions), a rotation of a 65 536-slot table with every slot due,
wire_seal_sessions of 65 536 frames alone against accept -> wire_seal_sessions on one stream (the
two alternating), and one host core admitting the same requests through the scalar drop-in API
(tools/handshake_host_bench.cpp, built here with g++).  Device figures: HIP events around REPS
back-to-back calls, the median of RUNS such runs after warm-up.  Results are checked before
anything is timed: every verdict is OK, and the host program's keys hash to the table's.
`python tools/handshake_bench.py [out.json]`; needs the MI355X."""
import dataclasses
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ephemeralnet_amd as E  # noqa: E402

N, DIFFICULTY, FRAME = 65536, 12, 1024
RUNS, REPS = 25, 10
LOCAL_PRIVATE = 0x5EED1234


def runs_of(fn, runs, reps):
    """`runs` timed runs: each the mean time of `reps` back-to-back calls between two events, microseconds."""
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / reps)
    return out


def summary(times):
    times = sorted(times)
    return times[len(times) // 2], times[0], times[-1]   # median, min, max


def timed(fn, runs=RUNS, reps=REPS):
    return summary(runs_of(fn, runs, reps))


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    E.lib()
    rng = np.random.default_rng(12)
    local_id = rng.integers(0, 256, 32, dtype=np.uint8)
    peers = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    privs = rng.integers(2, 2**31 - 2, N, dtype=np.int64).astype(np.uint32)
    d_priv = torch.from_numpy(privs.view(np.int32)).cuda()
    d_pub = torch.zeros(N, dtype=torch.int32, device="cuda")
    mine = torch.tensor([LOCAL_PRIVATE], dtype=torch.int32, device="cuda")
    mine_pub = torch.zeros(1, dtype=torch.int32, device="cuda")
    E.key_exchange(d_priv, None, d_pub, None)
    E.key_exchange(mine, None, mine_pub, None)
    pubs = d_pub.cpu().numpy().view(np.uint32)
    local_public = int(mine_pub.cpu().numpy().view(np.uint32)[0])

    # the 88-byte PoW prefixes BE64(32) || peer || BE64(32) || local id || BE64(public); the nonces
    # come from the device search
    pre = np.zeros((N, 88), np.uint8)
    pre[:, 7] = 32
    pre[:, 8:40] = peers
    pre[:, 47] = 32
    pre[:, 48:80] = local_id
    pre[:, 84:88] = pubs.astype(">u4").view(np.uint8).reshape(N, 4)
    d_pre = torch.from_numpy(pre.reshape(-1)).cuda()
    d_off = torch.arange(0, (N + 1) * 88, 88, dtype=torch.int64, device="cuda")
    d_diff = torch.full((N,), DIFFICULTY, dtype=torch.uint8, device="cuda")
    d_nonce = torch.zeros(N, dtype=torch.int64, device="cuda")
    found = torch.zeros(N, dtype=torch.uint8, device="cuda")
    E.pow_search(d_pre, d_off, d_diff, E.POW_NODE, 500000, d_nonce, found)
    assert int(found.sum()) == N

    table = E.SessionTable.empty(N)
    d_peers = torch.from_numpy(peers.reshape(-1)).cuda()
    d_lid = torch.from_numpy(local_id).cuda()
    verdict = torch.zeros(N, dtype=torch.uint8, device="cuda")
    rotated = torch.zeros(N, dtype=torch.uint8, device="cuda")

    def accept():
        E.handshake_accept(table, d_peers, d_pub, d_nonce, None, d_lid, LOCAL_PRIVATE, local_public, DIFFICULTY,
                           1_000_000, verdict)

    def rotate():
        E.session_rotate(table, 2_000_000, 0, rotated)

    accept()
    assert int((verdict == E.ENET_HS_OK).sum()) == N and int(table.live.sum()) == N
    keys_sha = hashlib.sha256(table.keys.cpu().numpy().tobytes()).hexdigest()
    rotate()
    assert int(rotated.sum()) == N and int(table.counters.sum()) == N
    accept()

    # frames: one per session
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda n: torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)  # noqa: E731
    plain, nonces = rnd(N * FRAME), rnd(N * 12)
    offsets = torch.arange(0, (N + 1) * FRAME, FRAME, dtype=torch.int64, device="cuda")
    ooffs = torch.arange(0, (N + 1) * (FRAME + 48), FRAME + 48, dtype=torch.int64, device="cuda")
    out = torch.zeros(N * (FRAME + 48), dtype=torch.uint8, device="cuda")
    sess = torch.arange(0, N, dtype=torch.int32, device="cuda")
    b = E.Batch(plain, offsets, table.keys, nonces, total_bytes_hint=N * FRAME, max_len_hint=FRAME)

    def seal_alone():
        E.wire_seal_sessions(b, out, ooffs, sess, N, table.mid)

    def accept_seal():
        accept()
        seal_alone()

    # the sealed frames open under the table
    seal_alone()
    back = torch.zeros_like(plain)
    macs = torch.zeros(32 * N, dtype=torch.uint8, device="cuda")
    ok = torch.zeros(N, dtype=torch.uint8, device="cuda")
    bo = dataclasses.replace(b, arena=out, offsets=ooffs, nonces=None, total_bytes_hint=N * (FRAME + 48),
                             max_len_hint=FRAME + 48)
    E.wire_open_sessions(bo, back, offsets, sess, N, table.mid, macs, ok)
    assert int(ok.sum()) == N and torch.equal(back, plain)

    res = {"requests": N, "difficulty": DIFFICULTY, "frame_bytes": FRAME, "device": torch.cuda.get_device_name(0),
           "timing": f"HIP events around {REPS} back-to-back calls; median (min, max) of {RUNS} runs after warm-up"}
    for f in (accept, rotate, seal_alone, accept_seal):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    res["handshake_accept_us"] = timed(accept)
    res["session_rotate_us"] = timed(rotate)
    accept()   # rotation replaced the keys: back to the admitted ones
    sa, acs = [], []
    for _ in range(3):   # alternate the two forms
        sa += runs_of(seal_alone, 9, 5)
        acs += runs_of(accept_seal, 9, 5)
    res["wire_seal_sessions_alone_us"] = summary(sa)
    res["accept_then_wire_seal_sessions_us"] = summary(acs)
    res["seal_timing"] = "the two forms in 3 alternating blocks of 9 runs x 5 calls; median (min, max) of each form's 27 runs"
    res["accept_adds_percent"] = 100.0 * (res["accept_then_wire_seal_sessions_us"][0] /
                                          res["wire_seal_sessions_alone_us"][0] - 1.0)
    res["accepts_per_second"] = N / (res["handshake_accept_us"][0] * 1e-6)

    # one host core, the same requests, through the scalar drop-in API
    with tempfile.TemporaryDirectory() as tmp:
        exe, req = os.path.join(tmp, "handshake_host_bench"), os.path.join(tmp, "requests.bin")
        libdir = os.path.dirname(E.LIB_PATH)
        subprocess.run(["g++", "-O2", "-std=c++20", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "handshake_host_bench.cpp"), "-o", exe, "-L", libdir,
                        "-lenet_crypto", "-Wl,-rpath," + libdir], check=True)
        rec = np.zeros(N, dtype=[("peer", "u1", 32), ("pub", "<u4"), ("nonce", "<u8")])
        rec["peer"], rec["pub"], rec["nonce"] = peers, pubs, d_nonce.cpu().numpy().view(np.uint64)
        with open(req, "wb") as f:
            f.write(np.array([N, DIFFICULTY], "<u4").tobytes() + local_id.tobytes() +
                    np.array([LOCAL_PRIVATE, local_public], "<u4").tobytes() + rec.tobytes())
        hostres = json.loads(subprocess.run([exe, req], capture_output=True, text=True, check=True,
                                            timeout=600).stdout)
    assert hostres["accepted"] == N and hostres["keys_sha256"] == keys_sha, hostres
    hostres["timing"] = "steady_clock around one pass over all requests; median of 21 passes after 3 warm-up passes"
    res["host_one_core"] = hostres
    res["device_over_host_core"] = hostres["median_ms"] * 1e3 / res["handshake_accept_us"][0]
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
