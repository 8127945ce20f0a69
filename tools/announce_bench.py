"""Device timings of the announce frames (profiles/announce_bench.json): the fused receive
(announce_frame_open: one launch) against wire_open_sessions followed by pow_check over pre-built
prefixes, the fused send (announce_frame_seal: search + seal) against pow_search over pre-built
prefixes followed by wire_seal_sessions over a pre-built message arena, the time to build those
two arenas on the device (the composed path needs them, the fused one does not), and the open at
difficulty 0 against wire_open_sessions alone -- all sides in the same run, alternating, HIP
events around `reps` back-to-back calls, median of rounds.  Shapes: 65 536 announces at the golden
manifest URI's length (354 bytes) and at MTU size (1 400-byte messages), difficulty 6, 64 shared
manifests, 256 shared endpoints.  Every output is checked (fused == composed, every status 0)
before anything is timed.  `python tools/announce_bench.py [out.json]`; needs the MI355X."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ephemeralnet_amd as E  # noqa: E402

SHAPES = [(65536, 21, 354, 5, 5), (65536, 14, 1290, 6, 5)]  # records, E, U, A, calls per timed round
SESSIONS, MANIFESTS, ENDPOINTS, TTL, DIFFICULTY, ATTEMPTS = 64, 64, 256, 3600, 6, 500_000


def timed(fn, reps, rounds=5):
    """Median over `rounds` of the mean time of `reps` back-to-back calls, in microseconds."""
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def arange_offsets(n, step):
    return torch.arange(0, (n + 1) * step, step, dtype=torch.int64, device="cuda")[: n + 1]


def be(value, width):
    return torch.tensor(list(int(value).to_bytes(width, "big")), dtype=torch.uint8, device="cuda")


def be64_rows(x):
    """int64 [n] -> uint8 [n, 8], most significant byte first"""
    sh = torch.arange(56, -8, -8, dtype=torch.int64, device="cuda")
    return ((x.unsqueeze(1) >> sh) & 0xFF).to(torch.uint8)


def shape(n, EL, UL, AL, reps, g):
    rnd = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=g)  # noqa: E731
    ridx = lambda hi: torch.randint(0, hi, (n,), dtype=torch.int32, device="cuda", generator=g)  # noqa: E731
    F = EL + UL + AL
    M, P = 90 + F, 112 + F          # message (v4) and PoW prefix bytes
    FR = M + 48
    cids, uris, eps = rnd(MANIFESTS, 32), rnd(MANIFESTS, UL), rnd(ENDPOINTS, EL)
    shards, local = rnd(n, AL), rnd(32)
    midx, eidx = ridx(MANIFESTS), ridx(ENDPOINTS)
    ttl = torch.full((n,), TTL, dtype=torch.int32, device="cuda")
    table = rnd(SESSIONS * 32)
    mid = torch.zeros(16 * SESSIONS, dtype=torch.int32, device="cuda")
    E.hmac_midstates(table, SESSIONS, mid)
    sess, fnonces = ridx(SESSIONS), rnd(n * 12)
    skw = dict(session=sess, sessions=SESSIONS, mid=mid)
    f_off, m_off, p_off = arange_offsets(n, FR), arange_offsets(n, M), arange_offsets(n, P)
    fields = E.AnnounceFields(chunk_ids=cids.reshape(-1), uris=uris.reshape(-1), uri_offsets=arange_offsets(MANIFESTS, UL),
                              endpoint_bytes=eps.reshape(-1), endpoint_offsets=arange_offsets(ENDPOINTS, EL),
                              shards=shards.reshape(-1), shard_offsets=arange_offsets(n, AL), peer_id=local, ttl=ttl,
                              manifest=midx, endpoint=eidx)

    # ---- send: fused search + seal
    tx = E.Batch(None, f_off, table, fnonces)
    frames = torch.zeros(n * FR, dtype=torch.uint8, device="cuda")
    nonce = torch.zeros(n, dtype=torch.int64, device="cuda")
    st_seal = torch.full((n,), 9, dtype=torch.uint8, device="cuda")

    def fused_seal():
        E.announce_frame_seal(tx, frames, f_off, fields, DIFFICULTY, nonce, st_seal, max_attempts=ATTEMPTS, **skw)

    def fused_seal_given():  # the seal launch alone: the nonces of an earlier search
        E.announce_frame_seal(tx, frames, f_off, fields, DIFFICULTY, nonce, st_seal, max_attempts=0, **skw)

    # ---- receive: fused open
    rx = E.Batch(frames, f_off, table, None, total_bytes_hint=n * FR, max_len_hint=FR)
    msgs = torch.zeros(n * M, dtype=torch.uint8, device="cuda")
    info = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
    st_open = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    peers = local.repeat(n)

    def fused_open():
        E.announce_frame_open(rx, msgs, m_off, peers, DIFFICULTY, info, st_open, **skw)

    def fused_open_d0():
        E.announce_frame_open(rx, msgs, m_off, peers, 0, info, st_open, **skw)

    # ---- composed: the two arenas, built on the device from the same tables
    pre = torch.zeros((n, P), dtype=torch.uint8, device="cuda")
    msgs2 = torch.zeros((n, M), dtype=torch.uint8, device="cuda")
    li, mi = midx.long(), eidx.long()

    def build_prefixes():
        o = 0
        for length, rows in ((32, cids[li]), (32, local.expand(n, 32)), (EL, eps[mi]), (UL, uris[li]), (AL, shards)):
            pre[:, o:o + 8] = be(length, 8)
            pre[:, o + 8:o + 8 + length] = rows
            o += 8 + length
        pre[:, o:o + 8] = be(TTL, 8)

    def build_messages():
        msgs2[:, 0], msgs2[:, 1] = 4, 1
        msgs2[:, 2:6], msgs2[:, 6:10], msgs2[:, 10:14], msgs2[:, 14:18] = be(TTL, 4), be(EL, 4), be(UL, 4), be(AL, 4)
        msgs2[:, 18:50], msgs2[:, 50:82] = cids[li], local
        msgs2[:, 82:82 + EL], msgs2[:, 82 + EL:82 + EL + UL], msgs2[:, 82 + EL + UL:82 + F] = eps[mi], uris[li], shards
        msgs2[:, 82 + F:] = be64_rows(nonce)

    diff = torch.full((n,), DIFFICULTY, dtype=torch.uint8, device="cuda")
    nonce2 = torch.zeros(n, dtype=torch.int64, device="cuda")
    found = torch.zeros(n, dtype=torch.uint8, device="cuda")
    frames2 = torch.zeros_like(frames)
    mb = E.Batch(msgs2.reshape(-1), m_off, table, fnonces, total_bytes_hint=n * M, max_len_hint=M)

    def composed_seal():
        E.pow_search(pre.reshape(-1), p_off, diff, E.POW_NODE, ATTEMPTS, nonce2, found)
        E.wire_seal_sessions(mb, frames2, f_off, sess, SESSIONS, mid)

    back = torch.zeros(n * M, dtype=torch.uint8, device="cuda")
    macs = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    ok_w = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ok_p = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def wire_open_alone():
        E.wire_open_sessions(rx, back, m_off, sess, SESSIONS, mid, macs, ok_w)

    def composed_open():  # (the host parse and prefix build between the two calls is not timed)
        wire_open_alone()
        E.pow_check(pre.reshape(-1), p_off, nonce, diff, ok_p)

    # ---- every output, before anything is timed
    fused_seal()
    assert int(st_seal.sum()) == 0, "a record found no nonce"
    first = frames.clone()
    fused_seal_given()
    assert torch.equal(frames, first) and int(st_seal.sum()) == 0
    fused_open()
    assert int(st_open.sum()) == 0, "a sealed frame was not admitted"
    want = torch.tensor([4, TTL, EL, UL, AL], dtype=torch.int32, device="cuda")
    assert torch.equal(info[:, :5], want.expand(n, 5))
    assert torch.equal((info[:, 6].long() << 32) | (info[:, 5].long() & 0xFFFFFFFF), nonce)
    build_prefixes()
    build_messages()
    assert torch.equal(msgs2.reshape(-1), msgs), "the fused open's message != the assembled message"
    composed_seal()
    assert int(found.sum()) == n and torch.equal(nonce2, nonce) and torch.equal(frames2, frames)
    composed_open()
    assert int(ok_w.sum()) == n and int(ok_p.sum()) == n and torch.equal(back, msgs)
    fused_open_d0()
    assert int(st_open.sum()) == 0

    fns = (fused_seal, fused_seal_given, composed_seal, build_prefixes, build_messages, fused_open, composed_open,
           fused_open_d0, wire_open_alone)
    for f in fns:
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    runs = {f.__name__: [] for f in fns}
    for _ in range(3):  # alternate, so that every form meets the same clocks
        for f in fns:
            runs[f.__name__].append(timed(f, reps, rounds=3))
    res = {"records": n, "endpoint_bytes": EL, "uri_bytes": UL, "shard_bytes": AL, "message_bytes": M, "frame_bytes": FR,
           "prefix_bytes": P, "difficulty": DIFFICULTY}
    for k, v in runs.items():
        res[k + "_us"] = sorted(v)[1]
    us = lambda k: res[k + "_us"][0]  # noqa: E731
    for k in ("fused_seal", "fused_seal_given", "composed_seal", "fused_open", "composed_open", "fused_open_d0",
              "wire_open_alone"):
        res[k + "_frame_gib_s"] = n * FR / (us(k) * 1e-6) / 2**30
    res["open_fused_over_composed"] = us("fused_open") / us("composed_open")
    res["open_fused_over_composed_with_prefix_build"] = us("fused_open") / (us("composed_open") + us("build_prefixes"))
    res["seal_fused_over_composed"] = us("fused_seal") / us("composed_seal")
    res["seal_fused_over_composed_with_builds"] = us("fused_seal") / (us("composed_seal") + us("build_prefixes")
                                                                        + us("build_messages"))
    res["open_d0_fused_over_wire_open"] = us("fused_open_d0") / us("wire_open_alone")
    return res


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    E.lib()
    g = torch.Generator(device="cuda").manual_seed(13)
    res = {"device": torch.cuda.get_device_name(0),
           "timing": "HIP events; per form the median of 3 alternating passes, each the median (min, max) of 3 rounds",
           "composed_open": "wire_open_sessions, then pow_check over a pre-built prefix arena, same stream; the host "
                            "parse and the prefix build between them are not in this figure",
           "composed_seal": "pow_search over the pre-built prefix arena, then wire_seal_sessions over a pre-built "
                            "message arena",
           "builds": "build_prefixes / build_messages: the arenas assembled on the device by tensor copies from the "
                     "same shared tables (the fused calls need neither)",
           "ratios": "fused time / composed time (below 1: the fused call is faster)",
           "shapes": []}
    for n, EL, UL, AL, reps in SHAPES:
        res["shapes"].append(shape(n, EL, UL, AL, reps, g))
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
