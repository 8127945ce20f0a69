"""Device timings of the chunk transfer frames (profiles/chunk_transfer_bench.json): the fused
receive (chunk_frame_open: one launch) against wire_open_sessions followed by chunk_fetch over the
data part of every opened message on the same stream, and the fused upload (chunk_frame_seal)
against the device copy that assembles header || data into a message arena followed by
wire_seal_sessions -- both sides of each pair in the same run, alternating, HIP events around
`reps` back-to-back calls, median of rounds.  Shapes: 65 536 x 1 458-byte chunks (1 500-byte
messages) and 16 384 x 64 KiB.  Every output is checked (fused == two-call == the inputs) before
anything is timed.  `python tools/chunk_transfer_bench.py [out.json]`; needs the MI355X."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ephemeralnet_amd as E  # noqa: E402

SHAPES = [(65536, 1458, 20), (16384, 65536, 4)]  # records, data bytes, calls per timed round
SESSIONS, TTL, HDR = 64, 3600, 42


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


def arange_offsets(n, step, first=0):
    return torch.arange(first, first + (n + 1) * step, step, dtype=torch.int64, device="cuda")[: n + 1]


def odd_rows(x, width):
    """[2n][width]: row 2i+1 = x[i] (record 2i+1 of the split message arena is chunk i's data)."""
    n = x.numel() // width
    out = torch.zeros((2 * n, width), dtype=torch.uint8, device="cuda")
    out[1::2] = x.reshape(n, width)
    return out.reshape(-1)


def shape(n, L, reps, g):
    rnd = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=g)  # noqa: E731
    M, F = L + HDR, L + 90  # message and frame bytes
    plain, ckeys, cnonces, ids = rnd(n * L), rnd(n * 32), rnd(n * 12), rnd(n * 32)
    d_off = arange_offsets(n, L)
    store = E.Batch(plain, d_off, ckeys, cnonces, total_bytes_hint=n * L, max_len_hint=L)
    data = torch.zeros_like(plain)
    hashes = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    E.chunk_store(store, data, hashes, chunk_ids=ids)

    table = rnd(SESSIONS * 32)
    mid = torch.zeros(16 * SESSIONS, dtype=torch.int32, device="cuda")
    E.hmac_midstates(table, SESSIONS, mid)
    sess = torch.randint(0, SESSIONS, (n,), dtype=torch.int32, device="cuda", generator=g)
    fnonces = rnd(n * 12)
    ttl = torch.full((n,), TTL, dtype=torch.int32, device="cuda")
    f_off, m_off = arange_offsets(n, F), arange_offsets(n, M)
    skw = dict(session=sess, sessions=SESSIONS, mid=mid)

    # ---- upload: fused seal vs message assembly + wire_seal_sessions
    up = E.Batch(data, d_off, table, fnonces, total_bytes_hint=n * L, max_len_hint=L)
    frames = torch.zeros(n * F, dtype=torch.uint8, device="cuda")

    def fused_seal():
        E.chunk_frame_seal(up, frames, f_off, ids, ttl, **skw)

    hdr = torch.zeros((n, HDR), dtype=torch.uint8, device="cuda")
    hdr[:, 0], hdr[:, 1] = 4, 3
    hdr[:, 2:6] = torch.tensor(list(TTL.to_bytes(4, "big")), dtype=torch.uint8, device="cuda")
    hdr[:, 6:10] = torch.tensor(list(L.to_bytes(4, "big")), dtype=torch.uint8, device="cuda")
    hdr[:, 10:] = ids.reshape(n, 32)
    msgs = torch.zeros(n * M, dtype=torch.uint8, device="cuda")
    msgs.view(n, M)[:, :HDR] = hdr  # the headers are in place; every upload copies the data in
    frames2 = torch.zeros_like(frames)
    mb = E.Batch(msgs, m_off, table, fnonces, total_bytes_hint=n * M, max_len_hint=M)

    def assemble():
        msgs.view(n, M)[:, HDR:].copy_(data.view(n, L))

    def two_call_seal():
        assemble()
        E.wire_seal_sessions(mb, frames2, f_off, sess, SESSIONS, mid)

    fused_seal()
    two_call_seal()
    assert torch.equal(frames, frames2), "fused seal != wire_seal_sessions over the assembled messages"

    # ---- receive: fused open vs wire_open_sessions + chunk_fetch at +42
    rx = E.Batch(frames, f_off, table, None, total_bytes_hint=n * F, max_len_hint=F)
    pt, ct = torch.zeros(n * L, dtype=torch.uint8, device="cuda"), torch.zeros(n * L, dtype=torch.uint8, device="cuda")
    status = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    ttl_out = torch.zeros(n, dtype=torch.int32, device="cuda")

    def fused_open():
        E.chunk_frame_open(rx, pt, d_off, ids, ckeys, cnonces, hashes, status, data_out=ct, ttl_out=ttl_out, **skw)

    def fused_open_plain():  # the plaintext alone: no copy of the stored ciphertext
        E.chunk_frame_open(rx, pt, d_off, ids, ckeys, cnonces, hashes, status, **skw)

    msgs2 = torch.zeros(n * M, dtype=torch.uint8, device="cuda")
    back = torch.zeros(n * M, dtype=torch.uint8, device="cuda")
    macs = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    ok_w = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ok_f = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    split = torch.stack([m_off[:-1], m_off[:-1] + HDR], dim=1).reshape(-1)
    split = torch.cat([split, m_off[-1:]]).contiguous()  # message i = header record 2i, data record 2i+1
    order = torch.arange(1, 2 * n, 2, dtype=torch.int32, device="cuda")
    fb = E.Batch(msgs2, split, odd_rows(ckeys, 32), odd_rows(cnonces, 12), order=order, count=n,
                 total_bytes_hint=n * L, max_len_hint=L)
    ids2, hashes2 = odd_rows(ids, 32), odd_rows(hashes, 32)

    def two_call_open():
        E.wire_open_sessions(rx, msgs2, m_off, sess, SESSIONS, mid, macs, ok_w)
        E.chunk_fetch(fb, back, ids2, hashes2, ok_f)

    fused_open()
    assert int(status.sum()) == 0 and torch.equal(pt, plain) and torch.equal(ct, data)
    assert int((ttl_out != TTL).sum()) == 0
    pt.zero_()
    status.fill_(9)
    fused_open_plain()
    assert int(status.sum()) == 0 and torch.equal(pt, plain)
    two_call_open()
    assert int(ok_w.sum()) == n and int(ok_f[1::2].sum()) == n
    assert torch.equal(back.view(n, M)[:, HDR:].reshape(-1), plain)
    assert torch.equal(msgs2, msgs)

    fns = (fused_seal, two_call_seal, assemble, fused_open, fused_open_plain, two_call_open)
    for f in fns:
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    runs = {f.__name__: [] for f in fns}
    for _ in range(3):  # alternate, so that every form meets the same clocks
        for f in fns:
            runs[f.__name__].append(timed(f, reps, rounds=3))
    res = {"records": n, "data_bytes": L, "message_bytes": M, "frame_bytes": F}
    for k, v in runs.items():
        res[k + "_us"] = sorted(v)[1]
    gib = lambda us: n * F / (us * 1e-6) / 2**30  # noqa: E731
    for k in ("fused_seal", "two_call_seal", "fused_open", "fused_open_plain", "two_call_open"):
        res[k + "_frame_gib_s"] = gib(res[k + "_us"][0])
    res["open_fused_over_two_call"] = res["fused_open_us"][0] / res["two_call_open_us"][0]
    res["open_plain_fused_over_two_call"] = res["fused_open_plain_us"][0] / res["two_call_open_us"][0]
    res["seal_fused_over_two_call"] = res["fused_seal_us"][0] / res["two_call_seal_us"][0]
    return res


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    E.lib()
    g = torch.Generator(device="cuda").manual_seed(11)
    res = {"device": torch.cuda.get_device_name(0),
           "timing": "HIP events; per form the median of 3 alternating passes, each the median (min, max) of 3 rounds",
           "two_call_open": "wire_open_sessions, then chunk_fetch over the data records of the opened arena "
                            "(2n-entry offsets table + order), same stream",
           "two_call_seal": "device copy of the data into a message arena with the headers in place, then wire_seal_sessions",
           "ratios": "fused time / two-call time (below 1: the fused call is faster)",
           "shapes": []}
    for n, L, reps in SHAPES:
        res["shapes"].append(shape(n, L, reps, g))
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
