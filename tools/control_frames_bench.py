"""Device timings of the Request / Acknowledge frames and the frame triage
(profiles/control_frames_bench.json): the fused send (control_frame_seal: one launch, no input
arena) against wire_seal_sessions over a message arena built on the device, that arena's build on
its own (the composed path needs it, the fused one does not), the fused receive
(control_frame_open) against wire_open_sessions alone (the composed path still owes a host parse of
the messages, which is NOT in its figure), and frame_classify against wire_open_sessions over a
C3-like mixed receive batch (1 M frames of about 1 500 bytes, 90 % Chunk frames) -- what the triage
costs next to the opens it routes.  All sides in the same run, alternating, HIP events around
`reps` back-to-back calls, median of rounds.  Shapes: 65 536 and 1 048 576 control frames (half
Request, half Acknowledge) over 64 sessions.  Every output is checked (fused == composed, every
status 0, every kind as built) before anything is timed.
`python tools/control_frames_bench.py [out.json]`; needs the MI355X."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ephemeralnet_amd as E  # noqa: E402

SHAPES = [(65536, 20), (1 << 20, 5)]  # control frames, calls per timed round
MIXED = (1 << 20, 3)                  # frames of the mixed receive batch, calls per timed round
SESSIONS = 64
REQ, ACK = 66, 67


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


def alternate(fns, reps):
    for f in fns:
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    runs = {f.__name__: [] for f in fns}
    for _ in range(3):  # alternate, so that every form meets the same clocks
        for f in fns:
            runs[f.__name__].append(timed(f, reps, rounds=3))
    return {k + "_us": sorted(v)[1] for k, v in runs.items()}


def offsets_of(lens):
    return torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(lens.long(), 0)])


def session_table(g):
    table = torch.randint(0, 256, (SESSIONS * 32,), dtype=torch.uint8, device="cuda", generator=g)
    mid = torch.zeros(16 * SESSIONS, dtype=torch.int32, device="cuda")
    E.hmac_midstates(table, SESSIONS, mid)
    return table, mid


def control_shape(n, reps, g):
    """The first half of the batch are Requests, the second half Acknowledges (so the composed side's
    message arena is two dense blocks that plain tensor copies can fill)."""
    rnd = lambda *s: torch.randint(0, 256, s, dtype=torch.uint8, device="cuda", generator=g)  # noqa: E731
    h = n // 2
    table, mid = session_table(g)
    sess = torch.randint(0, SESSIONS, (n,), dtype=torch.int32, device="cuda", generator=g)
    skw = dict(session=sess, sessions=SESSIONS, mid=mid)
    kinds = torch.cat([torch.full((h,), 2, dtype=torch.uint8, device="cuda"), torch.full((n - h,), 4, dtype=torch.uint8, device="cuda")])
    mlen = torch.where(kinds == 2, REQ, ACK)
    m_off, f_off = offsets_of(mlen), offsets_of(mlen + 48)
    cids, local, fnonces = rnd(n, 32), rnd(32), rnd(n * 12)
    accepted = (rnd(n) & 1).contiguous()
    mbytes, fbytes = int(m_off[-1]), int(f_off[-1])

    tx = E.Batch(None, f_off, table, fnonces)
    frames = torch.zeros(fbytes, dtype=torch.uint8, device="cuda")
    st_seal = torch.full((n,), 9, dtype=torch.uint8, device="cuda")

    def fused_seal():
        E.control_frame_seal(tx, frames, f_off, kinds, cids, local, st_seal, accepted=accepted, **skw)

    msgs = torch.zeros(mbytes, dtype=torch.uint8, device="cuda")
    req, ack = msgs[:h * REQ].view(h, REQ), msgs[h * REQ:].view(n - h, ACK)

    def build_messages():
        req[:, 0], req[:, 1] = 4, 2
        req[:, 2:34], req[:, 34:66] = cids[:h], local
        ack[:, 0], ack[:, 1], ack[:, 2] = 4, 4, accepted[h:]
        ack[:, 3:35], ack[:, 35:67] = cids[h:], local

    frames2 = torch.zeros_like(frames)
    mb = E.Batch(msgs, m_off, table, fnonces, total_bytes_hint=mbytes, max_len_hint=ACK)

    def composed_seal():
        E.wire_seal_sessions(mb, frames2, f_off, sess, SESSIONS, mid)

    rx = E.Batch(frames, f_off, table, None, total_bytes_hint=fbytes, max_len_hint=ACK + 48)
    cid_out, pid_out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda"), torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    info = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    st_open = torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    senders = local.repeat(n)

    def fused_open():
        E.control_frame_open(rx, cid_out, info, st_open, peer_ids_out=pid_out, sender_ids=senders, **skw)

    back = torch.zeros(mbytes, dtype=torch.uint8, device="cuda")
    macs = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    ok_w = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def wire_open_alone():
        E.wire_open_sessions(rx, back, m_off, sess, SESSIONS, mid, macs, ok_w)

    kind = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lists = torch.zeros((5, n), dtype=torch.int32, device="cuda")
    counts = torch.zeros(5, dtype=torch.int32, device="cuda")

    def classify():
        E.frame_classify(rx, kind, lists, counts, session=sess, sessions=SESSIONS)

    # ---- every output, before anything is timed
    fused_seal()
    build_messages()
    composed_seal()
    assert int(st_seal.sum()) == 0 and torch.equal(frames, frames2), "fused seal != wire_seal_sessions over the built arena"
    fused_open()
    wire_open_alone()
    assert int(st_open.sum()) == 0 and int(ok_w.sum()) == n and torch.equal(back, msgs)
    assert torch.equal(cid_out, cids) and torch.equal(pid_out, local.expand(n, 32))
    want = torch.stack([torch.full((n,), 4, dtype=torch.uint8, device="cuda"), kinds, torch.where(kinds == 4, accepted, 0).to(torch.uint8),
                        torch.ones(n, dtype=torch.uint8, device="cuda")], dim=1)
    assert torch.equal(info, want)
    classify()
    assert torch.equal(kind, kinds) and counts.tolist() == [0, h, 0, n - h, 0]

    res = {"records": n, "frame_bytes": fbytes, "message_bytes": mbytes}
    res.update(alternate((fused_seal, composed_seal, build_messages, fused_open, wire_open_alone, classify), reps))
    us = lambda k: res[k + "_us"][0]  # noqa: E731
    for k in ("fused_seal", "composed_seal", "fused_open", "wire_open_alone", "classify"):
        res[k + "_mframes_s"] = n / us(k)
    res["seal_fused_over_composed"] = us("fused_seal") / us("composed_seal")
    res["seal_fused_over_composed_with_build"] = us("fused_seal") / (us("composed_seal") + us("build_messages"))
    res["open_fused_over_wire_open"] = us("fused_open") / us("wire_open_alone")
    return res


def mixed_shape(n, reps, g):
    """Record i is a Request when i % 20 == 0, an Acknowledge when i % 20 == 1, else a Chunk message
    with 1 458 data bytes (|m| = 1 500); sealed on the device, so every frame is authentic."""
    table, mid = session_table(g)
    sess = torch.randint(0, SESSIONS, (n,), dtype=torch.int32, device="cuda", generator=g)
    i = torch.arange(n, device="cuda") % 20
    types = torch.where(i == 0, 2, torch.where(i == 1, 4, 3)).to(torch.uint8)
    mlen = torch.where(i == 0, REQ, torch.where(i == 1, ACK, 1500))
    m_off, f_off = offsets_of(mlen), offsets_of(mlen + 48)
    mbytes, fbytes = int(m_off[-1]), int(f_off[-1])
    msgs = torch.randint(0, 256, (mbytes,), dtype=torch.uint8, device="cuda", generator=g)
    msgs[m_off[:-1]] = 4
    msgs[m_off[:-1] + 1] = types
    fnonces = torch.randint(0, 256, (n * 12,), dtype=torch.uint8, device="cuda", generator=g)
    frames = torch.zeros(fbytes, dtype=torch.uint8, device="cuda")
    E.wire_seal_sessions(E.Batch(msgs, m_off, table, fnonces), frames, f_off, sess, SESSIONS, mid)
    rx = E.Batch(frames, f_off, table, None, total_bytes_hint=fbytes, max_len_hint=1548)
    kind = torch.zeros(n, dtype=torch.uint8, device="cuda")
    lists = torch.zeros((5, n), dtype=torch.int32, device="cuda")
    counts = torch.zeros(5, dtype=torch.int32, device="cuda")
    back = torch.zeros(mbytes, dtype=torch.uint8, device="cuda")
    macs = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    ok_w = torch.zeros(n, dtype=torch.uint8, device="cuda")

    def classify():
        E.frame_classify(rx, kind, lists, counts, session=sess, sessions=SESSIONS)

    def wire_open_alone():
        E.wire_open_sessions(rx, back, m_off, sess, SESSIONS, mid, macs, ok_w)

    classify()
    wire_open_alone()
    assert torch.equal(kind, types) and int(ok_w.sum()) == n and torch.equal(back, msgs)
    assert counts.tolist() == [0, int((types == 2).sum()), int((types == 3).sum()), int((types == 4).sum()), 0]
    res = {"records": n, "frame_bytes": fbytes, "chunk_share": float((types == 3).float().mean())}
    res.update(alternate((classify, wire_open_alone), reps))
    res["classify_over_wire_open"] = res["classify_us"][0] / res["wire_open_alone_us"][0]
    res["classify_mframes_s"] = n / res["classify_us"][0]
    return res


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    E.lib()
    g = torch.Generator(device="cuda").manual_seed(17)
    res = {"device": torch.cuda.get_device_name(0),
           "timing": "HIP events; per form the median of 3 alternating passes, each the median (min, max) of 3 rounds",
           "composed_seal": "wire_seal_sessions over a pre-built message arena; build_messages is that arena assembled "
                            "on the device by tensor copies (the fused seal needs none)",
           "wire_open_alone": "wire_open_sessions; the host parse of its messages that the composed receive still owes "
                              "is not in this figure",
           "ratios": "fused time / composed time (below 1: the fused call is faster)",
           "shapes": [], "mixed": None}
    for n, reps in SHAPES:
        res["shapes"].append(control_shape(n, reps, g))
        torch.cuda.empty_cache()
    res["mixed"] = mixed_shape(*MIXED, g)
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
