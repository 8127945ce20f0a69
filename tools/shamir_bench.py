"""Device timings of the batched Shamir calls (profiles/shamir_bench.json "device"): at 65 536
records, 3-of-5, with HIP events around `reps` back-to-back calls on one stream --
shamir_split and shamir_combine alone, and chunk_fetch of 4 KiB chunks alone against
shamir_combine -> chunk_fetch on the same stream, the two alternating.  Outputs are checked
(combine returns the split's secrets; both fetches return ok = 1 everywhere) before anything is
timed.  `python tools/shamir_bench.py [out.json]`; needs the MI355X."""
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ephemeralnet_amd as E  # noqa: E402

N, T, SC, L = 65536, 3, 5, 4096


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


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    E.lib()
    g = torch.Generator(device="cuda").manual_seed(7)
    rnd = lambda *shape: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g)  # noqa: E731
    keys, coeffs = rnd(N, 32), rnd(N, T - 1, 32)
    shares = torch.zeros((N, SC, 32), dtype=torch.uint8, device="cuda")
    E.shamir_split(keys, coeffs, T, SC, shares)
    indices = torch.tensor([5, 2, 3], dtype=torch.uint8, device="cuda").repeat(N, 1).contiguous()
    values = shares[:, [4, 1, 2], :].contiguous()
    combined = torch.zeros((N, 32), dtype=torch.uint8, device="cuda")
    ok_c = torch.zeros(N, dtype=torch.uint8, device="cuda")
    E.shamir_combine(indices, values, T, combined, ok_c)
    assert int(ok_c.sum()) == N and torch.equal(combined, keys)

    # a stored batch of 4 KiB chunks to fetch
    plain = rnd(N * L)
    offsets = torch.arange(0, (N + 1) * L, L, dtype=torch.int64, device="cuda")
    nonces, ids = rnd(N * 12), rnd(N * 32)
    b = E.Batch(plain, offsets, keys.reshape(-1), nonces, total_bytes_hint=N * L, max_len_hint=L)
    ct = torch.zeros_like(plain)
    hashes = torch.zeros(N * 32, dtype=torch.uint8, device="cuda")
    E.chunk_store(b, ct, hashes, chunk_ids=ids)
    back = torch.zeros_like(plain)
    ok_f = torch.zeros(N, dtype=torch.uint8, device="cuda")
    fetch_keys = dataclasses.replace(b, arena=ct)
    fetch_comb = dataclasses.replace(b, arena=ct, keys=combined.reshape(-1))

    def fetch_alone():
        E.chunk_fetch(fetch_keys, back, ids, hashes, ok_f)

    def combine_fetch():
        E.shamir_combine(indices, values, T, combined, ok_c)
        E.chunk_fetch(fetch_comb, back, ids, hashes, ok_f)

    for f in (fetch_alone, combine_fetch):
        ok_f.zero_()
        f()
        assert int(ok_f.sum()) == N and torch.equal(back, plain)

    res = {"records": N, "threshold": T, "share_count": SC, "chunk_bytes": L,
           "device": torch.cuda.get_device_name(0), "timing": "HIP events, median (min, max) of 5 rounds"}
    split = lambda: E.shamir_split(keys, coeffs, T, SC, shares)  # noqa: E731
    comb = lambda: E.shamir_combine(indices, values, T, combined, ok_c)  # noqa: E731
    for f in (split, comb, fetch_alone, combine_fetch):
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    res["shamir_split_us"] = timed(split, 200)
    res["shamir_combine_us"] = timed(comb, 200)
    fa, cf = [], []
    for _ in range(3):  # alternate the two fetch forms
        fa.append(timed(fetch_alone, 20, rounds=3))
        cf.append(timed(combine_fetch, 20, rounds=3))
    res["chunk_fetch_alone_us"] = sorted(fa)[1]
    res["combine_then_chunk_fetch_us"] = sorted(cf)[1]
    res["split_bytes_moved"] = N * 32 * (1 + (T - 1) + SC)
    res["combine_bytes_moved"] = N * (T + 32 * T + 32 + 1)
    res["fetch_alone_gib_s"] = N * L / (res["chunk_fetch_alone_us"][0] * 1e-6) / 2**30
    res["combine_adds_percent"] = 100.0 * (res["combine_then_chunk_fetch_us"][0] / res["chunk_fetch_alone_us"][0] - 1.0)
    text = json.dumps(res, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
