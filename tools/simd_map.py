#!/usr/bin/env python3
"""Where the 12 waves of a stream-kernel workgroup sit: one seal of the C2 shape with the
ENET_STREAM_DBG=32768 probe (stream.hip stream_where: every wave's entry shader clock and HW_ID
in the workgroup's tag slots), summarised over all workgroups.

Needs the tools build with the kernel probes (python -m ephemeralnet_amd.build --tools --probes):
    ENET_LIB_PATH=ephemeralnet_amd/libenet_crypto_tools.so ENET_STREAM_DBG=32768 \
        python tools/simd_map.py [--records 65536] > profiles/stream_simd_map.json

HW_ID (gfx9): wave slot [3:0], SIMD [5:4], CU [11:8], SH [12], SE [15:13].  The probe launch
computes no tags (its ciphertext is not checked here either).
"""
import argparse
import collections
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=65536)
    ap.add_argument("--record-bytes", type=int, default=4096)
    a = ap.parse_args()
    if os.environ.get("ENET_STREAM_DBG") != "32768" or not os.environ.get("ENET_LIB_PATH"):
        raise SystemExit("run with ENET_LIB_PATH=<tools build with probes> ENET_STREAM_DBG=32768")
    import numpy as np
    import torch

    import ephemeralnet_amd as E
    n, L = a.records, a.record_bytes
    lanes = E.lanes_per_record(n, n * L, L)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1)
    pt = torch.randint(0, 256, (n * L,), dtype=torch.uint8, device=dev, generator=g)
    keys = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device=dev, generator=g)
    nonces = torch.randint(0, 256, (n * 12,), dtype=torch.uint8, device=dev, generator=g)
    offs = torch.arange(0, (n + 1) * L, L, dtype=torch.int64, device=dev)
    ct = torch.empty_like(pt)
    tags = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    b = E.Batch(pt, offs, keys, nonces, total_bytes_hint=n * L, max_len_hint=L)
    E.aead_seal(b, ct, tags)  # warm-up launch; the second one's stamps are read
    tags.zero_()
    E.aead_seal(b, ct, tags)
    torch.cuda.synchronize()
    raw = tags.cpu().numpy().view(np.uint32).reshape(-1, 4)
    # workgroup g's slots start at record g * (512 / lanes): find the stride from the stamps
    # themselves (word 3 = wave number 0..11 in 12 consecutive slots)
    starts = [i for i in range(0, len(raw) - 11) if all(raw[i + w][3] == w for w in range(12))
              and (raw[i][0] or raw[i][1])]
    if not starts:
        raise SystemExit("no stamps found: is the library a tools build with probes?")
    same_simd = older_first = slots_in_order = 0
    simd_of_wave = collections.Counter()
    young_after = []
    example = None
    for s in starts:
        w = raw[s:s + 12]
        t = [(int(x[1]) << 32) | int(x[0]) for x in w]
        simd = [(int(x[2]) >> 4) & 3 for x in w]
        slot = [int(x[2]) & 15 for x in w]
        cu = {(int(x[2]) >> 8) & 0xff for x in w}
        ok = len(cu) == 1 and all(simd[k] == simd[k + 4] == simd[k + 8] for k in range(4)) \
            and len(set(simd[:4])) == 4
        same_simd += ok
        older = all(t[k] <= t[k + 4] <= t[k + 8] for k in range(4))
        older_first += older
        slots_in_order += slot == [0] * 4 + [1] * 4 + [2] * 4
        young_after.append(sum(t[k + 4] - t[k] for k in range(4)) / 4)
        simd_of_wave.update((k, simd[k]) for k in range(12))
        if example is None:
            example = {"first_slot": s, "simd": simd, "wave_slot": slot,
                       "entry_clock_minus_wave0": [x - t[0] for x in t]}
    out = {
        "what": "stream_kernel<1, 1, 0> (seal), one launch, ENET_STREAM_DBG=32768: HW_ID and entry "
                "shader clock of every wave of every workgroup",
        "config": {"records": n, "record_bytes": L, "lanes": lanes},
        "workgroups": len(starts),
        "waves_k_k4_k8_share_a_simd_and_0_3_cover_all_four": same_simd,
        "wave_slots_0_for_waves_0_3_then_1_for_4_7_then_2_for_8_11": slots_in_order,
        "entry_clock_order_k_then_k4_then_k8_on_every_simd": older_first,
        "mean_entry_delay_of_waves_4_7_behind_0_3_shader_clock_ticks": round(float(np.mean(young_after)), 1),
        "simd_of_wave_counts": {f"wave{k}": {str(sd): c for (kk, sd), c in sorted(simd_of_wave.items()) if kk == k}
                                for k in range(12)},
        "example_workgroup": example,
    }
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
