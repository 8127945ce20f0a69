"""bench.py's plain run, --full and --dump-outputs.  CPU: the options parse and the dump helper
writes float32 files, a buffer past DUMP_SAMPLE as the same sorted positions every time.  GPU:
one plain run at a small shape prints the headline keys without the --full measurements, and the
dumped arrays are what the timed path computed -- the oracle's ciphertext and tags of the seeded
inputs, every verdict 1, the opened bytes equal to the plaintext."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FULL_ONLY = ("seal_ms", "open_ms", "roofline", "valu_roofline", "power", "long_records",
             "host_resident", "cpu_baseline", "cpu_reference")


def test_full_and_dump_options_parse(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "d")
    for bad in (["--steps", "0"], ["--dump-outputs", "d", "--mode", "pow"], ["--dump-outputs", "d", "--c5"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + bad)
        with pytest.raises(SystemExit):
            bench.parse()


def test_dump_outputs_float32_and_fixed_sample(tmp_path, monkeypatch):
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    big = (torch.arange(50000, dtype=torch.int64) * 7 % 251).to(torch.uint8)
    small = torch.arange(1000, dtype=torch.int64).to(torch.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a_big, a_small = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "small.npy")
    assert a_big.dtype == a_small.dtype == np.float32
    assert np.array_equal(a_small, small.numpy().astype(np.float32))  # at the cap: written whole
    assert a_big.shape == (1000,) and np.array_equal(a_big, np.load(tmp_path / "b" / "big.npy"))
    # the sample is bytes of the buffer at non-decreasing positions: it embeds in order
    src, j = big.numpy().tolist(), 0
    for v in a_big.tolist():
        while j < len(src) and src[j] != v:
            j += 1
        assert j < len(src)
    assert len(set(a_big.tolist())) > 100  # not one position repeated


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    import torch
    n, L, steps = 256, 4096, 3
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--prewarm-s", "0", "--records", str(n), "--record-bytes", str(L),
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["unit"] == "GiB/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(n * L / (d["ms_per_step"] * 1e-3) / 2**30, rel=0.02)
    assert not [k for k in FULL_ONLY if k in d]
    assert sorted(os.listdir(out)) == ["ciphertext.npy", "ok.npy", "opened.npy", "tags.npy"]
    arr = {k: np.load(out / (k + ".npy")) for k in ("ciphertext", "ok", "opened", "tags")}
    assert all(a.dtype == np.float32 for a in arr.values())
    # the inputs bench.py draws (seed 1234 + rank, in this order)
    g = torch.Generator(device="cuda").manual_seed(1234)
    pt, keys, nonces = (torch.randint(0, 256, (n * k,), dtype=torch.uint8, device="cuda", generator=g).cpu().numpy()
                        for k in (L, 32, 12))
    assert np.array_equal(arr["ok"], np.ones(n, np.float32))
    assert np.array_equal(arr["opened"], pt.astype(np.float32))
    for i in (0, 1, n // 2, n - 1):
        c, t = oracle.aead_seal(keys[32 * i:32 * i + 32].tobytes(), nonces[12 * i:12 * i + 12].tobytes(),
                                pt[L * i:L * i + L].tobytes())
        assert arr["ciphertext"][L * i:L * i + L].astype(np.uint8).tobytes() == c, f"record {i}"
        assert arr["tags"][16 * i:16 * i + 16].astype(np.uint8).tobytes() == t, f"record {i}"
