"""CPU tests of the Shamir key-share feature: the field (csrc/gf256.hpp) against the exp / log
definition, the scalar drop-in Shamir::split / Shamir::combine of libenet_crypto.so against the
compiled reference's recorded answers (tests/golden/shamir.json, made by
tools/gen_shamir_golden.py from src/crypto/Shamir.cpp), the reference's own test program on the
library alone, and the C ABI's argument checks (no GPU is touched by a rejected call)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import gf256_ref as G
from util import splitmix_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
CSRC = os.path.join(ROOT, "ephemeralnet_amd", "csrc")


@pytest.fixture(scope="module")
def shamir_golden():
    with open(os.path.join(ROOT, "tests", "golden", "shamir.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib_path():
    from ephemeralnet_amd import build as B
    return B.build(verbose=False)


@pytest.fixture(scope="module")
def api_bin(lib_path, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shamir") / "shamir_api")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shamir_api.cpp"), "-o", out,
                    "-L", os.path.dirname(lib_path), "-lenet_crypto", "-Wl,-rpath," + os.path.dirname(lib_path)],
                   check=True)
    return out


def run_ops(api_bin, ops):
    res = subprocess.run([api_bin], input="\n".join(ops) + "\n", capture_output=True, text=True, check=True,
                         timeout=120).stdout.splitlines()
    assert len(res) == len(ops)
    return res


def case_shares(golden, case):
    """The [index, value bytes] list of a golden combine case (values by share number or hex)."""
    src = None
    if case["split_case"]:
        src = next(s for s in golden["split"] if [s["threshold"], s["share_count"]] == case["split_case"])
    return [(i, bytes.fromhex(src["shares"][v - 1] if isinstance(v, int) else v)) for i, v in case["shares"]]


def test_gf256_header_matches_tables(tmp_path):
    """All 256 x 256 products, all inverses and the SWAR multiply of gf256.hpp (g++ alone)."""
    out = str(tmp_path / "gf256_table")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "gf256_table.cpp"), "-o", out], check=True)
    res = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr


def test_gf256_ref_matches_golden(shamir_golden):
    """The golden file pins the Python restatement: the recorded coefficients give the reference's
    shares, and its combine gives the reference's secrets."""
    assert shamir_golden["field_polynomial"] == G.POLY == 0x11D
    assert [(s["threshold"], s["share_count"]) for s in shamir_golden["split"]] == [
        (1, 1), (1, 5), (2, 3), (3, 5), (5, 8), (16, 16), (32, 40), (254, 254)]
    for s in shamir_golden["split"]:
        secret = np.frombuffer(bytes.fromhex(s["secret"]), np.uint8)
        coeffs = np.frombuffer(bytes.fromhex("".join(s["coeffs"])), np.uint8).reshape(1, -1, 32)
        assert len(s["coeffs"]) == s["threshold"] - 1 and len(s["shares"]) == s["share_count"]
        got = G.split(secret[None, :], coeffs, s["share_count"])[0]
        assert [row.tobytes().hex() for row in got] == s["shares"]
    kinds = set()
    for c in shamir_golden["combine"]:
        kinds.add(c["kind"])
        if c["throws"] or c["kind"] == "duplicate_zero":
            continue
        sh = case_shares(shamir_golden, c)[:c["threshold"]]
        sec, ok = G.combine(np.array([[i for i, _ in sh]], np.uint8),
                            np.array([[list(v) for _, v in sh]], np.uint8))
        assert ok[0] == 1 and sec[0].tobytes().hex() == c["secret"], c["kind"]
    assert kinds == {"first", "reversed", "subset", "extra", "duplicate", "too_few", "duplicate_zero"}


def test_scalar_combine_matches_reference(api_bin, shamir_golden):
    """Every golden combine: first-t, reversed, a shuffled non-prefix subset, garbage behind the
    threshold (ignored), and the reference's exceptions -- duplicate indices on non-zero values,
    too few shares -- but not duplicate indices on all-zero values (it returns zeros there)."""
    ops, want = [], []
    for c in shamir_golden["combine"]:
        ops.append(f"combine {c['threshold']} " + " ".join(f"{i}:{v.hex()}" for i, v in case_shares(shamir_golden, c)))
        want.append("throw" if c["throws"] else c["secret"])
    assert "throw" in want and bytes(32).hex() in want
    # index 0 is legal: the share at x = 0 is the secret itself
    s = next(x for x in shamir_golden["split"] if (x["threshold"], x["share_count"]) == (3, 5))
    ops.append(f"combine 3 0:{s['secret']} 2:{s['shares'][1]} 4:{s['shares'][3]}")
    want.append(s["secret"])
    ops.append(f"combine 0 1:{s['shares'][0]}")   # threshold 0: an empty subset sums to zero
    want.append(bytes(32).hex())
    assert run_ops(api_bin, ops) == want


def test_scalar_split_roundtrip_and_exceptions(api_bin, shamir_golden):
    """split -> combine for every golden (t, n) plus (255, 255) -- where the reference's loop never
    ends -- and (1, 255); the shares of a split lie on ONE polynomial of degree < t whose constant
    term is the secret (checked with gf256_ref); the reference's invalid_argument cases."""
    shapes = [(s["threshold"], s["share_count"]) for s in shamir_golden["split"]] + [(255, 255), (1, 255), (200, 255)]
    ops = [f"roundtrip {t} {n} {splitmix_bytes(5000 + t + n, 32).hex()}" for t, n in shapes]
    assert run_ops(api_bin, ops) == ["1"] * len(ops)
    ops, secrets = [], []
    for t, n in [(3, 5), (5, 8), (255, 255), (1, 255)]:
        secrets.append(bytes([0x00, 0xFF]) + splitmix_bytes(6000 + t, 30))
        ops.append(f"split {t} {n} {secrets[-1].hex()}")
    outs = run_ops(api_bin, ops)
    for (t, n), secret, line in zip([(3, 5), (5, 8), (255, 255), (1, 255)], secrets, outs):
        shares = [(int(a), bytes.fromhex(b)) for a, b in (x.split(":") for x in line.split())]
        assert [i for i, _ in shares] == list(range(1, n + 1))
        c = G.solve_coefficients([i for i, _ in shares[:t]], [np.frombuffer(v, np.uint8) for _, v in shares[:t]])
        assert c[0].tobytes() == secret
        again = G.split(np.frombuffer(secret, np.uint8)[None, :], c[1:][None, :, :], n)[0]
        assert [r.tobytes() for r in again] == [v for _, v in shares]
    assert run_ops(api_bin, [ops[0]])[0] != outs[0]   # fresh random coefficients every call
    z = bytes(32).hex()
    assert run_ops(api_bin, [f"split 0 3 {z}", f"split 0 0 {z}", f"split 1 0 {z}", f"split 4 3 {z}",
                             f"split 255 254 {z}"]) == ["throw"] * 5


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "tests", "shamir.cpp")),
                    reason="reference sources absent")
def test_reference_shamir_program_on_library_alone(lib_path, tmp_path):
    """The reference's own tests/shamir.cpp, asserts on, compiled where it lies against this
    repo's headers and linked with libenet_crypto.so ALONE (no reference Shamir object)."""
    out = str(tmp_path / "ref_shamir")
    subprocess.run(["g++", "-std=c++20", "-O2", "-I", os.path.join(ROOT, "include"),
                    os.path.join(REF, "tests", "shamir.cpp"), "-o", out,
                    "-L", os.path.dirname(lib_path), "-lenet_crypto", "-Wl,-rpath," + os.path.dirname(lib_path)],
                   check=True)
    defined = subprocess.run(["nm", "-C", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert "Shamir::split" not in defined and "Shamir::combine" not in defined
    res = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr


def test_shamir_abi_rejects_bad_arguments_without_gpu(lib_path):
    """enet_shamir_*_batch: NULL buffers, threshold 0, threshold > share_count, share_count > 255
    and misaligned 32-byte-row buffers return ENET_EINVAL; n == 0 is a no-op."""
    import ephemeralnet_amd as E
    L = E.lib()
    assert L.enet_abi_version() == (1 << 16) | 4
    raw = (C.c_uint8 * 4096)()
    base = (C.addressof(raw) + 15) & ~15     # 16-byte aligned host memory: never dereferenced
    a, b, c, d = base, base + 1024, base + 2048, base + 3072
    split, comb = L.enet_shamir_split_batch, L.enet_shamir_combine_batch
    for args in [(2, None, b, 3, 5, c), (2, a, None, 3, 5, c), (2, a, b, 3, 5, None),   # NULL buffers
                 (2, a, b, 0, 5, c), (2, a, b, 6, 5, c), (2, a, b, 3, 256, c), (2, a, b, 256, 256, c),
                 (2, a + 1, b, 3, 5, c), (2, a, b + 2, 3, 5, c), (2, a, b, 3, 5, c + 3)]:   # misaligned
        assert split(*args, None) == -1, args
        assert L.enet_last_error().startswith(b"shamir_split")
    for args in [(2, 3, None, b, c, d), (2, 3, a, None, c, d), (2, 3, a, b, None, d), (2, 3, a, b, c, None),
                 (2, 0, a, b, c, d), (2, 256, a, b, c, d), (2, 3, a, b + 1, c, d), (2, 3, a, b, c + 2, d)]:
        assert comb(*args, None) == -1, args
        assert L.enet_last_error().startswith(b"shamir_combine")
    assert split(0, None, None, 3, 5, None, None) == 0
    assert split(0, a, None, 1, 1, c, None) == 0
    assert comb(0, 3, None, None, None, None, None) == 0
