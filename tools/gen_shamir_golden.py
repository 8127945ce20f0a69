"""Make tests/golden/shamir.json from the compiled reference (run once, where a reference checkout
exists: `python tools/gen_shamir_golden.py [reference root]`).

tools/shamir_golden.cpp is compiled against the reference's own include/ and src/crypto/Shamir.cpp
where they lie.  The reference's split is random, so each split case is pinned through its
polynomial: the threshold-1 coefficient rows are recovered by solving the Vandermonde system over
the first `threshold` shares (tests/gf256_ref.py), and this script asserts that they reproduce
EVERY share the reference produced and that the constant term is the secret.  The combine cases
(first-t, reversed, a shuffled non-prefix subset, more shares than threshold with garbage behind,
duplicate indices) record what the reference's own combine returned, or that it threw; a share
is [index, value] with the value either the number of the split case's share that holds it or hex."""
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import gf256_ref as G  # noqa: E402
from util import splitmix_bytes  # noqa: E402

CASES = [(1, 1), (1, 5), (2, 3), (3, 5), (5, 8), (16, 16), (32, 40), (254, 254)]


def tok(index, value):
    return f"{index}:{value.hex()}"


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "shamir_golden")
        subprocess.run(["g++", "-O2", "-std=c++20", "-I", os.path.join(ref, "include"),
                        os.path.join(ROOT, "tools", "shamir_golden.cpp"),
                        os.path.join(ref, "src", "crypto", "Shamir.cpp"), "-o", exe], check=True)

        def run(ops):
            out = subprocess.run([exe], input="\n".join(ops) + "\n", capture_output=True, text=True,
                                 check=True).stdout.splitlines()
            assert len(out) == len(ops)
            return out

        secrets = []
        for k, (t, n) in enumerate(CASES):
            s = bytearray(splitmix_bytes(77000 + k, 32))
            if (t, n) == (3, 5):
                s[0], s[1], s[30], s[31] = 0x00, 0xFF, 0xFF, 0x00
            secrets.append(bytes(s))
        res = run([f"split {t} {n} {s.hex()}" for (t, n), s in zip(CASES, secrets)])

        split_cases, combine_ops, combine_meta = [], [], []
        rng = random.Random(20240607)
        for (t, n), secret, line in zip(CASES, secrets, res):
            shares = [(int(a), bytes.fromhex(b)) for a, b in (x.split(":") for x in line.split())]
            assert [i for i, _ in shares] == list(range(1, n + 1))
            xs = [i for i, _ in shares[:t]]
            c = G.solve_coefficients(xs, [np.frombuffer(v, np.uint8) for _, v in shares[:t]])
            assert c[0].tobytes() == secret, "constant term is not the secret"
            again = G.split(np.frombuffer(secret, np.uint8)[None, :], c[1:][None, :, :], n)[0]
            for j, (_, v) in enumerate(shares):
                assert again[j].tobytes() == v, f"coefficients do not reproduce share {j + 1} of {(t, n)}"
            split_cases.append({"threshold": t, "share_count": n, "secret": secret.hex(),
                                "shares": [v.hex() for _, v in shares],
                                "coeffs": [row.tobytes().hex() for row in c[1:]]})

            def add(kind, sel, threshold=t):
                combine_ops.append(f"combine {threshold} " + " ".join(tok(i, v) for i, v in sel))
                # a value the split case holds is recorded as its share number, anything else as hex
                number = {v: j + 1 for j, (_, v) in enumerate(shares)}
                combine_meta.append({"kind": kind, "threshold": threshold, "split_case": [t, n],
                                     "shares": [[i, number.get(v, v.hex())] for i, v in sel]})

            add("first", shares[:t])
            add("reversed", shares[:t][::-1])
            if n > t:
                sub = shares[1:]          # never the prefix: drops share 1
                rng.shuffle(sub)
                add("subset", sub[:t])
                garbage = [(rng.randrange(256), splitmix_bytes(78000 + 10 * t + g, 32)) for g in range(2)]
                add("extra", sub[:t] + garbage)
            if t >= 2:
                dup = list(shares[:t])
                dup[1] = (dup[0][0], dup[1][1])
                add("duplicate", dup)
                add("too_few", shares[:t - 1])
        # duplicate indices on all-zero values: the reference never divides and returns zeros
        combine_ops.append("combine 2 " + tok(7, bytes(32)) + " " + tok(7, bytes(32)))
        combine_meta.append({"kind": "duplicate_zero", "threshold": 2, "split_case": None,
                             "shares": [[7, bytes(32).hex()], [7, bytes(32).hex()]]})
        out = run(combine_ops)
        by_case = {(s["threshold"], s["share_count"]): s["secret"] for s in split_cases}
        for meta, got in zip(combine_meta, out):
            meta["throws"] = got == "throw"
            meta["secret"] = None if meta["throws"] else got
            if meta["kind"] in ("first", "reversed", "subset", "extra"):
                assert got == by_case[tuple(meta["split_case"])], meta["kind"]   # the reference's own combine
            if meta["kind"] in ("duplicate", "too_few"):
                assert meta["throws"], meta["kind"]
    dst = os.path.join(ROOT, "tests", "golden", "shamir.json")
    with open(dst, "w") as f:
        json.dump({"field_polynomial": G.POLY, "split": split_cases, "combine": combine_meta}, f, indent=0)
        f.write("\n")
    print(dst, os.path.getsize(dst), "bytes;", len(split_cases), "split cases,", len(combine_meta), "combine cases")


if __name__ == "__main__":
    main()
