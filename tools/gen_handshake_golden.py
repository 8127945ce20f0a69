"""Make tests/golden/handshake.json from the compiled reference (run once, where a reference
checkout exists: `python tools/gen_handshake_golden.py [reference root]`).

tools/handshake_golden.cpp is compiled against the reference's own include/ and its
src/network/KeyExchange.cpp, src/network/KeyManager.cpp, src/core/Types.cpp and src/crypto/*.cpp
where they lie.  Every recorded public, shared secret, material key and rotated key is what the
reference's own KeyExchange / KeyManager returned.  KeyExchange::modexp is private, so the scalar
of a case is the restatement's (tests/handshake_ref.py) and this script asserts that the
reference's Sha256 of its four big-endian bytes IS the reference's shared secret.  The handshake
PoW digest lives in an anonymous namespace of src/core/Node.cpp (not linkable): as in
tests/golden/gen_pow_golden.py its serialisation (Node.cpp:232-244) is restated and hashed by the
reference's Sha256."""
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import handshake_ref as H  # noqa: E402
from util import splitmix_bytes  # noqa: E402

P = H.P
U32 = 2**32 - 1


def u32(seed):
    return int.from_bytes(splitmix_bytes(seed, 4), "little")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "handshake_golden")
        subprocess.run(["g++", "-O2", "-std=c++20", "-I", os.path.join(ref, "include"),
                        os.path.join(ROOT, "tools", "handshake_golden.cpp"),
                        os.path.join(ref, "src", "network", "KeyExchange.cpp"),
                        os.path.join(ref, "src", "network", "KeyManager.cpp"),
                        os.path.join(ref, "src", "core", "Types.cpp")]
                       + sorted(glob.glob(os.path.join(ref, "src", "crypto", "*.cpp"))) + ["-o", exe], check=True)

        def run(ops):
            out = subprocess.run([exe], input="\n".join(ops) + "\n", capture_output=True, text=True,
                                 check=True).stdout.splitlines()
            assert len(out) == len(ops) and "?" not in out
            return out

        # (local private, remote): remote = ("priv", x) the public of private x, or ("pub", v) a raw value
        pairs = [(123456789, ("priv", 987654321)), (987654321, ("priv", 123456789)),
                 (0, ("priv", 77)), (1, ("priv", 78)), (U32, ("priv", 79)), (79, ("priv", U32)),
                 (424242, ("priv", 424242)),                      # equal publics
                 (0, ("pub", 0)), (5, ("pub", 0)), (6, ("pub", 1)), (7, ("pub", 2)), (8, ("pub", P - 1)),
                 (9, ("pub", P)), (10, ("pub", P + 1)), (11, ("pub", U32)), (U32, ("pub", U32)),
                 (1, ("pub", P - 1)), (0, ("pub", P))]
        for k in range(8):
            pairs.append((u32(91000 + k), ("priv", u32(91100 + k))))
        # a scalar whose top byte is zero, from ordinary keys (BE32 must keep the leading zero)
        k = 0
        while True:
            a, b = u32(92000 + k) % (P - 3) + 2, u32(93000 + k) % (P - 3) + 2
            if 1 < H.shared_scalar(a, H.compute_public(b)) < 2**24:
                pairs.append((a, ("priv", b)))
                break
            k += 1

        cases = []
        for n, (priv, (kind, v)) in enumerate(pairs):
            local_public = int(run([f"public {priv}"])[0])
            remote_private = v if kind == "priv" else None
            remote_public = int(run([f"public {v}"])[0]) if kind == "priv" else v
            secret = run([f"secret {priv} {remote_public}"])[0]
            scalar = H.shared_scalar(priv, remote_public)
            assert run([f"sha {scalar.to_bytes(4, 'big').hex()}"])[0] == secret, "scalar does not give the secret"
            if remote_private is not None:   # both peers agree
                assert run([f"secret {remote_private} {local_public}"])[0] == secret
            material = H.handshake_material(local_public, remote_public)
            ticks = int.from_bytes(splitmix_bytes(94000 + n, 7), "little") + 2_000_000_000
            key, rotated = run([f"material {secret} {material.hex()}", f"rotate {secret} 0 {ticks}"])
            cases.append({"local_private": priv, "local_public": local_public, "remote_private": remote_private,
                          "remote_public": remote_public,
                          "remote_valid": run([f"valid {remote_public}"])[0] == "1",
                          "scalar": scalar, "secret": secret, "material": material.hex(), "material_key": key,
                          "rotate_ticks": ticks, "rotate_counter": 1, "rotated_key": rotated})
        assert run([f"rotate {cases[0]['secret']} 0 999999999"])[0] == "none"   # one ns short of the interval
        assert run([f"rotate {cases[0]['secret']} 5 1000000005"])[0] != "none"  # exactly the interval

        pows = []
        for n in range(12):
            s = 95000 + 10 * n
            init, resp = splitmix_bytes(s, 32), splitmix_bytes(s + 1, 32)
            pub = [u32(s + 2), 0, 2, P - 1, U32][n % 5] if n >= 7 else u32(s + 2)
            nonce = [0, 1, 2**64 - 1, 2**63][n % 4] if n < 4 else int.from_bytes(splitmix_bytes(s + 3, 8), "little")
            digest = run([f"sha {H.pow_message(init, resp, pub, nonce).hex()}"])[0]
            pows.append({"initiator": init.hex(), "responder": resp.hex(), "public": pub, "nonce": nonce,
                         "digest": digest, "leading_zero_bits": H.leading_zero_bits(bytes.fromhex(digest))})
        # solved nonces: found with the restatement, digest by the reference
        for n, diff in enumerate([1, 4, 8, 12]):
            s = 96000 + 10 * n
            init, resp, pub = splitmix_bytes(s, 32), splitmix_bytes(s + 1, 32), u32(s + 2) % (P - 3) + 2
            nonce = H.solve_pow(init, resp, pub, diff, start=u32(s + 3))
            digest = run([f"sha {H.pow_message(init, resp, pub, nonce).hex()}"])[0]
            assert H.leading_zero_bits(bytes.fromhex(digest)) >= diff
            pows.append({"initiator": init.hex(), "responder": resp.hex(), "public": pub, "nonce": nonce,
                         "digest": digest, "leading_zero_bits": H.leading_zero_bits(bytes.fromhex(digest))})

    about = ("handshake golden vectors; generator tools/gen_handshake_golden.py + tools/handshake_golden.cpp "
             "(reference KeyExchange.cpp / KeyManager.cpp / src/crypto compiled where they lie; the Node.cpp PoW "
             "serialisation restated and hashed by the reference Sha256; scalars restated and checked against the "
             "reference's secrets). Inputs: tests/util.py splitmix_bytes.")
    dst = os.path.join(ROOT, "tests", "golden", "handshake.json")
    with open(dst, "w") as f:
        json.dump({"_about": about, "prime": P, "generator": H.G, "cases": cases, "handshake_pow": pows}, f, indent=1)
        f.write("\n")
    print(dst, os.path.getsize(dst), "bytes;", len(cases), "cases,", len(pows), "PoW digests")


if __name__ == "__main__":
    main()
