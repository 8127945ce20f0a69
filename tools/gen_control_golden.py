"""Make tests/golden/control_frames.json from the compiled reference (run once, where a reference
checkout exists: `python tools/gen_control_golden.py [reference root]`; default: a `reference`
directory beside this repository).

tools/control_golden.cpp is compiled against the reference's own include/ and its
src/protocol/Message.cpp, src/core/Types.cpp and src/crypto/*.cpp where they lie.  Every recorded
signed message is the reference's own protocol::encode_signed output (or its HmacSha256 over bytes
encode cannot make), every verdict and parsed field its decode_signed's, every frame body its
ChaCha20::apply's."""
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from util import splitmix_bytes  # noqa: E402


def hx(b: bytes) -> str:
    return b.hex() if b else "-"


def unhx(s: str) -> bytes:
    return b"" if s == "-" else bytes.fromhex(s)


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "control_golden")
        subprocess.run(["g++", "-O2", "-std=c++20", "-I", os.path.join(ref, "include"),
                        os.path.join(ROOT, "tools", "control_golden.cpp"),
                        os.path.join(ref, "src", "protocol", "Message.cpp"),
                        os.path.join(ref, "src", "core", "Types.cpp")]
                       + sorted(glob.glob(os.path.join(ref, "src", "crypto", "*.cpp"))) + ["-o", exe], check=True)

        def run(ops):
            out = subprocess.run([exe], input="\n".join(ops) + "\n", capture_output=True, text=True,
                                 check=True).stdout.splitlines()
            assert len(out) == len(ops) and "?" not in out
            return out

        def decode(signed: bytes, key: bytes):
            r = run([f"decode {hx(signed)} {hx(key)}"])[0].split()
            if r[0] == "none":
                return {"decodes": False}
            if r[0] == "other":
                return {"decodes": True, "type": int(r[1])}
            if r[0] == "request":
                return {"decodes": True, "type": 2, "version": int(r[1]), "accepted": 0, "chunk_id": r[2], "peer_id": r[3]}
            return {"decodes": True, "type": 4, "version": int(r[1]), "accepted": int(r[2]), "chunk_id": r[3],
                    "peer_id": r[4]}

        # encode_signed as given: versions 0..5, both kinds, both accepted values
        cases = []
        n = 0
        for version in range(6):
            for kind, accepted in ((2, 0), (4, 0), (4, 1)):
                s = 81000 + 10 * n
                n += 1
                key, cid, pid = splitmix_bytes(s, 32), splitmix_bytes(s + 1, 32), splitmix_bytes(s + 2, 32)
                op = (f"request {version} {hx(cid)} {hx(pid)} {hx(key)}" if kind == 2
                      else f"ack {version} {accepted} {hx(cid)} {hx(pid)} {hx(key)}")
                signed = unhx(run([op])[0])
                cases.append({"name": f"encode {'request' if kind == 2 else 'ack'} v{version} a{accepted}",
                              "version_in": version, "kind": kind, "accepted": accepted, "chunk_id": cid.hex(),
                              "peer_id": pid.hex(), "key": key.hex(), "signed": signed.hex(),
                              "decoded": decode(signed, key)})

        # bytes encode cannot make, signed by the reference's HmacSha256
        def resigned(name, m: bytes, key: bytes):
            signed = unhx(run([f"sign {hx(m)} {hx(key)}"])[0])
            return {"name": name, "key": key.hex(), "signed": signed.hex(), "decoded": decode(signed, key)}

        by = {c["name"]: c for c in cases}
        mutations = []
        for label in ("request v4 a0", "ack v4 a1"):
            c = by["encode " + label]
            m, k = bytes.fromhex(c["signed"])[:-32], bytes.fromhex(c["key"])
            for t in (0x00, 0x01, 0x03, 0x05, 0x06, 0x02 if c["kind"] == 4 else 0x04, 0xFF):
                mutations.append(resigned(f"{label} with type {t:#04x}", m[:1] + bytes([t]) + m[2:], k))
            for v in (0, 5):
                mutations.append(resigned(f"{label} with version byte {v}", bytes([v]) + m[1:], k))
            mutations.append(resigned(f"{label} one byte short", m[:-1], k))
            mutations.append(resigned(f"{label} one byte long", m + b"\x5a", k))
            bad = bytearray(bytes.fromhex(c["signed"]))
            bad[-1] ^= 1
            mutations.append({"name": f"{label} with a flipped MAC bit", "key": k.hex(), "signed": bytes(bad).hex(),
                              "decoded": decode(bytes(bad), k)})
        c = by["encode ack v4 a1"]
        m, k = bytes.fromhex(c["signed"])[:-32], bytes.fromhex(c["key"])
        mutations.append(resigned("ack v4 with accepted byte 2", m[:2] + b"\x02" + m[3:], k))

        # frames under fixed nonces: body = ChaCha20::apply(key, nonce, signed) (SessionManager.cpp:362-374)
        frames = []
        for i, c in enumerate([by["encode request v4 a0"], by["encode request v0 a0"], by["encode ack v4 a1"],
                               by["encode ack v2 a0"]]):
            nonce = splitmix_bytes(83000 + i, 12)
            body = run([f"chacha {c['key']} {nonce.hex()} {c['signed']}"])[0]
            frames.append({"case": c["name"], "key": c["key"], "nonce": nonce.hex(), "signed": c["signed"], "body": body})

    about = ("Request / Acknowledge frame golden vectors; generator tools/gen_control_golden.py + "
             "tools/control_golden.cpp (reference Message.cpp / Types.cpp / src/crypto compiled where they lie). "
             "Inputs: tests/util.py splitmix_bytes.")
    dst = os.path.join(ROOT, "tests", "golden", "control_frames.json")
    with open(dst, "w") as f:
        json.dump({"_about": about, "cases": cases, "mutations": mutations, "frames": frames}, f, indent=1)
        f.write("\n")
    print(dst, os.path.getsize(dst), "bytes;", len(cases), "cases,", len(mutations), "mutations,", len(frames), "frames")


if __name__ == "__main__":
    main()
