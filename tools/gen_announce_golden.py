"""Make tests/golden/announce_frames.json from the compiled reference (run once, where a reference
checkout exists: `python tools/gen_announce_golden.py [reference root]`; default: a `reference`
directory beside this repository).

tools/announce_golden.cpp is compiled against the reference's own include/ and its
src/protocol/Message.cpp, src/protocol/Manifest.cpp, src/core/Types.cpp and src/crypto/*.cpp where
they lie.  Every recorded signed message is the reference's own protocol::encode_signed output (or
its HmacSha256 over bytes encode cannot make), every verdict and parsed field its decode_signed's,
every frame body its ChaCha20::apply's, the manifest URI its encode_manifest's.  The announce PoW
digest lives in an anonymous namespace of src/core/Node.cpp (not linkable): as in
tests/golden/gen_pow_golden.py its serialisation (Node.cpp:155-173) is restated and hashed by the
reference's Sha256.  The search itself is pinned by tests/golden/pow.json's announce_pow cases."""
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


def pow_message(cid, pid, ep, uri, sh, ttl, nonce) -> bytes:
    """announce_pow_digest's input (Node.cpp:155-173): BE64-length-prefixed fields, BE64 ttl, BE64 nonce."""
    out = b""
    for f in (cid, pid, ep, uri, sh):
        out += len(f).to_bytes(8, "big") + f
    return out + ttl.to_bytes(8, "big") + nonce.to_bytes(8, "big")


def lzb(d: bytes) -> int:
    n = int.from_bytes(d, "big")
    return 256 - n.bit_length()


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "announce_golden")
        subprocess.run(["g++", "-O2", "-std=c++20", "-I", os.path.join(ref, "include"),
                        os.path.join(ROOT, "tools", "announce_golden.cpp"),
                        os.path.join(ref, "src", "protocol", "Message.cpp"),
                        os.path.join(ref, "src", "protocol", "Manifest.cpp"),
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
            return {"decodes": True, "type": 1, "version": int(r[1]), "ttl": int(r[2]), "chunk_id": r[3],
                    "peer_id": r[4], "endpoint": r[5], "uri": r[6], "shards": r[7], "work_nonce": int(r[8])}

        # the URI of a default 3-of-5 manifest: five shards, no metadata, no hints
        mf = {"chunk_id": splitmix_bytes(71000, 32).hex(), "chunk_hash": splitmix_bytes(71001, 32).hex(),
              "nonce": splitmix_bytes(71002, 12).hex(), "threshold": 3, "total_shares": 5, "expires_at": 1900000000,
              "shard_values": splitmix_bytes(71003, 5 * 32).hex()}
        uri = unhx(run([f"manifest {mf['chunk_id']} {mf['chunk_hash']} {mf['nonce']} 3 5 {mf['expires_at']} "
                        f"{mf['shard_values']}"])[0])
        mf["uri"] = uri.decode()

        # encode_signed as given: versions 0..5, E / U / A including 0, the manifest URI
        shapes = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (14, 37, 3), (21, len(uri), 5), (9, 200, 0), (0, 64, 2)]
        cases = []
        n = 0
        for version in range(6):
            for (E, U, A) in shapes if version == 4 else shapes[4:6]:
                s = 72000 + 10 * n
                n += 1
                key = splitmix_bytes(s, 32)
                cid, pid = splitmix_bytes(s + 1, 32), splitmix_bytes(s + 2, 32)
                ep = splitmix_bytes(s + 3, E)
                u = uri if U == len(uri) else splitmix_bytes(s + 4, U)
                sh = splitmix_bytes(s + 5, A)
                ttl = [3600, 0, 1, 0xFFFFFFFF][n % 4]
                nonce = int.from_bytes(splitmix_bytes(s + 6, 8), "little")
                signed = unhx(run([f"encode {version} {ttl} {hx(cid)} {hx(pid)} {hx(ep)} {hx(u)} {hx(sh)} {nonce} "
                                   f"{hx(key)}"])[0])
                cases.append({"name": f"encode v{version} E{E} U{U} A{A}", "version_in": version, "ttl": ttl,
                              "chunk_id": cid.hex(), "peer_id": pid.hex(), "endpoint": hx(ep), "uri": hx(u),
                              "shards": hx(sh), "work_nonce": nonce, "key": key.hex(), "signed": signed.hex(),
                              "decoded": decode(signed, key)})

        # bytes encode cannot make, signed by the reference's HmacSha256
        def resigned(name, m: bytes, key: bytes):
            signed = unhx(run([f"sign {hx(m)} {hx(key)}"])[0])
            return {"name": name, "key": key.hex(), "signed": signed.hex(), "decoded": decode(signed, key)}

        mutations = []
        by = {c["name"]: c for c in cases}
        v3 = by["encode v3 E14 U37 A3"]
        v4 = by["encode v4 E14 U37 A3"]
        v1 = by["encode v1 E14 U37 A3"]
        m3, k3 = bytes.fromhex(v3["signed"])[:-32], bytes.fromhex(v3["key"])
        m4, k4 = bytes.fromhex(v4["signed"])[:-32], bytes.fromhex(v4["key"])
        m1, k1 = bytes.fromhex(v1["signed"])[:-32], bytes.fromhex(v1["key"])
        assert not v3["decoded"]["decodes"], "a v3 announce made by encode must not decode"
        mutations.append(resigned("v3 with a hand-appended nonce", m3 + (0x0102030405060708).to_bytes(8, "big"), k3))
        mutations.append(resigned("v4 with a trailing byte", m4 + b"\x5a", k4))
        mutations.append(resigned("v4 with eight trailing bytes", m4 + bytes(range(8)), k4))
        mutations.append(resigned("v1 with a trailing byte", m1 + b"\xa5", k1))
        for cut in (0, 1, 2, 81, 82, 89, 90, len(m4) - 9, len(m4) - 8, len(m4) - 1):
            mutations.append(resigned(f"v4 cut to {cut}", m4[:cut], k4))
        for cut in (81, 82, len(m1) - 1):
            mutations.append(resigned(f"v1 cut to {cut}", m1[:cut], k1))
        empty4 = bytes.fromhex(by["encode v4 E0 U0 A0"]["signed"])[:-32]
        ke = bytes.fromhex(by["encode v4 E0 U0 A0"]["key"])
        for cut in (89, 90):
            mutations.append(resigned(f"empty v4 cut to {cut}", empty4[:cut], ke))
        for t in (0x00, 0x02, 0x03, 0x07):
            mutations.append(resigned(f"v4 with type {t:#04x}", m4[:1] + bytes([t]) + m4[2:], k4))
        for v in (0, 5, 255):
            mutations.append(resigned(f"version byte {v}", bytes([v]) + m4[1:], k4))
        mutations.append(resigned("E one too large", m4[:9] + bytes([m4[9] + 1]) + m4[10:], k4))
        mutations.append(resigned("U one too small", m4[:13] + bytes([m4[13] - 1]) + m4[14:], k4))
        short = bytes.fromhex(v4["signed"])[:31]
        mutations.append({"name": "31 bytes in all", "key": k4.hex(), "signed": short.hex(), "decoded": decode(short, k4)})
        bad = bytearray(bytes.fromhex(v4["signed"]))
        bad[-1] ^= 1
        mutations.append({"name": "a flipped MAC bit", "key": k4.hex(), "signed": bytes(bad).hex(),
                          "decoded": decode(bytes(bad), k4)})

        # frames under fixed nonces: body = ChaCha20::apply(key, nonce, signed) (SessionManager.cpp:362-374)
        frames = []
        for i, c in enumerate([cases[0], v3, v4, by[f"encode v4 E21 U{len(uri)} A5"]]):
            nonce = splitmix_bytes(73000 + i, 12)
            body = run([f"chacha {c['key']} {nonce.hex()} {c['signed']}"])[0]
            frames.append({"case": c["name"], "key": c["key"], "nonce": nonce.hex(), "signed": c["signed"], "body": body})

        # PoW digests: the restated serialisation through the reference's Sha256
        pows = []
        for i, c in enumerate([c for c in cases if c["version_in"] == 4]):
            nonce = [0, 1, 2**64 - 1][i] if i < 3 else c["work_nonce"]
            msg = pow_message(bytes.fromhex(c["chunk_id"]), bytes.fromhex(c["peer_id"]), unhx(c["endpoint"]),
                              unhx(c["uri"]), unhx(c["shards"]), c["ttl"], nonce)
            d = run([f"sha {hx(msg)}"])[0]
            pows.append({"case": c["name"], "nonce": nonce, "digest": d, "leading_zero_bits": lzb(bytes.fromhex(d))})

    about = ("announce frame golden vectors; generator tools/gen_announce_golden.py + tools/announce_golden.cpp "
             "(reference Message.cpp / Manifest.cpp / src/crypto compiled where they lie; the Node.cpp PoW "
             "serialisation restated and hashed by the reference Sha256). Inputs: tests/util.py splitmix_bytes.")
    dst = os.path.join(ROOT, "tests", "golden", "announce_frames.json")
    with open(dst, "w") as f:
        json.dump({"_about": about, "manifest": mf, "cases": cases, "mutations": mutations, "frames": frames,
                   "announce_pow": pows}, f, indent=1)
        f.write("\n")
    print(dst, os.path.getsize(dst), "bytes;", len(cases), "cases,", len(mutations), "mutations,", len(frames),
          "frames,", len(pows), "PoW digests; manifest URI", len(uri), "bytes")


if __name__ == "__main__":
    main()
