"""The C++ drop-in API (include/ephemeralnet/crypto/*.hpp, reference signatures) compiled the way a
reference caller would be, linked against libenet_crypto.so.  CPU: it compiles and links.
GPU: every reference entry point reproduces the golden vectors of the compiled reference."""
import hashlib
import os
import subprocess

import pytest

import oracle

from util import splitmix_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "api_test.cpp")


@pytest.fixture(scope="module")
def api_bin(tmp_path_factory):
    from ephemeralnet_amd import build as B
    lib = B.build(verbose=False)
    out = str(tmp_path_factory.mktemp("cpp") / "api_test")
    subprocess.run(["g++", "-std=c++20", "-O1", "-I", os.path.join(ROOT, "include"), SRC, "-o", out,
                    "-L", os.path.dirname(lib), "-lenet_crypto", "-Wl,-rpath," + os.path.dirname(lib)],
                   check=True)
    return out


def h(b: bytes) -> str:
    return b.hex() if b else "-"


def test_cpp_api_compiles_and_links(api_bin):
    assert os.access(api_bin, os.X_OK)


def scalar_ops(golden, big=False):
    """Reference-signature calls (ChaCha20::apply, Sha256, HmacSha256, CryptoManager) with the
    golden answers of the compiled reference.  big: also the records over 4 KiB (64 KiB)."""
    ops, expect = [], []
    for c in golden["chacha20"]:
        if c["len"] > 4097 and not big:
            continue
        pt = splitmix_bytes(c["pt_seed"], c["len"])
        ops.append(f"chacha {c['key']} {c['nonce']} {c['counter']} {h(pt)}")
        expect.append(("hex", c["ct"]))
        if c["len"] <= 4097:
            ops.append(f"chacha_inplace {c['key']} {c['nonce']} {c['counter']} {h(pt)}")
            expect.append(("hex", c["ct"]))
    for c in golden["sha256"]:
        data = b"abc" if c["abc"] else splitmix_bytes(c["seed"], c["len"])
        ops.append(f"sha {h(data)}")
        expect.append(("eq", c["digest"]))
        if c["digest_pieces_7"]:
            ops.append(f"sha_pieces 7 {h(data)}")
            expect.append(("eq", c["digest_pieces_7"]))
            ops.append(f"sha_pieces 64 {h(data)}")
            expect.append(("eq", c["digest"]))
    for c in golden["hmac"]:
        ops.append(f"hmac {c['key'] or '-'} {h(splitmix_bytes(c['seed'], c['len']))}")
        expect.append(("eq", c["mac"]))
    for c in golden["hmac_verify"]:
        ops.append(f"hverify {c['key']} {h(splitmix_bytes(c['seed'], c['len']))} {c['mac']}")
        expect.append(("eq", "1" if c["ok"] else "0"))
    for c in golden["cryptomanager"]:
        if c["len"] > 4097 and not big:
            continue
        pt = splitmix_bytes(c["pt_seed"], c["len"])
        ct = oracle.chacha20_xor(bytes.fromhex(c["key"]), bytes.fromhex(c["nonce"]), pt,
                                 oracle.derive_counter(bytes.fromhex(c["chunk_id"])))
        assert ("hex" not in c["ct"]) or ct.hex() == c["ct"]["hex"]
        ops.append(f"cm_dec {c['key']} {c['chunk_id']} {c['nonce']} {h(ct)}")
        expect.append(("eq", h(pt)))
        ops.append(f"cm_roundtrip {c['chunk_id']} {h(pt)}")
        expect.append(("eq", "1"))
    for L in (0, 1, 4096):
        d = splitmix_bytes(40000 + L, L)
        ops.append(f"chunk_id {h(d)}")
        expect.append(("eq", hashlib.sha256(d).hexdigest()))
    return ops, expect


def run_ops(api_bin, ops):
    res = subprocess.run([api_bin], input="\n".join(ops) + "\n", capture_output=True, text=True,
                         check=True, timeout=300)
    return res.stdout.splitlines(), res.stderr


def check(ops, expect, res):
    assert len(res) == len(ops)
    for op, (kind, e), got in zip(ops, expect, res):
        if kind == "hex":
            if "hex" in e:
                assert got == (e["hex"] or "-"), op[:60]
            else:
                assert hashlib.sha256(bytes.fromhex(got)).hexdigest() == e["sha256"]
        elif kind == "wire":  # random nonce: check the frame against the oracle with its nonce
            key, m = e
            fr, flag = got.split()
            fr = bytes.fromhex(fr)
            nonce, body = fr[:12], fr[16:]
            assert flag == "1" and int.from_bytes(fr[12:16], "big") == len(body) == len(m) + 32
            assert body == oracle.frame_seal(key, nonce, m)
        else:
            assert got == e, op[:60]


def stats(line):
    host, dev, fail, launches, records = map(int, line.split())
    return {"host": host, "device": dev, "failures": fail, "launches": launches, "records": records}


@pytest.mark.parametrize("policy", ["host", "auto"])
def test_cpp_scalar_api_host_engine_golden(api_bin, golden, policy):
    """CPU, no GPU: the reference signatures served by the host engine (SHA-NI / AVX2 or portable)
    reproduce the compiled reference's golden vectors, including streaming Sha256 in 7- and
    64-byte pieces and in-place ChaCha20::apply; every call is counted on the host."""
    ops, expect = scalar_ops(golden, big=True)
    res, _ = run_ops(api_bin, [f"policy {policy}", "reset_stats"] + ops + ["stats"])
    assert res[:2] == ["0", "ok"]
    check(ops, expect, res[2:-1])
    st = stats(res[-1])
    assert st["host"] > 0 and st["device"] == 0 and st["failures"] == 0


def test_cpp_scalar_api_device_failure_finishes_on_host(api_bin, golden):
    """Injected failure on the CPU build: ENET_SCALAR_DEVICE with no usable
    device -- every device call fails, is counted, reported once on stderr, and finished on the
    host engine bit-exactly; nothing throws into the caller (the process exits 0)."""
    ops, expect = scalar_ops(golden)
    res, err = run_ops(api_bin, ["policy device", "reset_stats"] + ops + ["stats"])
    check(ops, expect, res[2:-1])
    st = stats(res[-1])
    assert st["failures"] > 0 and st["device"] == 0 and st["host"] >= st["failures"]
    assert err.count("finished on the host engine") == 1


@pytest.mark.gpu
@pytest.mark.parametrize("n,maxlen,seed", [(1, 100, 1), (37, 3000, 2), (300, 1600, 3), (12, 70000, 4)])
def test_cpp_packed_batch_overloads_vs_oracle(api_bin, n, maxlen, seed):
    """The contiguous-output forms of crypto::batch::aead_seal / aead_open / wire_seal / wire_open /
    chacha20_apply (host std::vector records in, ONE packed output span) through the host-memory
    batch runtime: bit-exact with the oracle record by record, a tampered tag / frame rejected and
    zeroed, and equal to the vector-per-record forms of the same calls -- fresh vectors and the
    reuse overloads into caller-owned vectors (resized exactly, capacity kept)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    lens = [int(x) for x in rng.integers(0, maxlen + 1, n)]
    lens[: min(n, 4)] = [0, 1, 64, maxlen][: min(n, 4)]
    keys = [splitmix_bytes(1000 * seed + i, 32) for i in range(n)]
    nonces = [splitmix_bytes(2000 * seed + i, 12) for i in range(n)]
    msgs = [splitmix_bytes(3000 * seed + i, L) for i, L in enumerate(lens)]
    line = f"packed {n} " + " ".join(f"{k.hex()} {v.hex()} {h(m)}" for k, v, m in zip(keys, nonces, msgs))
    res, err = run_ops(api_bin, [line])
    ct, tags, aok, pt, frames, wok, back, same = res[0].split()
    unhex = lambda x: b"" if x == "-" else bytes.fromhex(x)
    ct, tags, pt, frames, back = map(unhex, (ct, tags, pt, frames, back))
    assert same == "1"
    o = 0
    fo = 0
    want_ct, want_fr = b"", b""
    for i in range(n):
        c, t = oracle.aead_seal(keys[i], nonces[i], msgs[i])
        assert ct[o:o + lens[i]] == c and tags[16 * i:16 * i + 16] == t, i
        body = oracle.frame_seal(keys[i], nonces[i], msgs[i])
        wire = nonces[i] + (len(body)).to_bytes(4, "big") + body
        assert frames[fo:fo + len(wire)] == wire, i
        bad_a, bad_w = i == 1, i == 2
        assert aok[i] == ("0" if bad_a else "1") and wok[i] == ("0" if bad_w else "1"), i
        assert pt[o:o + lens[i]] == (bytes(lens[i]) if bad_a else msgs[i]), i
        assert back[o:o + lens[i]] == (bytes(lens[i]) if bad_w else msgs[i]), i
        o += lens[i]
        fo += len(wire)
    assert len(ct) == o and len(frames) == fo


def test_cpp_frame_nonces_differ_after_fork(api_bin):
    """the per-thread frame-nonce generator is copied by fork(); a pthread_atfork
    handler makes the child re-key, so parent and child never hand out the same nonce (the
    reference drew every nonce from std::random_device, SessionManager.cpp:365-371)."""
    for _ in range(3):
        res, _ = run_ops(api_bin, ["policy host", "fork_nonces"])
        parent, child, flag = res[1].split()
        assert flag == "1" and parent != child and len(parent) == len(child) == 24


SIZE_CHECKED = [  # entry points with per-record arrays, by overload
    "chacha20_apply/ret", "chacha20_apply/ret-counters", "chacha20_apply/vec", "chacha20_apply/span",
    "aead_seal/ret", "aead_seal/vec", "aead_seal/span", "aead_open/ret", "aead_open/vec", "aead_open/span",
    "frame_seal", "frame_open", "chunk_store", "chunk_fetch", "chunk_store_shared", "chunk_fetch_shared",
    "wire_seal/ret", "wire_seal/vec", "wire_seal/span", "wire_open/ret", "wire_open/vec", "wire_open/span",
    "wire_seal_sessions", "wire_open_sessions", "chunk_frames_seal", "chunk_frames_seal/versions",
    "chunk_frames_open", "pow_search", "pow_check", "session_keys", "key_exchange", "store_pow_valid"]
EMPTY_CHECKED = [e for e in SIZE_CHECKED if e not in ("chacha20_apply/ret-counters", "chunk_frames_seal/versions")] + [
    "sha256", "shamir_split", "shamir_combine", "handshake_accept", "compute_store_pow"]


def test_cpp_batch_argument_handling(api_bin):
    """CPU, no device call: every crypto::batch / security::batch entry point throws
    std::invalid_argument with its exact message for mismatched per-record array sizes and for a
    contiguous output one byte short (records of 1 and 65 bytes), and returns empty -- `ok` and
    reused output vectors emptied -- for an empty batch; the entry points without per-record
    arrays return their host-computed values."""
    res, _ = run_ops(api_bin, ["batch_args"])
    got = {}
    for line in res:
        label, _, value = line.partition(" | ")
        assert label not in got
        got[label] = value
    want = {}
    for e in SIZE_CHECKED:
        name = e.split("/")[0]
        want[f"mismatch {e}"] = (f"enet {name}: size mismatch" if name == "store_pow_valid"
                                 else f"enet batch::{name}: size mismatch")
    for name in ("chacha20_apply", "aead_seal", "aead_open", "wire_seal", "wire_open"):
        want[f"short {name}"] = f"enet batch::{name}: output span too small"
    for e in EMPTY_CHECKED:
        want[f"empty {e}"] = "empty"
    be64 = lambda x: x.to_bytes(8, "big")
    lp = lambda b: be64(len(b)) + b
    a, b, cid = b"\xaa" + bytes(31), bytes(31) + b"\xbb", b"\x00\xcc" + bytes(30)
    want["value packed_offsets"] = "0 49 162 0 0 17"
    want["value handshake_pow_prefix"] = (lp(a) + lp(b) + be64(0x01020304)).hex()
    want["value announce_pow_prefix"] = (lp(cid) + lp(a) + lp(b"ep:1") + lp(b"uri") + lp(b"\x01\x02\x03")
                                         + be64(258)).hex()
    want["value compute_handshake_pow"] = "1 0"
    want["value compute_announce_pow"] = "1 0"
    want["value compute_store_pow/0"] = "2 1"
    want["value store_pow_valid/0"] = "0101"
    assert got == want


@pytest.mark.gpu
def test_cpp_batch_sha256_blob_and_device_slot_paths(api_bin):
    """crypto::batch::sha256 in one process: six messages around the padding boundaries (arena
    under 8 KiB: the pinned zero-copy staging blob), then the same plus one of 8193 bytes (device
    staging slots) -- bit-exact with the host engine and hashlib."""
    msgs = [splitmix_bytes(9100 + L, L) for L in (0, 55, 56, 64, 119, 1000)]
    long = msgs + [splitmix_bytes(9999, 8193)]
    res, _ = run_ops(api_bin, ["sha_batch " + " ".join(h(m) for m in msgs),
                               "sha_batch " + " ".join(h(m) for m in long)])
    for line, ms in zip(res, (msgs, long)):
        assert line.split() == [hashlib.sha256(m).hexdigest() for m in ms] + ["1"]


@pytest.mark.gpu
def test_cpp_batch_session_keys_vs_host_hmac(api_bin):
    """crypto::batch::session_keys for 3 secrets, counters {0, 1, 2^40}: bit-exact with the host
    engine's HMAC-SHA256(secret, BE64(counter) || BE64(ticks)) and Python's hmac."""
    import hmac
    sec, t0 = splitmix_bytes(4242, 32), 1234567890123
    res, _ = run_ops(api_bin, [f"session_keys {sec.hex()} {t0}"])
    want = []
    for i, (c, t) in enumerate(zip((0, 1, 1 << 40), (t0, t0 + 1, -t0))):
        key = bytes([sec[0] ^ i]) + sec[1:]
        msg = c.to_bytes(8, "big") + (t % (1 << 64)).to_bytes(8, "big")
        want.append(hmac.new(key, msg, hashlib.sha256).hexdigest())
    assert res[0].split() == want + ["1"]


@pytest.mark.gpu
def test_cpp_api_matches_reference_golden(api_bin, golden):
    ops, expect = scalar_ops(golden, big=True)
    for f in golden["frames"]:
        m = bytes.fromhex(f["signed"])[:-32]
        ops.append(f"frame_seal {f['key']} {f['nonce']} {h(m)}")
        expect.append(("eq", f"{f['body']} 1"))
    for f in golden["frames"]:
        m = bytes.fromhex(f["signed"])[:-32]
        ops.append(f"wire_queue {f['key']} {h(m)}")
        expect.append(("wire", (bytes.fromhex(f["key"]), m)))
    # session-keyed frames: frame 0 is filed under table[1]
    for f in golden["frames"][:3]:
        m = bytes.fromhex(f["signed"])[:-32]
        k0 = hashlib.sha256(bytes.fromhex(f["key"])).hexdigest()
        ops.append(f"wire_sessions {k0} {f['key']} {h(m)}")
        expect.append(("wire", (bytes.fromhex(f["key"]), m)))
    for L in (0, 1, 64, 1500, 4096):
        pt = splitmix_bytes(777 + L, L)
        ops.append(f"chunk_pipe {h(pt)}")
        expect.append(("eq", f"{hashlib.sha256(pt).hexdigest()} 1"))
    for c in golden["aead"]:
        if c["aad_len"] or c["len"] > 1500:
            continue
        pt = splitmix_bytes(c["pt_seed"], c["len"])
        ops.append(f"aead_seal {c['key']} {c['nonce']} {h(pt)}")
        expect.append(("eq", f"{c['ct']['hex'] or '-'} {c['tag']}"))
    # every policy: the device (each call one GPU round trip), auto with a 1-byte crossover (every
    # ChaCha20 record through the coalescer), the default auto and the host engine
    for pol in ("policy device", "policy auto 1", "policy auto 0", "policy host"):
        res, err = run_ops(api_bin, [pol, "reset_stats"] + ops + ["stats"])
        assert res[:2] == ["0", "ok"], pol
        check(ops, expect, res[2:-1])
        st = stats(res[-1])
        assert st["failures"] == 0, (pol, err)
        if pol == "policy device":
            assert st["device"] > 0
        if pol == "policy auto 1":
            assert st["launches"] > 0 and st["records"] >= st["launches"]


@pytest.mark.gpu
def test_cpp_scalar_device_failure_injected_on_gpu(api_bin, golden):
    """On the GPU box: the next 5 device calls fail (enet_scalar_inject_device_failures); those
    calls are finished on the host engine with the same bytes, later calls use the device."""
    ops, expect = scalar_ops(golden)
    res, err = run_ops(api_bin, ["policy device", "reset_stats", "inject 5"] + ops + ["stats"])
    check(ops, expect, res[3:-1])
    st = stats(res[-1])
    assert st["failures"] == 5 and st["device"] > 0
    assert err.count("finished on the host engine") == 1


def pow_ops(batch=True):
    """security::StoreProof, network::KeyManager (and with batch=True the crypto::batch PoW
    searches of Node.cpp announce / handshake) against tests/golden/pow.json."""
    import json
    with open(os.path.join(ROOT, "tests", "golden", "pow.json")) as f:
        pg = json.load(f)
    ops, expect = [], []
    for c in pg["store_pow"]:
        if c["max_attempts"] == 0:
            continue
        ops.append(f"store_pow {c['chunk_id']} {c['payload_size']} {c['hint'] or '-'} {c['difficulty']} "
                   f"{c['max_attempts']}")
        expect.append(f"{c['nonce']} {int(c['valid'])} {int(c['valid_next'])}" if c["found"] else "none")
    if batch:
        for c in pg["handshake_pow"]:
            ops.append(f"handshake_pow {c['initiator']} {c['responder']} {c['public']} {c['difficulty']}")
            dn = c["nonce"] if c["found"] else 2**64 - 1  # Node.cpp drop-in: nonce_out untouched if not found
            expect.append(f"{int(c['found'])} {c['nonce']} {c['attempt']} 1 {int(c['found'])} {dn}")
        for c in pg["announce_pow"]:
            ops.append("announce_pow " + " ".join(c[k] or "-" for k in ("chunk_id", "peer_id", "endpoint",
                                                                       "manifest_uri", "assigned_shards"))
                       + f" {c['ttl']} {c['difficulty']}")
            dn = c["nonce"] if c["found"] else 2**64 - 1
            expect.append(f"{int(c['found'])} {c['nonce']} {c['attempt']} {int(c['found'])} {dn}")
    for c in pg["session_keys"]:
        ops.append(f"keymgr {c['secret']} {c['material']} {c['rotate_ticks']}")
        expect.append(f"{c['material_key']} {c['rotated_key']} 1")
    for c in pg["sanitize_filename_hint"]:
        ops.append(f"sanitize {c['raw'] or '-'}")
        expect.append(c["result"] if c["result"] is not None else "none")
    for L in (0, 1, 4096):
        d = splitmix_bytes(40000 + L, L)
        ops.append(f"chunk_id {h(d)}")
        expect.append(hashlib.sha256(d).hexdigest())
    return ops, expect


def test_cpp_storeproof_and_keys_host_engine_golden(api_bin):
    """CPU: compute_store_pow / store_pow_valid (StoreProof.cpp), KeyManager (KeyManager.cpp) and
    derive_chunk_id through the reference signatures on the host engine -- the reference's own
    golden answers (tests/golden/pow.json)."""
    ops, expect = pow_ops(batch=False)
    res, _ = run_ops(api_bin, ["policy host"] + ops)
    assert res[0] == "0"
    assert len(res) == len(ops) + 1
    for op, e, got in zip(ops, expect, res[1:]):
        assert got == e, op[:80]


@pytest.mark.gpu
def test_cpp_pow_and_keys_match_reference_golden(api_bin):
    """security::StoreProof, crypto::batch PoW (Node.cpp announce / handshake) and
    network::KeyManager through the reference C++ signatures against tests/golden/pow.json, on
    the device (policy device and the default auto)."""
    ops, expect = pow_ops()
    for pol in ("policy device", "policy auto"):
        res, err = run_ops(api_bin, [pol, "reset_stats"] + ops + ["stats"])
        assert len(res) == len(ops) + 3
        for op, e, got in zip(ops, expect, res[2:-1]):
            assert got == e, (pol, op[:80])
        st = stats(res[-1])
        assert st["failures"] == 0 and st["device"] > 0, (pol, err)
