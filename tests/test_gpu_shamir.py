"""GPU tests of the batched Shamir key shares (shamir.hip, enet_shamir_split_batch /
enet_shamir_combine_batch): byte-equal to the compiled reference's recorded shares and secrets
(tests/golden/shamir.json; reference Shamir::split / combine, src/crypto/Shamir.cpp:114-163) and,
where the reference cannot reach (255 shares, seeded extra records), to tests/gf256_ref.py, which
the golden file pins.  Composition with the chunk kernels is on one stream with no synchronisation
between the calls: combine -> chunk_fetch (Node.cpp:1632-1655) and chunk_store -> split
(:1414-1428).  Bit-exact comparisons throughout."""
import dataclasses
import hashlib
import json
import os
import subprocess
import time

import numpy as np
import pytest

import gf256_ref as G
import oracle
from util import splitmix_array, splitmix_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL = 6  # distinct records per case: the golden one and five seeded extras


@pytest.fixture(scope="module")
def enet():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import ephemeralnet_amd as E
    E.lib()
    return E


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()  # a writable, contiguous copy


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def pools():
    """Per (threshold, share_count): POOL secrets [POOL,32], coefficient rows [POOL,t-1,32] and the
    expected shares [POOL,share_count,32].  Entry 0 is the golden case (the reference's own shares);
    the rest, and the share_count 255 cases, come from gf256_ref.  Computed once, never modified."""
    with open(os.path.join(ROOT, "tests", "golden", "shamir.json")) as f:
        golden = json.load(f)
    out = {}
    shapes = [(s["threshold"], s["share_count"], s) for s in golden["split"]] + [(3, 255, None), (255, 255, None)]
    for t, sc, s in shapes:
        secrets = splitmix_array(91000 + 300 * t + sc, POOL * 32).reshape(POOL, 32)
        coeffs = splitmix_array(92000 + 300 * t + sc, POOL * (t - 1) * 32).reshape(POOL, t - 1, 32)
        secrets[1, :4] = (0x00, 0xFF, 0x80, 0x01)
        if s is not None:
            secrets[0] = np.frombuffer(bytes.fromhex(s["secret"]), np.uint8)
            if t > 1:
                coeffs[0] = np.frombuffer(bytes.fromhex("".join(s["coeffs"])), np.uint8).reshape(t - 1, 32)
        shares = G.split(secrets, coeffs, sc)
        if s is not None:
            shares[0] = np.frombuffer(bytes.fromhex("".join(s["shares"])), np.uint8).reshape(sc, 32)
        for a in (secrets, coeffs, shares):
            a.setflags(write=False)
        out[(t, sc)] = (secrets, coeffs, shares)
    return golden, out


def pick(n, seed):
    """Which pool entry each of n records is: seeded, record 0 the golden one."""
    p = np.frombuffer(splitmix_bytes(seed, n), np.uint8) % POOL
    p = p.astype(np.int64)
    p[0] = 0
    return p


def run_split(enet, secrets, coeffs, t, sc):
    import torch
    n = secrets.shape[0]
    shares = torch.full((n, sc, 32), 0x5A, dtype=torch.uint8, device="cuda")
    enet.shamir_split(dev(secrets), dev(coeffs) if t > 1 else None, t, sc, shares)
    return host(shares)


def run_combine(enet, indices, values):
    import torch
    n, t = indices.shape
    out = torch.full((n, 32), 0x5A, dtype=torch.uint8, device="cuda")
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    enet.shamir_combine(dev(indices), dev(values), t, out, ok)
    return host(out), host(ok)


@pytest.mark.parametrize("n", [1, 7, 65, 1000])
def test_split_matches_reference_shares(enet, pools, n):
    """Every golden (t, n) with the recorded coefficients gives the reference's shares, tiled with
    seeded extra records into batches that end inside a wave (1, 7), cross a wave (65 records = 520
    lanes) and many workgroups (1000); threshold 1 passes coeffs = NULL; share_count 255."""
    _, pool = pools
    for (t, sc), (secrets, coeffs, shares) in pool.items():
        if t >= 254 and n > 65:
            continue  # 8 MB of coefficients per call says nothing the 65-record batch does not
        p = pick(n, 100 * t + sc + n)
        got = run_split(enet, secrets[p], coeffs[p], t, sc)
        assert np.array_equal(got, shares[p]), (t, sc, n, np.argwhere(got != shares[p])[:3].tolist())


def golden_combine_rows(golden, t, sc):
    """(indices, values, secret) of every golden combine case of a split case that the reference
    answered: the first t shares of what the caller supplied."""
    src = next(s for s in golden["split"] if (s["threshold"], s["share_count"]) == (t, sc))
    rows = []
    for c in golden["combine"]:
        if c["split_case"] != [t, sc] or c["throws"]:
            continue
        sh = [(i, bytes.fromhex(src["shares"][v - 1] if isinstance(v, int) else v)) for i, v in c["shares"]][:t]
        rows.append(([i for i, _ in sh], [list(v) for _, v in sh], bytes.fromhex(c["secret"])))
    return rows


def subsets(pool_entry, p, t, sc, seed):
    """A different t-subset of its shares for every record: seeded start and stride through the
    share numbers, in that (unsorted) order."""
    secrets, _, shares = pool_entry
    n = len(p)
    r = np.frombuffer(splitmix_bytes(seed, 2 * n), np.uint8).reshape(n, 2).astype(np.int64)
    idx = np.zeros((n, t), np.uint8)
    val = np.zeros((n, t, 32), np.uint8)
    for i in range(n):
        order = np.roll(np.arange(sc), -int(r[i, 0] % sc))
        if r[i, 1] & 1:
            order = order[::-1]
        chosen = order[:t]
        idx[i] = chosen + 1
        val[i] = shares[p[i], chosen]
    return idx, val, secrets[p]


def test_combine_matches_reference_secrets(enet, pools):
    """Every golden combine -- first-t, reversed, shuffled non-prefix subset, garbage behind the
    threshold -- at the head of a batch of seeded subsets of the pool's shares (1000 records for
    the small thresholds); threshold 255 and share_count 255 through gf256_ref's shares."""
    golden, pool = pools
    for (t, sc), entry in pool.items():
        n = 1000 if t <= 5 else (65 if t <= 32 else 2)
        p = pick(n, 7 * t + sc)
        idx, val, want = subsets(entry, p, t, sc, 500 + t + sc)
        want = want.copy()
        if (t, sc) in [(s["threshold"], s["share_count"]) for s in golden["split"]]:
            rows = golden_combine_rows(golden, t, sc)
            assert rows
            for k, (gi, gv, gs) in enumerate(rows[:n]):
                idx[k], val[k], want[k] = gi, gv, np.frombuffer(gs, np.uint8)
        got, ok = run_combine(enet, idx, val)
        assert ok.tolist() == [1] * n, (t, sc)
        assert np.array_equal(got, want), (t, sc, np.argwhere(got != want)[:3].tolist())


def test_combine_index_zero_and_duplicates(enet, pools):
    """Index 0 is legal (the share at x = 0 is the secret).  Two equal indices among the first t --
    at positions (0, 1) and (t-2, t-1) -- give ok = 0 and 32 zero bytes; the records beside them in
    the same wave do not notice."""
    _, pool = pools
    for (t, sc) in [(2, 3), (3, 5), (5, 8)]:
        entry = pool[(t, sc)]
        n = 130
        p = pick(n, 900 + t)
        idx, val, want = subsets(entry, p, t, sc, 950 + t)
        want = want.copy()
        for r in (4, 77):                    # the secret itself stands in for one share, at x = 0
            idx[r, t - 1] = 0
            val[r, t - 1] = want[r]
        idx[3, 1] = idx[3, 0]
        idx[70, t - 1] = idx[70, t - 2]
        want[3] = 0
        want[70] = 0
        got, ok = run_combine(enet, idx, val)
        assert [i for i in range(n) if ok[i] != 1] == [3, 70], (t, sc)
        assert np.array_equal(got, want), (t, sc, np.argwhere(got != want)[:3].tolist())


@pytest.mark.parametrize("t,sc", [(3, 5), (5, 8)])
def test_split_then_combine_on_device(enet, t, sc):
    """1000 seeded records: split, then a different subset of every record's shares gathered on
    the device and combined, all on the current stream; the secrets come back."""
    import torch
    n = 1000
    secrets = dev(splitmix_array(31000 + t, n * 32).reshape(n, 32))
    coeffs = dev(splitmix_array(32000 + t, n * (t - 1) * 32).reshape(n, t - 1, 32))
    shares = torch.zeros((n, sc, 32), dtype=torch.uint8, device="cuda")
    enet.shamir_split(secrets, coeffs, t, sc, shares)
    r = np.frombuffer(splitmix_bytes(33000 + t, n), np.uint8).astype(np.int64)
    chosen = np.stack([(np.roll(np.arange(sc), -int(r[i] % sc))[::(-1 if r[i] & 16 else 1)])[:t] for i in range(n)])
    ci = dev(chosen)
    values = torch.gather(shares, 1, ci[:, :, None].expand(n, t, 32)).contiguous()
    indices = (ci + 1).to(torch.uint8).contiguous()
    out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    enet.shamir_combine(indices, values, t, out, ok)
    assert int(ok.sum()) == n and torch.equal(out, secrets)


def test_split_and_combine_past_the_block_cap(enet):
    """n = 2^21 + 300 records of 2-of-2: 8 n words on workgroups of 256 threads would be 65 546
    workgroups, over kShamirMaxBlocks = 65 536 (shamir.hip), so the records from 2 097 152 on are
    reached only by the kernels' grid-stride step.  Every share against gf256_ref.split; combine
    from the shares in the order (2, 1) gives every secret back -- gf256_ref.combine agrees on the
    records at both ends -- except record n - 7, whose two indices are equal: ok = 0, 32 zero bytes."""
    t0 = time.time()
    n, t, sc = (1 << 21) + 300, 2, 2
    assert -(-8 * n // 256) == 65546 > 65536 and 65536 * 256 // 8 == 2097152 < n - 7
    secrets = splitmix_array(61000, n * 32).reshape(n, 32)
    coeffs = splitmix_array(62000, n * 32).reshape(n, 1, 32)
    want = G.split(secrets, coeffs, sc)
    got = run_split(enet, secrets, coeffs, t, sc)
    assert np.array_equal(got, want), np.argwhere(got != want)[:3].tolist()
    idx = np.tile(np.array([2, 1], np.uint8), (n, 1))
    val = np.ascontiguousarray(want[:, ::-1, :])
    dup = n - 7
    idx[dup] = (2, 2)
    ends = np.r_[0:4, n - 12:n]
    ref_secret, ref_ok = G.combine(idx[ends], val[ends])
    out, ok = run_combine(enet, idx, val)
    assert np.array_equal(out[ends], ref_secret) and np.array_equal(ok[ends], ref_ok)
    assert np.flatnonzero(ok != 1).tolist() == [dup] and ok[dup] == 0
    expect = secrets.copy()
    expect[dup] = 0
    assert np.array_equal(out, expect), np.argwhere(out != expect)[:3].tolist()
    print(f"\n[shamir] {n} records past the block cap: {time.time() - t0:.1f} s")


def chunk_case(n, L, seed):
    items = [splitmix_bytes(seed + i, L) for i in range(n)]
    keys = splitmix_array(seed + 10000, n * 32).reshape(n, 32)
    nonces = [splitmix_bytes(seed + 20000 + i, 12) for i in range(n)]
    ids = [splitmix_bytes(seed + 30000 + i, 32) for i in range(n)]
    cts = [oracle.chacha20_xor(keys[i].tobytes(), nonces[i], items[i], int.from_bytes(ids[i][:4], "little"))
           for i in range(n)]
    return items, keys, nonces, ids, cts


@pytest.mark.parametrize("n,L", [(300, 256), (64, 4096)])
def test_combine_feeds_chunk_fetch_on_one_stream(enet, n, L):
    """shamir_combine writes a key buffer, chunk_fetch reads it as `keys` on the same stream with
    no synchronisation between the two calls: every chunk is the oracle's plaintext with ok = 1,
    and the one record with a corrupted share fails its hash check and is zeroed."""
    import torch
    t, sc = 3, 5
    items, keys, nonces, ids, cts = chunk_case(n, L, 41000 + L)
    coeffs = splitmix_array(42000 + L, n * (t - 1) * 32).reshape(n, t - 1, 32)
    shares = G.split(keys, coeffs, sc)
    idx = np.tile(np.array([5, 2, 3], np.uint8), (n, 1))
    val = shares[:, [4, 1, 2], :].copy()
    bad = n // 2
    val[bad, 1, 9] ^= 0x40
    hashes = b"".join(hashlib.sha256(x).digest() for x in items)
    b = enet.make_batch(cts, [bytes(32)] * n, nonces)
    d_idx, d_val, d_ids = dev(idx), dev(val), dev(np.frombuffer(b"".join(ids), np.uint8))
    d_hash = dev(np.frombuffer(hashes, np.uint8))
    keybuf = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    ok_c = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ok_f = torch.zeros(n, dtype=torch.uint8, device="cuda")
    back = torch.full_like(b.arena, 0xAA)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        enet.shamir_combine(d_idx, d_val, t, keybuf, ok_c, stream=s)
        enet.chunk_fetch(dataclasses.replace(b, keys=keybuf), back, d_ids, d_hash, ok_f, stream=s)
    s.synchronize()
    got = host(back).tobytes()
    assert host(ok_c).tolist() == [1] * n            # a corrupted value still combines: to a wrong key
    assert host(ok_f).tolist() == [0 if i == bad else 1 for i in range(n)]
    for i in range(n):
        assert got[i * L:(i + 1) * L] == (bytes(L) if i == bad else items[i]), i
    kb = host(keybuf).reshape(n, 32)
    assert np.array_equal(np.delete(kb, bad, 0), np.delete(keys, bad, 0)) and not np.array_equal(kb[bad], keys[bad])


def test_chunk_store_then_split_on_one_stream(enet):
    """chunk_store under a key buffer, then shamir_split of that buffer on the same stream: the
    ciphertexts are the oracle's under those keys and the shares recombine (gf256_ref) to them."""
    import torch
    n, L, t, sc = 300, 256, 3, 5
    items, keys, nonces, ids, cts = chunk_case(n, L, 51000)
    coeffs = splitmix_array(52000, n * (t - 1) * 32).reshape(n, t - 1, 32)
    b = enet.make_batch(items, [k.tobytes() for k in keys], nonces)
    d_ids, d_co = dev(np.frombuffer(b"".join(ids), np.uint8)), dev(coeffs)
    out = torch.full_like(b.arena, 0x55)
    hashes = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    shares = torch.zeros((n, sc, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        enet.chunk_store(b, out, hashes, chunk_ids=d_ids, stream=s)
        enet.shamir_split(b.keys, d_co, t, sc, shares, stream=s)
    s.synchronize()
    assert host(out).tobytes() == b"".join(cts)
    assert host(hashes).tobytes() == b"".join(hashlib.sha256(x).digest() for x in items)
    sh = host(shares)
    assert np.array_equal(sh, G.split(keys, coeffs, sc))
    sec, ok = G.combine(np.tile(np.array([4, 1, 5], np.uint8), (n, 1)), sh[:, [3, 0, 4], :])
    assert ok.all() and np.array_equal(sec, keys)


def test_cpp_batch_store_shared_fetch_shared(enet, tmp_path):
    """crypto::batch::shamir_split / shamir_combine and chunk_store_shared -> chunk_fetch_shared
    through tests/cpp/shamir_batch.cpp (checked there with the scalar reference-signature API),
    linked against the library the package loaded."""
    lib = enet.LIB_PATH
    out = str(tmp_path / "shamir_batch")
    subprocess.run(["g++", "-std=c++20", "-O1", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "shamir_batch.cpp"), "-o", out,
                    "-L", os.path.dirname(lib), "-lenet_crypto", "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    res = subprocess.run([out], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "shamir batch ok" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
