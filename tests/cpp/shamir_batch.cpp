// shamir_batch.cpp -- crypto::batch's Shamir calls on the device (tests/test_gpu_shamir.py):
// shamir_split -> shamir_combine against the scalar drop-in, and the node's two steps
// chunk_store_shared -> chunk_fetch_shared (Node.cpp:1414-1428, 1632-1655) checked with the scalar
// reference-signature API (Shamir::combine, ChaCha20::apply, Sha256::digest).  Prints what failed
// and exits non-zero; "shamir batch ok" otherwise.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <span>
#include <stdexcept>
#include <vector>

#include "enet_crypto.h"
#include "ephemeralnet/crypto/Batch.hpp"
#include "ephemeralnet/crypto/ChaCha20.hpp"
#include "ephemeralnet/crypto/Sha256.hpp"
#include "ephemeralnet/crypto/Shamir.hpp"

using namespace ephemeralnet;
using namespace ephemeralnet::crypto;

static int g_bad = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (g_bad++ < 20) {           \
                std::printf(__VA_ARGS__); \
                std::printf("\n");        \
            }                             \
        }                                 \
    } while (0)

static std::uint64_t g_seed = 99;
static std::uint64_t splitmix() {
    std::uint64_t z = (g_seed += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static void fill(std::uint8_t* p, std::size_t n) {
    for (std::size_t i = 0; i < n; ++i) p[i] = (std::uint8_t)splitmix();
}

// t shares of a record starting at share (i mod n), wrapping: a different subset per record
static std::vector<ShamirShare> subset(const std::vector<ShamirShare>& all, std::size_t i, unsigned t) {
    std::vector<ShamirShare> s;
    for (unsigned k = 0; k < t; ++k) s.push_back(all[(i + k) % all.size()]);
    return s;
}

static void split_combine(unsigned t, unsigned n, std::size_t records) {
    std::vector<std::array<std::uint8_t, 32>> secrets(records);
    for (auto& s : secrets) fill(s.data(), 32);
    const auto shares = batch::shamir_split(secrets, (std::uint8_t)t, (std::uint8_t)n);
    CHECK(shares.size() == records, "split %u/%u: %zu records back", t, n, shares.size());
    std::vector<std::vector<ShamirShare>> picked(records);
    for (std::size_t i = 0; i < records; ++i) {
        CHECK(shares[i].size() == n, "split %u/%u: record %zu has %zu shares", t, n, i, shares[i].size());
        for (unsigned j = 0; j < n; ++j) CHECK(shares[i][j].index == j + 1, "split: index of share %u", j);
        picked[i] = subset(shares[i], i, t);
        if (i % 97 == 0)  // the scalar drop-in reads the device's shares
            CHECK(Shamir::combine(picked[i], (std::uint8_t)t) == secrets[i], "scalar combine of device shares, record %zu", i);
    }
    if (t > 1 && records > 1) CHECK(shares[0][0].value != secrets[0], "share 1 of a threshold > 1 split is the secret");
    std::vector<std::uint8_t> ok;
    const auto back = batch::shamir_combine(picked, (std::uint8_t)t, ok);
    for (std::size_t i = 0; i < records; ++i)
        CHECK(ok[i] == 1 && back[i] == secrets[i], "combine %u/%u: record %zu (ok %u)", t, n, i, (unsigned)ok[i]);
}

static void store_fetch(unsigned t, unsigned n) {
    std::vector<std::size_t> lens;
    for (int i = 0; i < 300; ++i) lens.push_back(256);
    for (int i = 0; i < 64; ++i) lens.push_back(4096);
    for (std::size_t l : {0, 1, 63, 65, 1500}) lens.push_back(l);
    const std::size_t m = lens.size();
    std::vector<std::vector<std::uint8_t>> chunks(m);
    std::vector<std::span<const std::uint8_t>> views(m);
    std::vector<Nonce> nonces(m);
    std::vector<ChunkId> ids(m);
    for (std::size_t i = 0; i < m; ++i) {
        chunks[i].resize(lens[i]);
        fill(chunks[i].data(), lens[i]);
        views[i] = chunks[i];
        fill(nonces[i].bytes.data(), 12);
        fill(ids[i].data(), 32);
    }
    const auto stored = batch::chunk_store_shared(nonces, views, ids, (std::uint8_t)t, (std::uint8_t)n);
    CHECK(stored.size() == m, "store_shared: %zu records back", stored.size());
    std::vector<std::vector<ShamirShare>> picked(m);
    std::vector<std::span<const std::uint8_t>> cts(m);
    std::vector<std::array<std::uint8_t, 32>> hashes(m);
    for (std::size_t i = 0; i < m; ++i) {
        CHECK(stored[i].shares.size() == n, "store_shared: record %zu has %zu shares", i, stored[i].shares.size());
        picked[i] = subset(stored[i].shares, i, t);
        cts[i] = stored[i].chunk.data;
        hashes[i] = stored[i].chunk.chunk_hash;
        CHECK(hashes[i] == Sha256::digest(chunks[i]), "store_shared: chunk_hash of record %zu", i);
        // the shares are the key: the scalar API recombines it and opens the ciphertext
        Key key{};
        key.bytes = Shamir::combine(picked[i], (std::uint8_t)t);
        std::vector<std::uint8_t> pt;
        ChaCha20::apply(key, nonces[i], stored[i].chunk.data, pt, enet_chunk_counter(ids[i].data()));
        CHECK(pt == chunks[i], "store_shared: record %zu does not open under its recombined key", i);
        if (i > 0 && lens[i] >= 32) CHECK(stored[i].shares[0].value != stored[i - 1].shares[0].value, "store_shared: keys repeat");
    }
    std::vector<std::uint8_t> ok;
    auto back = batch::chunk_fetch_shared(picked, (std::uint8_t)t, nonces, ids, cts, hashes, ok);
    for (std::size_t i = 0; i < m; ++i)
        CHECK(ok[i] == 1 && back[i] == chunks[i], "fetch_shared: record %zu (ok %u)", i, (unsigned)ok[i]);
    // a corrupted share (wrong key -> hash mismatch) and a duplicate index (no key at all) fail
    // closed; their neighbours do not notice
    picked[5][0].value[7] ^= 0x10;
    if (t > 1) picked[301][t - 1].index = picked[301][0].index;
    back = batch::chunk_fetch_shared(picked, (std::uint8_t)t, nonces, ids, cts, hashes, ok);
    for (std::size_t i = 0; i < m; ++i) {
        const bool broken = i == 5 || (t > 1 && i == 301);
        if (broken)
            CHECK(ok[i] == 0 && back[i] == std::vector<std::uint8_t>(lens[i], 0), "fetch_shared: broken record %zu got through", i);
        else
            CHECK(ok[i] == 1 && back[i] == chunks[i], "fetch_shared: record %zu beside a broken one (ok %u)", i, (unsigned)ok[i]);
    }
}

template <class F>
static bool throws_invalid(F&& f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}

int main() {
    split_combine(3, 5, 1000);
    split_combine(5, 8, 1000);
    split_combine(1, 1, 3);
    split_combine(255, 255, 2);
    store_fetch(3, 5);
    store_fetch(1, 2);
    std::vector<std::array<std::uint8_t, 32>> one(1);
    std::vector<std::vector<ShamirShare>> few(1, std::vector<ShamirShare>(2));
    std::vector<std::uint8_t> ok;
    CHECK(throws_invalid([&] { batch::shamir_split(one, 0, 3); }), "shamir_split threshold 0");
    CHECK(throws_invalid([&] { batch::shamir_split(one, 4, 3); }), "shamir_split threshold > share_count");
    CHECK(throws_invalid([&] { batch::shamir_combine(few, 3, ok); }), "shamir_combine with too few shares");
    CHECK(throws_invalid([&] { batch::shamir_combine(few, 0, ok); }), "shamir_combine threshold 0");
    if (g_bad) {
        std::printf("%d checks failed\n", g_bad);
        return 1;
    }
    std::printf("shamir batch ok\n");
    return 0;
}
