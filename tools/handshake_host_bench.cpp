// handshake_host_bench.cpp -- one host thread admitting handshakes through the scalar drop-in API
// (profiles/handshake_bench.json "host"): per request, as Node::perform_handshake does it
// (src/core/Node.cpp:1872-1926), validate_public, the handshake PoW digest (one streaming Sha256,
// :232-244), a 32-bit modexp mod 2^31-1 + Sha256::digest of the scalar (derive_shared_secret) and
// HmacSha256::compute over the sorted publics (register_session_with_material).  The library
// defines no KeyExchange symbol, so the modexp is restated here.  Reads the requests
// tools/handshake_bench.py wrote (binary: n, difficulty, local id, local private, local public,
// then per request peer id, public, nonce), prints one JSON line: the median of 21 timed passes
// after 3 warm-up passes, and a digest of the keys for the caller to compare with the device's.
//   g++ -O2 -std=c++20 -I include tools/handshake_host_bench.cpp -L ephemeralnet_amd -lenet_crypto
//       -Wl,-rpath,$PWD/ephemeralnet_amd -o <program>      (one command line)
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <span>
#include <vector>

#include "ephemeralnet/crypto/HmacSha256.hpp"
#include "ephemeralnet/crypto/Sha256.hpp"

using ephemeralnet::crypto::HmacSha256;
using ephemeralnet::crypto::Sha256;

static constexpr std::uint32_t kPrime = 2147483647u;

static std::uint32_t modexp(std::uint64_t base, std::uint32_t exponent) {
    std::uint64_t result = 1;
    base %= kPrime;
    while (exponent > 0) {
        if (exponent & 1u) result = (result * base) % kPrime;
        base = (base * base) % kPrime;
        exponent >>= 1u;
    }
    return (std::uint32_t)result;
}

static void be64(std::uint64_t v, std::uint8_t* out) {
    for (int i = 0; i < 8; ++i) out[i] = (std::uint8_t)(v >> (56 - 8 * i));
}

static unsigned leading_zero_bits(const std::array<std::uint8_t, 32>& d) {
    unsigned total = 0;
    for (std::uint8_t b : d) {
        if (b == 0) {
            total += 8;
            continue;
        }
        return total + (unsigned)__builtin_clz((unsigned)b) - 24;
    }
    return total;
}

struct Request {
    std::uint8_t peer[32];
    std::uint32_t pub;
    std::uint64_t nonce;
};

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::uint32_t n = 0, difficulty = 0, local_private = 0, local_public = 0;
    std::uint8_t local_id[32];
    bool ok = std::fread(&n, 4, 1, f) == 1 && std::fread(&difficulty, 4, 1, f) == 1 &&
              std::fread(local_id, 32, 1, f) == 1 && std::fread(&local_private, 4, 1, f) == 1 &&
              std::fread(&local_public, 4, 1, f) == 1;
    std::vector<Request> reqs(ok ? n : 0);
    for (auto& q : reqs)
        ok = ok && std::fread(q.peer, 32, 1, f) == 1 && std::fread(&q.pub, 4, 1, f) == 1 &&
             std::fread(&q.nonce, 8, 1, f) == 1;
    std::fclose(f);
    if (!ok) return 2;

    std::vector<std::array<std::uint8_t, 32>> keys(n);
    std::vector<std::uint8_t> verdict(n);
    auto pass = [&] {
        for (std::uint32_t i = 0; i < n; ++i) {
            const Request& q = reqs[i];
            keys[i] = {};
            if (!(q.pub > 1u && q.pub < kPrime)) {
                verdict[i] = 0;
                continue;
            }
            if (difficulty != 0) {
                std::uint8_t len[8], tail[16];
                be64(32, len);
                be64(q.pub, tail);
                be64(q.nonce, tail + 8);
                Sha256 h;
                h.update(len);
                h.update(std::span<const std::uint8_t>(q.peer, 32));
                h.update(len);
                h.update(std::span<const std::uint8_t>(local_id, 32));
                h.update(tail);
                if (leading_zero_bits(h.finalize()) < difficulty) {
                    verdict[i] = 2;
                    continue;
                }
            }
            const std::uint32_t scalar = modexp(q.pub, local_private);
            const std::uint8_t sb[4] = {(std::uint8_t)(scalar >> 24), (std::uint8_t)(scalar >> 16),
                                        (std::uint8_t)(scalar >> 8), (std::uint8_t)scalar};
            const auto secret = Sha256::digest(sb);
            const std::uint32_t lo = std::min(local_public, q.pub), hi = std::max(local_public, q.pub);
            const std::uint8_t material[8] = {(std::uint8_t)(lo >> 24), (std::uint8_t)(lo >> 16), (std::uint8_t)(lo >> 8),
                                              (std::uint8_t)lo, (std::uint8_t)(hi >> 24), (std::uint8_t)(hi >> 16),
                                              (std::uint8_t)(hi >> 8), (std::uint8_t)hi};
            keys[i] = HmacSha256::compute(secret, material);
            verdict[i] = 1;
        }
    };
    using clk = std::chrono::steady_clock;
    for (int w = 0; w < 3; ++w) pass();
    std::vector<double> ms;
    for (int rep = 0; rep < 21; ++rep) {
        const auto t0 = clk::now();
        pass();
        ms.push_back(std::chrono::duration<double, std::milli>(clk::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::uint32_t accepted = 0;
    for (auto v : verdict) accepted += v == 1;
    std::vector<std::uint8_t> flat(32ull * n);
    for (std::uint32_t i = 0; i < n; ++i) std::memcpy(flat.data() + 32ull * i, keys[i].data(), 32);
    const auto d = Sha256::digest(flat);
    char hex[65];
    for (int i = 0; i < 32; ++i) std::snprintf(hex + 2 * i, 3, "%02x", d[i]);
    std::printf("{\"requests\": %u, \"difficulty\": %u, \"accepted\": %u, \"runs\": 21, \"median_ms\": %.3f, "
                "\"min_ms\": %.3f, \"max_ms\": %.3f, \"us_per_request\": %.4f, \"keys_sha256\": \"%s\"}\n",
                n, difficulty, accepted, ms[10], ms.front(), ms.back(), 1e3 * ms[10] / n, hex);
    return 0;
}
