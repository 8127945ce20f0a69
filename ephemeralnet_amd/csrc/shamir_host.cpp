// shamir_host.cpp -- the reference's scalar Shamir API (include/ephemeralnet/crypto/Shamir.hpp;
// reference src/crypto/Shamir.cpp:114-163) on the calling thread: one 32-byte secret per call is
// ~100 field multiplies, far below a device round trip.  The field is gf256.hpp's (0x11D,
// table-free), the same definition the kernels of shamir.hip use for whole batches.
#include "ephemeralnet/crypto/Shamir.hpp"

#include <cstring>
#include <random>

#include "gf256.hpp"

namespace ephemeralnet::crypto {

namespace gf = enet::gf256;

std::vector<ShamirShare> Shamir::split(const std::array<std::uint8_t, 32>& secret, std::uint8_t threshold,
                                       std::uint8_t share_count) {
    if (threshold == 0 || share_count == 0)
        throw std::invalid_argument("Shamir::split: threshold and share_count must be at least 1");
    if (threshold > share_count) throw std::invalid_argument("Shamir::split: threshold is larger than share_count");

    // coefficient words c[d - 1][w], d = 1 .. threshold-1: one std::random_device (the source of
    // CryptoManager's fill_random_bytes, CryptoManager.cpp:17-24) per call, every draw used whole
    std::vector<std::uint32_t> c(8u * (threshold - 1u));
    if (!c.empty()) {
        std::random_device rd;
        for (auto& word : c) word = static_cast<std::uint32_t>(rd());
    }
    std::uint32_t s[8];
    std::memcpy(s, secret.data(), 32);

    std::vector<ShamirShare> shares(share_count);
    for (unsigned j = 0; j < share_count; ++j) {  // unsigned: 255 shares end the loop (Shamir.cpp:131 wraps)
        const auto x = static_cast<std::uint8_t>(j + 1);
        shares[j].index = x;
        std::uint32_t v[8];
        for (unsigned w = 0; w < 8; ++w) {  // Horner: the field element evaluate_polynomial gives (:68-80)
            std::uint32_t acc = 0;
            for (unsigned d = threshold - 1u; d >= 1; --d) acc = gf::mul4(acc ^ c[8 * (d - 1) + w], x);
            v[w] = acc ^ s[w];
        }
        std::memcpy(shares[j].value.data(), v, 32);
    }
    return shares;
}

std::array<std::uint8_t, 32> Shamir::combine(const std::vector<ShamirShare>& shares, std::uint8_t threshold) {
    if (shares.size() < threshold) throw std::invalid_argument("Shamir::combine: fewer shares than threshold");

    std::uint32_t acc[8] = {};
    for (unsigned i = 0; i < threshold; ++i) {  // the first `threshold` shares, in the caller's order (:161)
        std::uint8_t num = 1, den = 1;
        for (unsigned j = 0; j < threshold; ++j) {
            if (j == i) continue;
            num = gf::mul(num, shares[j].index);
            den = gf::mul(den, static_cast<std::uint8_t>(shares[j].index ^ shares[i].index));
        }
        std::uint32_t v[8];
        std::memcpy(v, shares[i].value.data(), 32);
        if (den == 0) {
            // the reference divides only for a non-zero value byte (:90-92) and throws there (:54-56)
            std::uint32_t any = 0;
            for (unsigned w = 0; w < 8; ++w) any |= v[w];
            if (any != 0) throw std::invalid_argument("Shamir::combine: two shares with the same index (division by zero)");
            continue;
        }
        const std::uint8_t factor = gf::mul(num, gf::inv(den));
        for (unsigned w = 0; w < 8; ++w) acc[w] ^= gf::mul4(v[w], factor);
    }
    std::array<std::uint8_t, 32> secret{};
    std::memcpy(secret.data(), acc, 32);
    return secret;
}

}  // namespace ephemeralnet::crypto
