// Shamir.hpp -- drop-in for the reference include/ephemeralnet/crypto/Shamir.hpp:12-25.  Same
// types and signatures, same results and the same std::invalid_argument cases
// (src/crypto/Shamir.cpp:114-163); GF(2^8)/0x11D multiplied without tables, on the calling
// thread.  split draws its coefficients from std::random_device once per call and returns 255
// shares for share_count == 255 (the reference's uint8_t loop counter wraps there, :131).
// Batches of keys: crypto::batch::shamir_split / shamir_combine (Batch.hpp) and
// enet_shamir_*_batch on the MI355X.
#pragma once

#include "ephemeralnet/crypto/CryptoTypes.hpp"

#include <array>
#include <cstdint>
#include <stdexcept>
#include <vector>

#ifndef ENET_CXX_API
#define ENET_CXX_API __attribute__((visibility("default")))
#endif

namespace ephemeralnet::crypto {

struct ShamirShare {
    std::uint8_t index{0};
    std::array<std::uint8_t, 32> value{};
};

class ENET_CXX_API Shamir {
public:
    static std::vector<ShamirShare> split(const std::array<std::uint8_t, 32>& secret,
                                          std::uint8_t threshold,
                                          std::uint8_t share_count);

    static std::array<std::uint8_t, 32> combine(const std::vector<ShamirShare>& shares,
                                                std::uint8_t threshold);
};

}  // namespace ephemeralnet::crypto
