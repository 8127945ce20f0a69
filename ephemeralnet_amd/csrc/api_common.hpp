// api_common.hpp -- small host helpers shared by the translation units of the C++ drop-in
// (scalar_api.cpp, batch_records.cpp, batch_staged.cpp): the packed views of the reference's
// value types, argument checks, big-endian writers, the enet_records filler.
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <random>
#include <span>
#include <stdexcept>
#include <string>

#include "enet_crypto.h"
#include "ephemeralnet/crypto/CryptoTypes.hpp"
#include "ephemeralnet/security/StoreProof.hpp"

namespace enet::api {

using Records = std::span<const std::span<const std::uint8_t>>;  // one span per record
using Keys32 = std::span<const std::array<std::uint8_t, 32>>;

static_assert(sizeof(ephemeralnet::crypto::Key) == 32 && sizeof(ephemeralnet::crypto::Nonce) == 12 && sizeof(ephemeralnet::ChunkId) == 32,
              "crypto::Key / Nonce / ChunkId are passed to the device as packed arrays");
inline const std::uint8_t* key_bytes(std::span<const ephemeralnet::crypto::Key> k) {
    return reinterpret_cast<const std::uint8_t*>(k.data());
}
inline const std::uint8_t* nonce_bytes(std::span<const ephemeralnet::crypto::Nonce> n) {
    return reinterpret_cast<const std::uint8_t*>(n.data());
}

// every per-record array of a batch call has one entry per record (`also`: a further condition
// reported the same way)
inline void check_sizes(const char* name, std::size_t n, std::initializer_list<std::size_t> sizes, bool also = true) {
    const bool ok = also && std::all_of(sizes.begin(), sizes.end(), [n](std::size_t s) { return s == n; });
    if (!ok) throw std::invalid_argument(std::string("enet batch::") + name + ": size mismatch");
}
// the size of an array that may be left empty
template <class T>
std::size_t optional_size(std::span<T> s, std::size_t n) {
    return s.empty() ? n : s.size();
}

inline void check_count(std::size_t n, const char* what) {
    if (n > 0xFFFFFFFFull) throw std::invalid_argument(std::string("enet batch::") + what + ": too many records");
}

inline void check_sessions(std::span<const std::uint32_t> session, std::size_t K, const char* what) {
    for (std::uint32_t s : session)
        if (s >= K) throw std::invalid_argument(std::string("enet batch::") + what + ": session index outside the table");
}

// big-endian, most significant byte first, through an output iterator
template <class It>
It put_be64(It out, std::uint64_t x) {
    for (int s = 56; s >= 0; s -= 8) *out++ = static_cast<std::uint8_t>(x >> s);
    return out;
}
template <class It>
It put_be32(It out, std::uint32_t x) {
    for (int s = 24; s >= 0; s -= 8) *out++ = static_cast<std::uint8_t>(x >> s);
    return out;
}

inline void fill_random_bytes(std::span<std::uint8_t> buffer) {  // CryptoManager.cpp:17-24
    std::random_device rd;
    for (auto& b : buffer) b = static_cast<std::uint8_t>(rd());
}

inline std::uint8_t clamp_store_difficulty(std::uint8_t d) {  // StoreProof.cpp:114-116, 128-130
    return d > ephemeralnet::security::kMaxStorePowDifficulty ? ephemeralnet::security::kMaxStorePowDifficulty : d;
}

// The records descriptor of a device call over device-visible arrays: keys [n][32], nonces
// [n][12] or null; hints 0 = not given.
inline enet_records records_of(std::size_t n, const std::uint64_t* in_off, const std::uint64_t* out_off,
                               const std::uint8_t* in, std::uint8_t* out, const std::uint8_t* keys,
                               const std::uint8_t* nonces, std::uint64_t total_bytes_hint = 0,
                               std::uint32_t max_len_hint = 0) {
    enet_records r{};
    r.count = static_cast<std::uint32_t>(n);
    r.in_offsets = in_off;
    r.out_offsets = out_off;
    r.in = in;
    r.out = out;
    r.keys = keys;
    r.key_stride = 32;
    r.nonces = nonces;
    r.total_bytes_hint = total_bytes_hint;
    r.max_len_hint = max_len_hint;
    return r;
}

}  // namespace enet::api
