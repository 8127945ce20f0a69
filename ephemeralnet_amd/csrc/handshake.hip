// handshake.hip -- the device session table (gfx950): batched handshake admission, key rotation
// and the plain key exchange, one record per lane.
//
// Reference behaviour (ShardianLabs/EphemeralNet), in Node::perform_handshake's order
// (src/core/Node.cpp:1872-1926):
//   KeyExchange::validate_public         src/network/KeyExchange.cpp:30-32   1 < c < 2^31-1
//   handshake_pow_valid / _digest        src/core/Node.cpp:232-256           SHA-256 of 96 bytes
//   KeyExchange::modexp / derive_shared_secret  KeyExchange.cpp:9-48        SHA-256(BE32(scalar))
//   make_handshake_material              Node.cpp:61-75                      BE32(min) || BE32(max)
//   KeyManager::register_session_with_material  src/network/KeyManager.cpp:32-46
//   KeyManager::rotate_if_needed / derive_key   KeyManager.cpp:56-92
//
// Every hash here has a fixed, short message, so each is built in registers as whole 16-word
// blocks (no arena, no byte loop): an accepted handshake is 9 compressions (2 PoW, 1 secret,
// 4 HMAC, 2 midstates), a rejected one at most 2.  The table rows a lane writes are its own
// slot's (the caller keeps the slots of one batch distinct), so there are no atomics.
#include "enet_device.hpp"
#include "enet_internal.hpp"

namespace enet {

namespace {

constexpr uint32_t kDhPrime = 2147483647u;  // KeyExchange::kPrime = 2^31 - 1
constexpr uint32_t kDhGenerator = 5u;       // KeyExchange::kGenerator

// a * b mod 2^31-1 for a, b < 2^31-1, exact: 2^31 == 1, so the 62-bit product folds twice
// (first sum < 2^32, second <= P + 1) and one conditional subtraction finishes it.
__device__ __forceinline__ uint32_t mulmod_p(uint32_t a, uint32_t b) {
    const uint64_t prod = (uint64_t)a * b;
    const uint64_t s = (prod & kDhPrime) + (prod >> 31);
    uint32_t r = ((uint32_t)s & kDhPrime) + (uint32_t)(s >> 31);
    if (r >= kDhPrime) r -= kDhPrime;
    return r;
}

// KeyExchange::modexp(base, exponent, kPrime) for base < kPrime (the caller reduces, as the
// reference's `base %= modulus`): exponent 0 -> 1, base 0 with exponent > 0 -> 0.
__device__ __forceinline__ uint32_t modexp_p(uint32_t base, uint32_t exponent) {
    uint32_t result = 1u;
    while (exponent != 0u) {
        if (exponent & 1u) result = mulmod_p(result, base);
        base = mulmod_p(base, base);
        exponent >>= 1;
    }
    return result;
}

// remote % kPrime for a 32-bit remote (< 2^32 < 3 P)
__device__ __forceinline__ uint32_t reduce_p(uint32_t v) {
    if (v >= kDhPrime) v -= kDhPrime;
    if (v >= kDhPrime) v -= kDhPrime;
    return v;
}

// KeyExchange::derive_shared_secret: SHA-256 of the 4 bytes BE32(scalar), as big-endian words
__device__ __forceinline__ void shared_secret(uint32_t scalar, uint32_t secret[8]) {
    uint32_t w[16];
    w[0] = scalar;
    w[1] = 0x80000000u;
#pragma unroll
    for (int j = 2; j < 15; ++j) w[j] = 0u;
    w[15] = 4 * 8;
    sha256_init(secret);
    sha256_compress(secret, w);
}

// The shared hmac32_short / hmac_midstates (enet_device.hpp), written out over one w[16].  These
// two kernels run one wave per SIMD, so their time is one wave's instruction schedule: built from
// the shared pieces, the same 8 198 instructions were allocated 93 VGPRs instead of 130 and ran
// 1.5-3 % slower (accept 32.2 -> 32.7 us, rotate 18.8 -> 19.4 us, profiles/hash_vocab_ab.jsonl).
template <int NW>
__device__ __forceinline__ void hs_hmac32_short(const uint32_t kb[8], const uint32_t m[NW], uint32_t out[8]) {
    uint32_t st[8], w[16];
    sha256_init(st);
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = (j < 8 ? kb[j] : 0u) ^ kHmacIpad;
    sha256_compress(st, w);
#pragma unroll
    for (int j = 0; j < 15; ++j) w[j] = j < NW ? m[j] : (j == NW ? 0x80000000u : 0u);
    w[15] = (64 + 4 * NW) * 8;
    sha256_compress(st, w);
    sha256_init(out);
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = (j < 8 ? kb[j] : 0u) ^ kHmacOpad;
    sha256_compress(out, w);
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j] = st[j];
    w[8] = 0x80000000u;
#pragma unroll
    for (int j = 9; j < 15; ++j) w[j] = 0u;
    w[15] = (64 + 32) * 8;
    sha256_compress(out, w);
}

// the enet_hmac_midstates layout for one key: inner state at mid[0..8), outer at mid[8..16)
__device__ __forceinline__ void store_midstates(const uint32_t kb[8], uint32_t* __restrict__ mid) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const uint32_t pad = pass == 0 ? kHmacIpad : kHmacOpad;
        uint32_t st[8], w[16];
        sha256_init(st);
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = (j < 8 ? kb[j] : 0u) ^ pad;
        sha256_compress(st, w);
#pragma unroll
        for (int j = 0; j < 8; ++j) mid[8 * pass + j] = st[j];
    }
}

// 8 big-endian words as 32 bytes at a 4-byte-aligned row
__device__ __forceinline__ void store_row(uint8_t* __restrict__ row, const uint32_t v[8]) {
    uint32_t* o = reinterpret_cast<uint32_t*>(row);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = bswap32(v[j]);
}

}  // namespace

__global__ __launch_bounds__(kWG) void handshake_accept_kernel(HandshakeParams P) {
    const uint32_t i = blockIdx.x * kWG + threadIdx.x;
    if (i >= P.n) return;
    const uint32_t remote = P.remote_public[i];
    if (!(remote > 1u && remote < kDhPrime)) {
        P.verdict[i] = ENET_DEV_HS_BAD_PUBLIC;
        return;
    }
    if (P.difficulty != 0u) {
        // BE64(32) || peer_id || BE64(32) || local_id || BE64(remote_public) || BE64(nonce)
        const uint32_t* pid = reinterpret_cast<const uint32_t*>(P.peer_ids + 32ull * i);
        const uint32_t* lid = reinterpret_cast<const uint32_t*>(P.local_id);
        const uint64_t nonce = P.work_nonce[i];
        uint32_t st[8], w[16];
        w[0] = 0u; w[1] = 32u;
#pragma unroll
        for (int j = 0; j < 8; ++j) w[2 + j] = bswap32(pid[j]);
        w[10] = 0u; w[11] = 32u;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[12 + j] = bswap32(lid[j]);
        sha256_init(st);
        sha256_compress(st, w);
#pragma unroll
        for (int j = 0; j < 4; ++j) w[j] = bswap32(lid[4 + j]);
        w[4] = 0u; w[5] = remote;
        w[6] = (uint32_t)(nonce >> 32); w[7] = (uint32_t)nonce;
        w[8] = 0x80000000u;
#pragma unroll
        for (int j = 9; j < 15; ++j) w[j] = 0u;
        w[15] = 96 * 8;
        sha256_compress(st, w);
        if (digest_leading_zero_bits(st) < P.difficulty) {
            P.verdict[i] = ENET_DEV_HS_BAD_POW;
            return;
        }
    }
    const uint32_t slot = P.slot ? P.slot[i] : i;
    if (slot >= P.table.sessions) {
        P.verdict[i] = ENET_DEV_HS_BAD_SLOT;
        return;
    }
    uint32_t secret[8], key[8];
    shared_secret(modexp_p(reduce_p(remote), P.local_private), secret);
    const uint32_t material[2] = {remote < P.local_public ? remote : P.local_public,
                                  remote < P.local_public ? P.local_public : remote};
    hs_hmac32_short<2>(secret, material, key);
    store_row(P.table.secrets + 32ull * slot, secret);
    store_row(P.table.keys + 32ull * slot, key);
    store_midstates(key, P.table.mid + 16ull * slot);
    P.table.counters[slot] = 0ull;
    P.table.last_rotation[slot] = P.now;
    P.table.live[slot] = 1;
    P.verdict[i] = ENET_DEV_HS_OK;
}

__global__ __launch_bounds__(kWG) void session_rotate_kernel(SessionTableParams T, int64_t now, int64_t interval,
                                                             uint8_t* __restrict__ rotated) {
    const uint32_t s = blockIdx.x * kWG + threadIdx.x;
    if (s >= T.sessions) return;
    // now - last_rotation in wrapping arithmetic (the reference subtracts two time_points)
    const bool due = T.live[s] != 0 &&
                     (int64_t)((uint64_t)now - (uint64_t)T.last_rotation[s]) >= interval;
    if (!due) {
        rotated[s] = 0;
        return;
    }
    const uint64_t c = T.counters[s] + 1ull;
    const uint32_t* sp = reinterpret_cast<const uint32_t*>(T.secrets + 32ull * s);
    uint32_t secret[8], key[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) secret[j] = bswap32(sp[j]);
    const uint32_t material[4] = {(uint32_t)(c >> 32), (uint32_t)c, (uint32_t)((uint64_t)now >> 32),
                                  (uint32_t)(uint64_t)now};
    hs_hmac32_short<4>(secret, material, key);
    T.counters[s] = c;
    T.last_rotation[s] = now;
    store_row(T.keys + 32ull * s, key);
    store_midstates(key, T.mid + 16ull * s);
    rotated[s] = 1;
}

__global__ __launch_bounds__(kWG) void key_exchange_kernel(uint32_t n, const uint32_t* __restrict__ privates,
                                                           const uint32_t* __restrict__ remotes,
                                                           uint32_t* __restrict__ public_out,
                                                           uint8_t* __restrict__ secret_out) {
    const uint32_t i = blockIdx.x * kWG + threadIdx.x;
    if (i >= n) return;
    const uint32_t priv = privates[i];
    if (public_out) public_out[i] = modexp_p(kDhGenerator, priv);
    if (remotes && secret_out) {
        uint32_t secret[8];
        shared_secret(modexp_p(reduce_p(remotes[i]), priv), secret);
        store_row(secret_out + 32ull * i, secret);
    }
}

static uint32_t blocks_for(uint32_t n) { return (uint32_t)(((uint64_t)n + kWG - 1) / kWG); }

hipError_t launch_handshake_accept(const HandshakeParams& p, hipStream_t s) {
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(handshake_accept_kernel, dim3(blocks_for(p.n)), dim3(kWG), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_session_rotate(const SessionTableParams& t, int64_t now, int64_t interval, uint8_t* rotated,
                                 hipStream_t s) {
    if (t.sessions == 0) return hipSuccess;
    hipLaunchKernelGGL(session_rotate_kernel, dim3(blocks_for(t.sessions)), dim3(kWG), 0, s, t, now, interval,
                       rotated);
    return hipGetLastError();
}

hipError_t launch_key_exchange(uint32_t n, const uint32_t* privates, const uint32_t* remotes, uint32_t* public_out,
                               uint8_t* secret_out, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(key_exchange_kernel, dim3(blocks_for(n)), dim3(kWG), 0, s, n, privates, remotes, public_out,
                       secret_out);
    return hipGetLastError();
}

}  // namespace enet
