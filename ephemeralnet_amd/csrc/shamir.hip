// shamir.hip -- Shamir split / combine of 32-byte secrets over GF(2^8)/0x11D for whole batches
// (reference: Shamir::split / Shamir::combine, src/crypto/Shamir.cpp:114-163, one key per call on
// a host core: Node::store_chunk, src/core/Node.cpp:1428, and Node::receive_chunk / fetch_chunk,
// :1632-1642, :1804-1813).  A thread owns one 32-bit word (four secret bytes) of one record, so a
// record is eight neighbouring lanes and every load and store is a whole aligned word; the field
// arithmetic is gf256.hpp's table-free SWAR multiply -- no LDS, no table indexed by key bytes.
// Both kernels loop over `threshold` (1 .. 255).  At the chunk pipeline's batch (65 536 x 3-of-5:
// ~17 MB split, ~9 MB combine) split takes ~12 us and combine ~25 us, the latter bound by the
// multiplies of its per-record factors, not by bytes (profiles/shamir_bench.json).
#include "enet_internal.hpp"
#include "gf256.hpp"

namespace enet {

namespace {

constexpr uint32_t kShamirMaxBlocks = 1u << 16;  // grid-stride beyond (grid.x * block.x < 2^32)

// shares[i][j] = sum_{d < t} c_d x^d with x = j + 1, c_0 = secrets[i], c_d = coeffs[i][d - 1]
// (evaluate_polynomial, Shamir.cpp:68-80, in Horner form: the same field element).  blockIdx.y is
// the share, so x is uniform over the launch dimension and the multiply's conditional xors are
// scalar decisions, the same for every lane of a wave.
__global__ __launch_bounds__(kWG) void shamir_split_kernel(uint32_t n, const uint32_t* __restrict__ secrets,
                                                           const uint32_t* __restrict__ coeffs, uint32_t threshold,
                                                           uint32_t share_count, uint32_t* __restrict__ shares) {
    const uint32_t j = blockIdx.y;
    const uint8_t x = (uint8_t)(j + 1u);
    const uint64_t words = 8ull * n;
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    for (uint64_t t = (uint64_t)blockIdx.x * kWG + threadIdx.x; t < words; t += stride) {
        const uint64_t rec = t >> 3;
        const uint32_t w = (uint32_t)t & 7u;
        uint32_t acc = 0;
        if (threshold > 1) {
            const uint32_t* c = coeffs + rec * (threshold - 1) * 8ull + w;
            acc = c[8ull * (threshold - 2)];
            for (uint32_t d = threshold - 2; d >= 1; --d) acc = gf256::mul4(acc, x) ^ c[8ull * (d - 1)];
            acc = gf256::mul4(acc, x);
        }
        shares[(rec * share_count + j) * 8ull + w] = acc ^ secrets[t];
    }
}

// Lagrange interpolation at 0 over the first `threshold` shares of each record, in the caller's
// order (interpolate, Shamir.cpp:82-110): secret = sum_i value_i * prod_{j != i} x_j / (x_j ^ x_i).
// The indices differ per record, so the factors are per lane (the eight lanes of a record compute
// the same ones), four shares' factors at a time in the packed bytes of one word: one inversion
// (13 multiplies) serves four shares.  A zero denominator means two equal indices: the record
// fails closed.
__global__ __launch_bounds__(kWG) void shamir_combine_kernel(uint32_t n, uint32_t threshold,
                                                             const uint8_t* __restrict__ indices,
                                                             const uint32_t* __restrict__ values,
                                                             uint32_t* __restrict__ secrets_out,
                                                             uint8_t* __restrict__ ok) {
    const uint64_t words = 8ull * n;
    const uint64_t stride = (uint64_t)gridDim.x * kWG;
    for (uint64_t t = (uint64_t)blockIdx.x * kWG + threadIdx.x; t < words; t += stride) {
        const uint64_t rec = t >> 3;
        const uint32_t w = (uint32_t)t & 7u;
        const uint8_t* idx = indices + rec * threshold;
        const uint32_t* val = values + rec * threshold * 8ull + w;
        uint32_t acc = 0;
        bool good = true;
        for (uint32_t g = 0; g < threshold; g += 4) {  // the factors of shares g .. g+3, one per packed byte
            const uint32_t m = threshold - g < 4u ? threshold - g : 4u;
            uint32_t xi = 0;
            for (uint32_t k = 0; k < m; ++k) xi |= (uint32_t)idx[g + k] << (8 * k);
            uint32_t num = 0x01010101u, den = 0x01010101u;
            for (uint32_t j = 0; j < threshold; ++j) {
                const uint32_t xj = idx[j] * 0x01010101u;
                // share j's own byte takes the factor 1 in both products (its xj ^ xi is 0)
                const uint32_t self = j - g < 4u ? 0xFFu << (8 * (j - g)) : 0u;
                num = gf256::mul4x4(num, (xj & ~self) | (0x01010101u & self));
                den = gf256::mul4x4(den, (xj ^ xi) | (0x01010101u & self));
            }
            const uint32_t factor = gf256::mul4x4(num, gf256::inv4(den));
            for (uint32_t k = 0; k < m; ++k) {
                good = good && ((den >> (8 * k)) & 0xFFu) != 0;
                acc ^= gf256::mul4(val[8ull * (g + k)], (uint8_t)(factor >> (8 * k)));
            }
        }
        secrets_out[t] = good ? acc : 0u;
        if (w == 0) ok[rec] = good ? 1 : 0;
    }
}

uint32_t shamir_blocks(uint32_t n) {
    const uint64_t b = (8ull * n + kWG - 1) / kWG;
    return (uint32_t)(b < kShamirMaxBlocks ? b : kShamirMaxBlocks);
}

}  // namespace

hipError_t launch_shamir_split(uint32_t n, const uint8_t* secrets, const uint8_t* coeffs, uint32_t threshold,
                               uint32_t share_count, uint8_t* shares, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(shamir_split_kernel, dim3(shamir_blocks(n), share_count), dim3(kWG), 0, s, n,
                       reinterpret_cast<const uint32_t*>(secrets), reinterpret_cast<const uint32_t*>(coeffs),
                       threshold, share_count, reinterpret_cast<uint32_t*>(shares));
    return hipGetLastError();
}

hipError_t launch_shamir_combine(uint32_t n, uint32_t threshold, const uint8_t* indices, const uint8_t* values,
                                 uint8_t* secrets_out, uint8_t* ok, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(shamir_combine_kernel, dim3(shamir_blocks(n)), dim3(kWG), 0, s, n, threshold, indices,
                       reinterpret_cast<const uint32_t*>(values), reinterpret_cast<uint32_t*>(secrets_out), ok);
    return hipGetLastError();
}

}  // namespace enet
