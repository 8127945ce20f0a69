// pow.hip -- batched proof-of-work search and check, gfx950.
//
// Every PoW in the reference hashes  SHA-256(prefix || BE64(candidate))  and takes the FIRST
// candidate, in attempt order, whose digest has >= difficulty leading zero bits:
//   store      src/security/StoreProof.cpp:39-52 (pow_digest), :124-146 (compute_store_pow):
//              candidates = successive std::mt19937_64(LE64(digest(nonce 0)[0..8])) outputs
//   announce   src/core/Node.cpp:155-171 (digest), :200-230 (compute_announce_pow)
//   handshake  src/core/Node.cpp:233-245 (digest), :257-292 (compute_handshake_pow):
//              candidates = start + attempt, start = first std::mt19937_64(BE64(digest(0)[0..8]))
//   leading-zero count  Node.cpp:174-190 == StoreProof.cpp:61-80
//
// One workgroup per job (1..16 waves; the host picks enough waves per job that the grid holds
// ~4 waves per SIMD).  Each step tests 64*waves consecutive attempts, one per lane; a workgroup
// min-reduction over the successful attempt indices keeps the reference's first-found order
// exactly, and the job stops at the first step that finds one.  Per job, once:
//   * the prefix's whole 64-byte blocks are absorbed into a midstate;
//   * the final block(s) become a template (tail || 8 zero nonce bytes || 0x80 || BE64 length)
//     and the SHA rounds before the nonce's first word (q = tail/4 of them) are precomputed, so
//     a candidate costs 64 - q rounds (+ one more compression when the tail is > 47 bytes);
//     q is workgroup-uniform and dispatched to 16 straight-line variants;
//   * the mt19937_64 state lives in LDS; the workgroup twists it cooperatively (groups of
//     <= 156 words keep the in-place recurrence's read-old / read-new order) and tempers 312
//     candidates at a time into an LDS ring the lanes read.
// No MFMA, no atomics, no host round trips: one launch per batch.
#include "pow_common.hpp"

namespace enet {

__global__ __launch_bounds__(1024) void pow_search_kernel(PowParams P) {
    extern __shared__ uint64_t smem[];
    const uint32_t job = blockIdx.x;
    const uint32_t tid = threadIdx.x;
    const uint32_t diff = P.difficulty[job];
    if (diff == 0u) {  // compute_store_pow / compute_*_pow: difficulty 0 -> nonce 0
        if (tid == 0) {
            P.nonces[job] = 0;
            if (P.attempts) P.attempts[job] = 0;
            P.found[job] = 1;
        }
        return;
    }
    const uint64_t off = P.off[job];
    PowTemplate T;
    // The prefix address is workgroup-uniform, so the compiler would fetch it with scalar
    // (SMEM) loads -- which ignore the low two address bits.  Prefixes start at arbitrary byte
    // offsets: keep the pointer in VGPRs so the loads are vector loads (unaligned-safe).
    const uint8_t* pre = P.prefixes + off;
    asm volatile("" : "+v"(pre));
    pow_prepare(pre, P.off[job + 1] - off, T);
    pow_uniform(T);
    const PowFound f = pow_search_run(T, diff, P.schedule, P.max_attempts, P.ring, smem);
    if (tid == 0) {
        P.found[job] = f.ok ? 1 : 0;
        P.nonces[job] = f.nonce;
        if (P.attempts) P.attempts[job] = f.attempt;
    }
}

// store_pow_valid / announce_pow_valid: one lane per job (difficulty 0 -> valid).
__global__ __launch_bounds__(kWG) void pow_check_kernel(PowParams P) {
    const uint32_t job = blockIdx.x * kWG + threadIdx.x;
    if (job >= P.n) return;
    const uint32_t diff = P.difficulty[job];
    uint8_t ok = 1;
    if (diff != 0u) {
        const uint64_t off = P.off[job];
        PowTemplate T;
        pow_prepare(P.prefixes + off, P.off[job + 1] - off, T);
        uint32_t st[8];
        ok = pow_hash<false>(T, P.check_nonces[job], st) >= diff ? 1 : 0;
    }
    P.found[job] = ok;
}

hipError_t launch_pow_search(const PowParams& p, uint32_t waves, hipStream_t s) {
    if (p.n == 0) return hipSuccess;
    const size_t lds = pow_search_lds_words(p.ring, waves) * sizeof(uint64_t);
    hipLaunchKernelGGL(pow_search_kernel, dim3(p.n), dim3(64 * waves), lds, s, p);
    return hipGetLastError();
}

hipError_t launch_pow_check(const PowParams& p, hipStream_t s) {
    if (p.n == 0) return hipSuccess;
    hipLaunchKernelGGL(pow_check_kernel, dim3((p.n + kWG - 1) / kWG), dim3(kWG), 0, s, p);
    return hipGetLastError();
}

}  // namespace enet
