// duplex_common.hpp -- what the two duplex kernels (duplex.hip: one cipher + one hash lane per
// record; duplex_split.hip: four waves per record) say the same way: a record's geometry, the
// ragged-end byte helpers, the LDS-only barrier, the AEAD lane (RFC 8439 one-time key, Poly1305
// absorb, tag) and the per-record epilogue.
#pragma once

#include "enet_device.hpp"
#include "enet_internal.hpp"

namespace enet {

constexpr uint32_t kDxRun = 128;  // bytes per stage and record

// all waves: this wave's LDS traffic is done, then meet (no vmcnt drain)
#define ENET_DX_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// keep bytes [0, r) of the LE byte string in w[0..N)
template <int N>
__device__ __forceinline__ void keep_le(uint32_t* w, uint32_t r) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        const uint32_t b = 4u * j;
        const uint32_t m = b + 4u <= r ? 0xffffffffu : (b >= r ? 0u : (1u << (8u * (r - b))) - 1u);
        w[j] &= m;
    }
}

__device__ __forceinline__ void zero_bytes(uint8_t* p, uint64_t n) {
    const uint32_t z[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint64_t o = 0; o < n; o += 64) store_block(p + o, (uint32_t)min<uint64_t>(64, n - o), z);
}

// One record as every lane that serves it sees it.
struct DuplexGeom {
    bool live, ordered, valid;
    uint32_t rec;
    uint64_t ib, Li, ob, Lo;  // input / output offset and length
    uint64_t Lm;              // message bytes (0 unless valid)
    // whole 128-byte stages; the ragged end (< 128) and its message offset
    __device__ __forceinline__ uint32_t Ts() const { return (uint32_t)(Lm / kDxRun); }
    __device__ __forceinline__ uint64_t tb() const { return (uint64_t)kDxRun * Ts(); }
    __device__ __forceinline__ uint32_t r() const { return (uint32_t)(Lm - tb()); }
};

// live / rec / offsets / lengths of the record at batch position pos
__device__ __forceinline__ DuplexGeom duplex_geom(const DuplexParams& p, uint32_t pos) {
    DuplexGeom g{};
    g.live = pos < p.n;
    g.rec = g.live ? (p.order ? p.order[pos] : pos) : 0u;
    g.ordered = true;  // offsets non-decreasing: a decreasing pair would wrap Li / Lo to ~2^64
    if (g.live) {
        g.ib = p.in_off[g.rec];
        const uint64_t ie = p.in_off[g.rec + 1];
        g.ob = p.out_off[g.rec];
        const uint64_t oe = p.out_off[g.rec + 1];
        g.ordered = ie >= g.ib && oe >= g.ob;
        g.Li = g.ordered ? ie - g.ib : 0u;
        g.Lo = g.ordered ? oe - g.ob : 0u;  // nothing is zeroed for a disordered record
    }
    return g;
}

// the kind's rule gives the message length and whether the record's lengths fit it
__device__ __forceinline__ void duplex_geom_message(DuplexGeom& g, uint64_t Lm, bool fits) {
    g.valid = g.live && g.ordered && fits;
    g.Lm = g.valid ? Lm : 0u;
}

// RFC 8439 AEAD state of one record: Poly1305 key halves and accumulator
struct AeadLane {
    PolyR32 PR;
    uint32_t h[5], pad[4];
};

// one-time key = keystream block 0 (RFC 8439 2.6)
__device__ __forceinline__ void aead_lane_init(AeadLane& A, const ChachaRecord& R) {
    uint32_t otk[16];
    chacha_block(R, 0u, otk);
    A.PR = polyr32_make(otk[0], otk[1], otk[2], otk[3]);
    A.pad[0] = otk[4]; A.pad[1] = otk[5]; A.pad[2] = otk[6]; A.pad[3] = otk[7];
}

// `blocks` <= 8 whole 16-byte blocks of ciphertext (the caller zero-pads the last)
__device__ __forceinline__ void aead_absorb(AeadLane& A, const uint32_t* w, uint32_t blocks) {
#pragma unroll
    for (uint32_t q = 0; q < 8; ++q)
        if (q < blocks) poly32_block(A.h, A.PR, w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3], 1u);
}

// lengths block (LE64 |aad| = 0, LE64 |ct| = Lm), then the tag
__device__ __forceinline__ void aead_tag(AeadLane& A, uint64_t Lm, uint32_t tag[4]) {
    poly32_block(A.h, A.PR, 0u, 0u, (uint32_t)Lm, (uint32_t)(Lm >> 32), 1u);
    uint32_t l[5];
    h32_to_limbs(A.h, l);
    pfinish(l, A.pad, tag);
}

// 0 when the 16 bytes at tp are the tag
__device__ __forceinline__ uint32_t tag_diff(const uint32_t tag[4], const uint8_t* tp) {
    return (tag[0] ^ ld32(tp)) | (tag[1] ^ ld32(tp + 4)) | (tag[2] ^ ld32(tp + 8)) | (tag[3] ^ ld32(tp + 12));
}

// The record's epilogue, d = its digest / MAC as LE words of its bytes.  Seal: store d at `put`;
// a record that was not processed has its output zeroed.  Open: d must equal the 32 bytes at
// `expect` and `diff` (the caller's other checks) be 0; write ok, and leave no plaintext of a
// failed or unprocessed record.  A null put / expect: the caller placed / compared d itself.
template <bool OPEN>
__device__ __forceinline__ void finish_record(const DuplexParams& p, const DuplexGeom& g, const uint32_t d[8],
                                              uint8_t* put, const uint8_t* expect, uint32_t diff) {
    if (!g.live) return;
    if (!OPEN) {
        if (!g.valid) {
            zero_bytes(p.out + g.ob, g.Lo);
        } else if (put) {
            reinterpret_cast<uint4*>(put)[0] = make_uint4(d[0], d[1], d[2], d[3]);
            reinterpret_cast<uint4*>(put)[1] = make_uint4(d[4], d[5], d[6], d[7]);
        }
    } else {
        if (!g.valid) diff = 1u;
        if (g.valid && expect) {
#pragma unroll
            for (int j = 0; j < 8; ++j) diff |= ld32(expect + 4 * j) ^ d[j];
        }
        p.ok[g.rec] = diff == 0u ? 1 : 0;
        if (diff != 0u) zero_bytes(p.out + g.ob, g.Lo);
    }
}

}  // namespace enet
