// duplex.hip -- one HBM pass of cipher + hash over ANY batch of records (gfx950).
//
// Three reference paths encrypt a record and hash the same bytes:
//   frames   protocol::encode_signed + SessionManager::send (Message.cpp:305-311,
//            SessionManager.cpp:362-387): body = ChaCha20_{K,N,0}(m || HMAC-SHA256_K(m)), optionally
//            behind the nonce(12) || BE32(|body|) wire header; receive reverses it
//            (SessionManager.cpp:760-822, Message.cpp:313-328);
//   chunks   Node::store_chunk / fetch_chunk (Node.cpp:1414-1417, 1644-1655): ChaCha20 from counter
//            LE32(chunk_id) (CryptoManager.cpp:8-13, 38-58) and SHA-256(m) (= derive_chunk_id);
//   AEAD+MAC RFC 8439 ChaCha20-Poly1305 with HMAC-SHA256_K(m) beside the tag (BASELINE config 5).
// SHA-256 is serial inside a record, so a record gets one lane for its hash; a 512-thread workgroup
// owns 256 records and splits into 4 "cipher" waves and 4 "hash" waves (waves w and w + 4 share a
// SIMD and a record set: lane l of both serves record 64 w + l).  The cipher lane streams its
// record in 128-byte stages (one stage prefetched in registers), runs ChaCha20 (and Poly1305 over
// the ciphertext), stores, and hands every stage's plaintext to the hash lane through a
// double-buffered LDS slab -- one workgroup barrier per stage.  The plaintext is never re-read
// from HBM.
//
// Unlike frames.hip (uniform lengths, multiple of 128 B, whole workgroups), nothing is assumed:
// every lane reads its own record's offsets, lengths may differ lane to lane (a workgroup runs
// the stages of its longest record; `order` -- e.g. length-sorted -- keeps workgroups balanced),
// record starts may have any alignment, and the ragged end of a record (< 128 bytes, plus the
// 32-byte MAC of a frame body) goes through a 160-byte LDS tail slot per record:
//   seal  T1 cipher loads the message tail and parks it in the slot (chunks / AEAD also encrypt
//            and store it); T2 hash lane hashes it (masked, SHA padding) and finishes the digest --
//            frames put the MAC bytes right behind the message tail in the slot; T3 (frames) the
//            cipher lane encrypts message tail || MAC as one run of body bytes and stores it.
//   open  T1 cipher loads the body tail, checks Poly1305 (AEAD), decrypts, stores the message
//            tail, parks it (frames: with the decrypted MAC) in the slot; T2 hash lane finishes,
//            compares, writes ok, and zeroes a failed record's output.
// A record whose output length does not match its input (frames: out = in + 32 + hdr) is not
// processed: its output range is zeroed and, when opening, ok = 0.
#include "duplex_common.hpp"

#include <cstdlib>

namespace enet {

namespace {

constexpr uint32_t kRun = kDxRun;

// A record's 160-byte LDS tail slot: bytes 0..127 in `trow` (the record's row of the stage slab
// the last stage left free), bytes 128..159 in `xrow`.  16-byte chunk swizzles (row = record):
// conflict-free ds_write_b128 (8-lane groups) and ds_read_b128 (16-lane groups) for the 128-byte
// runs (msw, also the stage slabs' swizzle) and the 32-byte extension (xsw).
struct TailSlot {
    uint8_t *trow, *xrow;
    uint32_t msw, xsw;
    __device__ __forceinline__ uint8_t* chunk(int c) const {
        return c < 8 ? trow + 16u * (c ^ msw) : xrow + 16u * ((c - 8) ^ xsw);
    }
    __device__ __forceinline__ uint8_t* slot_byte(uint32_t i) const {
        return i < kRun ? trow + 16u * ((i >> 4) ^ msw) + (i & 15u)
                        : xrow + 16u * (((i - kRun) >> 4) ^ xsw) + (i & 15u);
    }
    __device__ __forceinline__ void slot_put(const uint32_t* w, int chunks) const {  // slot words [0, 4 * chunks)
#pragma unroll
        for (int c = 0; c < 10; ++c)
            if (c < chunks)
                *reinterpret_cast<uint4*>(chunk(c)) = make_uint4(w[4 * c], w[4 * c + 1], w[4 * c + 2], w[4 * c + 3]);
    }
    __device__ __forceinline__ uint4 slot_chunk(int c) const { return *reinterpret_cast<const uint4*>(chunk(c)); }
};

// What the two lanes of a record share beside its geometry.
struct DuplexLane {
    uint32_t H, sid;   // frame header bytes (0 / 16); session index (session-keyed frames)
    uint32_t rl, Tmax; // the record's row in the workgroup; stages of the workgroup's longest record
    uint32_t kw[8];    // key, LE words
    uint8_t* ptb;      // stage slabs [2][RPW][128]
    uint64_t* odst_s;  // chunk fetch: each record's output base ...
    uint32_t* ots_s;   // ... and whole stages, for the line-wise plaintext stores
    TailSlot slot;
};

}  // namespace

// ================================================================== cipher lane
template <int KIND, bool OPEN, int RPW>
__device__ __forceinline__ void duplex_cipher_lane(const DuplexParams& p, const DuplexGeom& g, const DuplexLane& L) {
    constexpr uint32_t kBuf = RPW * kRun;
    // chunk fetch stores its plaintext line-wise from the slab (the frame and AEAD+HMAC opens keep
    // per-lane stores: at the 128-VGPR cap the line-wise form spilled there and cost C3 wire open
    // 4 %, 1 904 -> 1 981 us, r06 prof_c3w)
    constexpr bool kLines = OPEN && KIND == DK_CHUNK;
    const uint32_t H = L.H, rl = L.rl, Tmax = L.Tmax, rec = g.rec, Ts = g.Ts(), r = g.r();
    const uint32_t lane = rl & 63u, msw = L.slot.msw;
    const uint64_t tb = g.tb();
    const bool live = g.live, valid = g.valid;

    if (p.prio == 2) __builtin_amdgcn_s_setprio(2);
    const uint8_t* src = p.in + g.ib + (OPEN ? H : 0u);
    uint8_t* dst = p.out + g.ob + (OPEN ? 0u : H);
    const uint32_t off0 = OPEN ? H : 0u;  // offset of src inside the input record
    if (kLines) {
        L.odst_s[rl] = reinterpret_cast<uint64_t>(dst);  // read after the first stage barrier
        L.ots_s[rl] = Ts;
    }
    uint32_t nw[3];
    if (OPEN && KIND == DK_FRAME && H) {  // nonce = the frame's first 12 bytes (SessionManager.cpp:815-822)
#pragma unroll
        for (int i = 0; i < 3; ++i) nw[i] = valid ? ld32(p.in + g.ib + 4 * i) : 0u;
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) nw[i] = live ? ld32(p.nonces + 12ull * rec + 4 * i) : 0u;
    }
    ChachaRecord R;
    chacha_record_init(R, L.kw, nw);
    // ChaCha20::apply start counter: frames 0, chunks LE32(chunk_id) (u32 wrap), AEAD 1
    const uint32_t c0 = KIND == DK_FRAME ? 0u
                      : KIND == DK_CHUNK ? (live ? ld32(p.chunk_ids + 32ull * rec) : 0u)
                                         : 1u;
    AeadLane A{};
    if (KIND == DK_AEADH) aead_lane_init(A, R);

    uint32_t pf[32];
    auto load_run = [&](uint32_t s) {
        const uint4* q = reinterpret_cast<const uint4*>(src + (uint64_t)kRun * s);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint4 v = q[i];
            pf[4 * i] = v.x; pf[4 * i + 1] = v.y; pf[4 * i + 2] = v.z; pf[4 * i + 3] = v.w;
        }
    };
    auto put_run = [&](uint8_t* d, const uint32_t* v) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            *reinterpret_cast<uint4*>(d + 16u * (k ^ msw)) =
                make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    };
    // Chunk fetch: every stage's plaintext is in the slab (for the hash lane); it is stored from there
    // line by line one stage later (after the barrier that hands the slab to the hash lanes,
    // which only read it; the cipher lanes rewrite it two stages on) -- instruction i serves
    // the wave's records 8i .. 8i+7, eight lanes per record, each record's whole 128-byte run
    // in one instruction.  Per-lane 16-byte stores wrote 64 records' lines in eight pieces
    // each, and the pieces the L2 wrote back separately doubled the fetch's HBM writes
    // (pmc_st_r05z.json: 2.03x the algorithmic write bytes; seal 1.42x).
    auto store_stage = [&](uint32_t t) {
        const uint32_t kk = lane & 7u;
        const uint32_t wrow = rl - lane;
        const uint8_t* slab = L.ptb + (t & 1u) * kBuf;
#pragma unroll 1
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t o = 8u * i + (lane >> 3);
            if (t < L.ots_s[wrow + o]) {
                const uint32_t sw = ((o >> 1) & 7u) ^ ((o & 1u) << 2);
                const uint4 v = *reinterpret_cast<const uint4*>(slab + (wrow + o) * kRun + 16u * kk);
                uint8_t* d = reinterpret_cast<uint8_t*>(L.odst_s[wrow + o]) + (uint64_t)kRun * t + 16u * (kk ^ sw);
                *reinterpret_cast<uint4*>(d) = v;
            }
        }
    };
    if (Ts > 0) load_run(0);
    for (uint32_t s = 0; s < Tmax; ++s) {
        if (kLines && s > 0) store_stage(s - 1);
        if (s < Ts) {
            uint32_t x[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) x[i] = pf[i];
            if (s + 1 < Ts) load_run(s + 1);
            uint8_t* const pt = L.ptb + (s & 1u) * kBuf + rl * kRun;
            if (!OPEN) put_run(pt, x);  // plaintext for the hash lane
            if (KIND == DK_AEADH && OPEN) aead_absorb(A, x, 8);
            {
                uint32_t ka[16], kb[16];
                chacha_block2(R, c0 + 2u * s, c0 + 2u * s + 1u, ka, kb);
#pragma unroll
                for (int i = 0; i < 16; ++i) { x[i] ^= ka[i]; x[16 + i] ^= kb[i]; }
            }
            if (KIND == DK_AEADH && !OPEN) aead_absorb(A, x, 8);
            if (OPEN) put_run(pt, x);
            if (!kLines) {
                uint4* o = reinterpret_cast<uint4*>(dst + (uint64_t)kRun * s);
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = make_uint4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
            }
        }
        ENET_DX_BARRIER();  // stage s plaintext is in ptb[s & 1]
    }
    if (kLines && Tmax > 0) store_stage(Tmax - 1);

    // ---- ragged end
    const uint32_t tin = (OPEN && KIND == DK_FRAME) ? r + 32u : r;  // body-tail bytes read now
    uint32_t w[48];
#pragma unroll
    for (int i = 0; i < 48; ++i) w[i] = 0u;
    if (valid && tin) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (tin > 64u * k) {
                const uint32_t nk = min(64u, tin - 64u * k);
                load_block(src + tb + 64u * k, nk, w + 16 * k, off0 + tb + 64u * k + nk >= 16u);
            }
        }
    }
    uint32_t ks[48];
#pragma unroll
    for (int i = 32; i < 48; ++i) ks[i] = 0u;  // the third block is only made when a body needs it
    if (valid && (tin || (!OPEN && KIND == DK_FRAME))) {
        chacha_block2(R, c0 + 2u * Ts, c0 + 2u * Ts + 1u, ks, ks + 16);
        if (KIND == DK_FRAME && r + 32u > 128u) chacha_block(R, c0 + 2u * Ts + 2u, ks + 32);
    }
    if (!OPEN) {
        if (valid) {
            // T1: the message tail to the hash lane
            L.slot.slot_put(w, 8);
            if (KIND != DK_FRAME && r) {
#pragma unroll
                for (int j = 0; j < 32; ++j) w[j] ^= ks[j];
                store_block(dst + tb, min(r, 64u), w);
                if (r > 64u) store_block(dst + tb + 64, r - 64u, w + 16);
                if (KIND == DK_AEADH) {
                    keep_le<32>(w, r);
                    aead_absorb(A, w, (r + 15u) >> 4);
                }
            }
            if (KIND == DK_AEADH) {
                uint32_t tag[4];
                aead_tag(A, g.Lm, tag);
                *reinterpret_cast<uint4*>(p.tags + 16ull * rec) = make_uint4(tag[0], tag[1], tag[2], tag[3]);
            }
        }
        ENET_DX_BARRIER();  // T1
        ENET_DX_BARRIER();  // T2: frames -- the MAC sits behind the message tail in the slot
        if (KIND == DK_FRAME && valid) {
            // T3: body tail = message tail || MAC, one run of body bytes
            const uint32_t t = r + 32u;
#pragma unroll
            for (int c = 0; c < 10; ++c) {
                const uint4 v = L.slot.slot_chunk(c);
                w[4 * c] = v.x ^ ks[4 * c]; w[4 * c + 1] = v.y ^ ks[4 * c + 1];
                w[4 * c + 2] = v.z ^ ks[4 * c + 2]; w[4 * c + 3] = v.w ^ ks[4 * c + 3];
            }
            store_block(dst + tb, min(t, 64u), w);
            if (t > 64u) store_block(dst + tb + 64, min(t - 64u, 64u), w + 16);
            if (t > 128u) store_block(dst + tb + 128, t - 128u, w + 32);
            if (H) {  // nonce(12) || BE32(|body|) (SessionManager.cpp:376-385)
                *reinterpret_cast<uint4*>(p.out + g.ob) =
                    make_uint4(nw[0], nw[1], nw[2], bswap32((uint32_t)(g.Lm + 32u)));
            }
        }
    } else {
        if (valid) {
            uint32_t aok = 1;
            if (KIND == DK_AEADH) {  // Poly1305 over the ciphertext (zero beyond r), then lengths
                aead_absorb(A, w, (r + 15u) >> 4);
                uint32_t tag[4];
                aead_tag(A, g.Lm, tag);
                aok = tag_diff(tag, p.tags_in + 16ull * rec) == 0u;
            }
            if (tin) {
#pragma unroll
                for (int j = 0; j < 40; ++j) w[j] ^= ks[j];
            }
            if (r) {
                store_block(dst + tb, min(r, 64u), w);
                if (r > 64u) store_block(dst + tb + 64, r - 64u, w + 16);
            }
            L.slot.slot_put(w, KIND == DK_FRAME ? 10 : 8);
            if (KIND == DK_AEADH) *L.slot.slot_byte(159) = (uint8_t)aok;
        }
        // the plaintext stores are complete before a hash lane may zero them on failure
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        ENET_DX_BARRIER();  // T1
    }
}

// ================================================================== hash lane
// frames / AEAD: HMAC-SHA256 (HmacSha256.cpp:11-39) with the 32-byte record key;
// chunks: SHA-256 (Sha256::digest, Sha256.cpp:66-132)
template <int KIND, bool OPEN, int RPW>
__device__ __forceinline__ void duplex_hash_lane(const DuplexParams& p, const DuplexGeom& g, const DuplexLane& L) {
    constexpr uint32_t kBuf = RPW * kRun;
    const uint32_t H = L.H, rl = L.rl, Tmax = L.Tmax, rec = g.rec, Ts = g.Ts(), r = g.r(), msw = L.slot.msw;
    const bool live = g.live, valid = g.valid;

    if (p.prio == 1) __builtin_amdgcn_s_setprio(2);
    uint32_t kb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) kb[i] = bswap32(L.kw[i]);
    uint32_t st[8], x[16];
    // session-keyed frames: the session's midstates replace the ipad / opad compressions
    const uint32_t* ms = (KIND == DK_FRAME && p.mid && live) ? p.mid + 16ull * L.sid : nullptr;
    if (KIND == DK_CHUNK) {
        sha256_init(st);
    } else if (ms) {
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = ms[i];
    } else {
        hmac_key_state(st, kb, kHmacIpad);
    }
    for (uint32_t s = 0; s < Tmax; ++s) {
        ENET_DX_BARRIER();
        if (s < Ts) {
            const uint8_t* pt = L.ptb + (s & 1u) * kBuf + rl * kRun;
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint4 v = *reinterpret_cast<const uint4*>(pt + 16u * ((4 * hb + k) ^ msw));
                    x[4 * k] = bswap32(v.x); x[4 * k + 1] = bswap32(v.y);
                    x[4 * k + 2] = bswap32(v.z); x[4 * k + 3] = bswap32(v.w);
                }
                sha256_compress(st, x);
            }
        }
    }
    ENET_DX_BARRIER();  // T1: the ragged end is in the slot
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // digest as LE words of its bytes
    if (valid) {
        // message tail, 0x80, zeros, BE64 bit length of [ipad ||] m
        const uint64_t bits = ((KIND == DK_CHUNK ? 0ull : 64ull) + g.Lm) * 8ull;
        uint32_t tail[32];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if ((uint32_t)k < sha256_tail_blocks(r)) {
#pragma unroll
                for (int c = 4 * k; c < 4 * k + 4 && c < 8; ++c) {
                    const uint4 v = L.slot.slot_chunk(c);
                    tail[4 * c] = v.x; tail[4 * c + 1] = v.y; tail[4 * c + 2] = v.z; tail[4 * c + 3] = v.w;
                }
                sha256_tail_block(k, tail, r, bits, x);
                sha256_compress(st, x);
            }
        }
        if (KIND != DK_CHUNK) {
            uint32_t inner[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) inner[i] = st[i];
            if (ms) {
#pragma unroll
                for (int i = 0; i < 8; ++i) st[i] = ms[8 + i];
            } else {
                hmac_key_state(st, kb, kHmacOpad);
            }
            hmac_outer_finish(st, inner);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = bswap32(st[i]);
    }
    if (!OPEN) {
        if (KIND == DK_FRAME) {
            if (valid) {  // the MAC follows the message tail in the slot
                for (uint32_t i = 0; i < 32u; ++i) *L.slot.slot_byte(r + i) = (uint8_t)(d[i >> 2] >> (8u * (i & 3u)));
            }
            finish_record<false>(p, g, d, nullptr, nullptr, 0u);
        } else {
            finish_record<false>(p, g, d, (KIND == DK_CHUNK ? p.digests : p.macs) + 32ull * rec, nullptr, 0u);
        }
        ENET_DX_BARRIER();  // T2
    } else if (KIND == DK_FRAME) {
        uint32_t diff = 0u;
        if (valid) {  // HmacSha256::verify (HmacSha256.cpp:41-54)
            uint32_t e[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint32_t v = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) v |= (uint32_t)*L.slot.slot_byte(r + 4u * j + b) << (8 * b);
                e[j] = v;
                diff |= v ^ d[j];
            }
            uint8_t* mp = p.macs + 32ull * rec;
            reinterpret_cast<uint4*>(mp)[0] = make_uint4(e[0], e[1], e[2], e[3]);
            reinterpret_cast<uint4*>(mp)[1] = make_uint4(e[4], e[5], e[6], e[7]);
            if (H) {  // the length field must give the body (SessionManager.cpp:770-796)
                const uint32_t be = bswap32(ld32(p.in + g.ib + 12));
                if ((uint64_t)be != g.Li - H) diff = 1;
            }
        }
        finish_record<true>(p, g, d, nullptr, nullptr, diff);
    } else {
        const bool tag_bad = KIND == DK_AEADH && valid && *L.slot.slot_byte(159) == 0;
        finish_record<true>(p, g, d, nullptr, (KIND == DK_CHUNK ? p.expect : p.macs_in) + 32ull * rec, tag_bad);
    }
}

// RPW records per workgroup: RPW / 64 cipher waves + RPW / 64 hash waves.
template <int KIND, bool OPEN, int RPW>
__device__ __forceinline__ void duplex_body(const DuplexParams& p) {
    constexpr uint32_t kW = RPW / 64;          // waves per role
    constexpr uint32_t kBuf = RPW * kRun;      // one stage of the workgroup (32 KB at 256 records)
    __shared__ __attribute__((aligned(16))) uint8_t ptb[2 * kBuf];  // stage slabs
    __shared__ __attribute__((aligned(16))) uint8_t text[RPW * 32];  // tail slot bytes 128..159
    __shared__ uint32_t tmax_s;
    constexpr bool kLines = OPEN && KIND == DK_CHUNK;  // see duplex_cipher_lane
    __shared__ uint64_t odst_s[kLines ? RPW : 1];
    __shared__ uint32_t ots_s[kLines ? RPW : 1];

    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    const bool cipher = wave < kW;
    DuplexLane L;
    L.rl = 64u * (wave % kW) + lane;
    L.H = KIND == DK_FRAME ? p.hdr : 0u;

    // ---- geometry (both lanes of a record compute it)
    DuplexGeom g = duplex_geom(p, blockIdx.x * RPW + L.rl);
    uint64_t Lm = g.Li;  // message bytes
    bool fits;
    if (KIND == DK_FRAME && !OPEN) {
        fits = g.Lo == g.Li + 32u + L.H;
    } else if (KIND == DK_FRAME) {  // frames shorter than [hdr] + MAC fail (Message.cpp:315)
        const bool whole = g.Li >= 32ull + L.H;
        Lm = whole ? g.Li - 32u - L.H : 0;
        fits = whole && g.Lo == Lm;
    } else {
        fits = g.Lo == g.Li;
    }
    // session-keyed frames: an index outside the table fails closed -- the record is processed
    // as invalid (seal: the whole output slot zeroed, no byte encrypted under another session's
    // key; open: ok = 0, plaintext zeroed), and no key or midstate past the table is read
    const uint32_t sraw = (p.session && g.live) ? p.session[g.rec] : 0u;
    const bool sbad = p.session && sraw >= p.n_sessions;
    L.sid = sbad ? 0u : sraw;
    duplex_geom_message(g, Lm, fits && !sbad);

    if (threadIdx.x == 0) tmax_s = 0;
    __syncthreads();
    if (cipher && g.Ts()) atomicMax(&tmax_s, g.Ts());
    __syncthreads();
    L.Tmax = __builtin_amdgcn_readfirstlane(tmax_s);
    // Length-graded issue priority: a workgroup lasts as long as its longest record's serial
    // SHA-256 chain (one lane; 64 KiB = 1 027 compressions, ~2.8 ms), so with mixed lengths (C5)
    // the kernel's tail is that chain -- and when other workgroups (or, with overlapped steps, the
    // other direction's kernel) share its SIMDs, the chain only gets its share of issue slots.
    // Both waves of a long workgroup are on that chain (they meet at every stage barrier), so
    // they win arbitration over shorter workgroups'.
    if (p.prio == 0) {
        if (L.Tmax >= 256) __builtin_amdgcn_s_setprio(3);
        else if (L.Tmax >= 64) __builtin_amdgcn_s_setprio(2);
        else if (L.Tmax >= 16) __builtin_amdgcn_s_setprio(1);
    }

    L.ptb = ptb;
    L.odst_s = odst_s;
    L.ots_s = ots_s;
    L.slot.msw = ((lane >> 1) & 7u) ^ ((lane & 1u) << 2);
    L.slot.xsw = ((lane >> 2) ^ (lane >> 3)) & 1u;
    L.slot.trow = ptb + (L.Tmax & 1u) * kBuf + L.rl * kRun;  // tail slot bytes 0..127
    L.slot.xrow = text + L.rl * 32u;                          // tail slot bytes 128..159
    {
        const uint8_t* kp = p.session ? p.keys + 32ull * L.sid : p.keys + (size_t)p.key_stride * g.rec;
#pragma unroll
        for (int i = 0; i < 8; ++i) L.kw[i] = g.live ? reinterpret_cast<const uint32_t*>(kp)[i] : 0u;
    }

    if (cipher) duplex_cipher_lane<KIND, OPEN, RPW>(p, g, L);
    else duplex_hash_lane<KIND, OPEN, RPW>(p, g, L);
}

// Frames and chunks fit 128 VGPRs, so two workgroups share a CU (LDS 72 KB each) when the batch
// has more than 256 workgroups (C3: 1 M frames, 358 -> 388 GiB/s).  The AEAD + HMAC body would
// spill at 128, so it keeps one workgroup per CU.
template <int KIND, bool OPEN, int RPW>
__global__ __launch_bounds__(2 * RPW) __attribute__((amdgpu_waves_per_eu(4))) void duplex_kernel(DuplexParams p) {
    duplex_body<KIND, OPEN, RPW>(p);
}
template <int KIND, bool OPEN, int RPW>
__global__ __launch_bounds__(2 * RPW) void duplex_kernel_wide(DuplexParams p) {
    duplex_body<KIND, OPEN, RPW>(p);
}

template <int RPW>
hipError_t launch_duplex_rpw(int kind, bool open, const DuplexParams& p, hipStream_t s) {
    const uint32_t blocks = (p.n + RPW - 1) / RPW;
    const dim3 g(blocks), b(2 * RPW);
    switch (kind * 2 + (open ? 1 : 0)) {
        case DK_FRAME * 2: hipLaunchKernelGGL((duplex_kernel<DK_FRAME, false, RPW>), g, b, 0, s, p); break;
        case DK_FRAME * 2 + 1: hipLaunchKernelGGL((duplex_kernel<DK_FRAME, true, RPW>), g, b, 0, s, p); break;
        case DK_CHUNK * 2: hipLaunchKernelGGL((duplex_kernel<DK_CHUNK, false, RPW>), g, b, 0, s, p); break;
        case DK_CHUNK * 2 + 1: hipLaunchKernelGGL((duplex_kernel<DK_CHUNK, true, RPW>), g, b, 0, s, p); break;
        case DK_AEADH * 2: hipLaunchKernelGGL((duplex_kernel_wide<DK_AEADH, false, RPW>), g, b, 0, s, p); break;
        case DK_AEADH * 2 + 1: hipLaunchKernelGGL((duplex_kernel_wide<DK_AEADH, true, RPW>), g, b, 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_duplex(int kind, bool open, const DuplexParams& p, hipStream_t s) {
    if (p.n == 0) return hipSuccess;
    // long records (a 64 KiB record's serial hash chain is the whole kernel time): chunks and
    // AEAD + HMAC split each record over four waves (duplex_split.hip) -- for uniform batches
    // and batches the caller ordered (length-sorted, like C5).  The split kernel holds 2
    // workgroups per CU (80 KiB LDS) against 6 here, so an UNSORTED mixed batch, where every
    // workgroup holds some long record, runs two rounds of chains there: 45 vs 69 GiB/s at C5.
    if (kind == DK_CHUNK || kind == DK_AEADH) {
        const int m = duplex_split_mode();
        if (m == 1 || (m == -1 && p.max_len >= 16384u && (p.uniform || p.order != nullptr))) {
            DuplexParams q = p;
            return launch_duplex_split(kind, open, q, s);
        }
    }
    // A/B knobs, compiled into kernel objects built with -DENET_TOOLS_BUILD only (build.py --tools
    // --probes)
#ifdef ENET_TOOLS_BUILD
    static const int prio_env = [] {
        const char* e = std::getenv("ENET_DUPLEX_PRIO");
        return e ? (int)std::strtol(e, nullptr, 10) : 0;
    }();
    static const int rpw_env = [] {
        const char* e = std::getenv("ENET_DUPLEX_RPW");
        return e ? (int)std::strtol(e, nullptr, 10) : 0;
    }();
#else
    constexpr int prio_env = 0, rpw_env = 0;
#endif
    DuplexParams q = p;
    q.prio = prio_env;
    // Mixed lengths: 64-record workgroups, so the few long records (a workgroup lasts as long as
    // its longest record's serial hash) occupy few SIMDs and the rest of the chip keeps pulling
    // short workgroups (C5 device-resident: 88 -> 138 GiB/s).  Uniform batches: 256-record
    // workgroups once there are >= 128 of them (C4 store 64 KiB: 230 vs 217 GiB/s), else 64.
    const bool small = rpw_env ? rpw_env == 64 : (!p.uniform || p.n < 128u * 256u);
    return small ? launch_duplex_rpw<64>(kind, open, q, s) : launch_duplex_rpw<256>(kind, open, q, s);
}

}  // namespace enet
