// chunk_frames.hip -- a chunk's transfer frame in one HBM pass (gfx950).
//
// The reference moves a stored chunk between two nodes as a `Chunk` message inside a session
// frame (Node::dispatch_upload, Node.cpp:1254-1297; encode, Message.cpp:204-246; encode_signed,
// Message.cpp:305-311; SessionManager::send, SessionManager.cpp:362-387):
//   m     = version || 0x03 || BE32(ttl) || BE32(|data|) || chunk_id(32) || data       (42 + D)
//   frame = nonce(12) || BE32(|m| + 32) || ChaCha20_{Ks,nonce,0}(m || HMAC_Ks(m))
//   data  = ChaCha20_{Kc,Nc,LE32(chunk_id[0..3])}(plaintext)       (what the node has stored)
// and the receiver undoes both layers and checks both hashes (receive_loop,
// SessionManager.cpp:760-822; decode_signed, Message.cpp:313-328; decode, Message.cpp:144-159;
// receive_chunk, Node.cpp:1615-1677): two keystreams and two hash chains over the same bytes.
//
// open  three lanes per record, 64 records per 192-thread workgroup: wave 0 "cipher" (both
//       keystreams), wave 1 "mac" (HMAC-SHA256 over m), wave 2 "sha" (SHA-256 over the
//       plaintext).  Stages are 128 message bytes, as in duplex.hip.  The header is always 42
//       bytes, so the chunk layer trails the message by a constant: stage s needs the last 42
//       bytes of chunk keystream block 2s-1 (carried from the stage before), all of block 2s and
//       the first 22 bytes of block 2s+1 -- two new blocks per stage, an 11-word carry and a
//       constant 16-bit funnel shift (v_alignbyte) over compile-time register indices.  The cipher lane hands every stage to the mac lane (message bytes,
//       slab `msg`) and to the sha lane (plaintext at its MESSAGE position, slab `pt`) through
//       double-buffered LDS, one barrier per stage; the sha lane keeps the stage's last 22 bytes
//       in registers across the barrier and realigns by the same constant.  The ragged end goes
//       through 160-byte (msg, with the MAC) and 128-byte (pt) tail slots.  The mac lane holds
//       the verdict: it writes status / ttl and zeroes what a failed record stored.
// seal  the frame seal of duplex.hip with a gather: two lanes per record (cipher, mac), stage
//       bytes from data - 42 + 128 s, the first 42 bytes of stage 0 being the synthesized header.
// No load touches a byte outside [in_off[i], in_off[i+1]), no store one outside the record's
// output ranges: stage 0 and the ragged end start at the record's first data byte.
#include "duplex_common.hpp"

namespace enet {

namespace {

constexpr uint32_t kRun = kDxRun;
constexpr uint32_t kRecs = 64;                     // records per workgroup: one wave per role
constexpr uint32_t kBuf = kRecs * kRun;            // one stage of the workgroup in one slab
constexpr uint32_t kHdr = kChunkFrameHeader;       // 42
constexpr uint32_t kWire = 16;                     // nonce(12) || BE32(|body|)

// bytes [2 + 4 j, 6 + 4 j) of the LE byte string in w: the 16-bit half of every constant shift
__device__ __forceinline__ uint32_t half_up(const uint32_t* w, int j) {
    return __builtin_amdgcn_alignbyte(w[j + 1], w[j], 2);
}

// What the lanes of a record share beside its geometry.
struct CfLane {
    uint32_t sid, rl, Tmax;  // session index; the record's row; stages of the longest record
    uint32_t msw, xsw;       // 16-byte chunk swizzles of a 128-byte row / the 32-byte extension
    uint32_t kw[8];          // session key, LE words
    uint8_t *msg, *pt;       // stage slabs [2][kRecs][128]: message bytes / plaintext
    uint8_t* text;           // [kRecs][32]: msg tail slot bytes 128..159
    uint32_t *hs_s, *ttl_s, *sha_s;  // per record: header status, ttl, SHA-256 mismatch
    bool chunked;            // open: the frame is processed and its message holds a header
    __device__ __forceinline__ uint8_t* row(uint8_t* slab, uint32_t s) const {
        return slab + (s & 1u) * kBuf + rl * kRun;
    }
    __device__ __forceinline__ void put_row(uint8_t* r, const uint32_t* v) const {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            *reinterpret_cast<uint4*>(r + 16u * (k ^ msw)) = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    }
    __device__ __forceinline__ void get_row(const uint8_t* r, uint32_t* v, int c0, int c1) const {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            if (k < c0 || k >= c1) continue;
            const uint4 q = *reinterpret_cast<const uint4*>(r + 16u * (k ^ msw));
            v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
        }
    }
    // the msg tail slot: bytes 0..127 in the row the last stage left free, 128..159 in text
    __device__ __forceinline__ uint8_t* xchunk(int c) const { return text + rl * 32u + 16u * (c ^ xsw); }
    __device__ __forceinline__ uint8_t* slot_byte(uint32_t i) const {
        return i < kRun ? row(msg, Tmax) + 16u * ((i >> 4) ^ msw) + (i & 15u)
                        : text + rl * 32u + 16u * (((i - kRun) >> 4) ^ xsw) + (i & 15u);
    }
};

// 128 message bytes of stage s (v, at message offset 128 s) to base + 128 s - 42, base = the
// address of message byte 42; stage 0 starts at message byte 42 (2 bytes, 5 x 16, 4)
__device__ __forceinline__ void store_stage(uint8_t* base, uint32_t s, const uint32_t* v) {
    if (s == 0) {
        base[0] = (uint8_t)(v[10] >> 16);
        base[1] = (uint8_t)(v[10] >> 24);
#pragma unroll
        for (int i = 0; i < 5; ++i)
            *reinterpret_cast<uint4*>(base + 2 + 16 * i) =
                make_uint4(v[11 + 4 * i], v[12 + 4 * i], v[13 + 4 * i], v[14 + 4 * i]);
        *reinterpret_cast<uint32_t*>(base + 82) = v[31];
    } else {
        uint4* o = reinterpret_cast<uint4*>(base + (uint64_t)kRun * s - kHdr);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    }
}

// the ragged end: message bytes [lo, r) of v (at message offset tb; lo = 42 when tb == 0, else
// 0) to base + tb + lo - 42
__device__ __forceinline__ void store_tail(uint8_t* base, uint64_t tb, uint32_t r, const uint32_t* v) {
    const bool first = tb == 0;
    uint32_t t[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) t[j] = first ? (j < 22 ? half_up(v, 10 + j) : 0u) : v[j];
    const uint32_t n = first ? r - kHdr : r;
    uint8_t* d = first ? base : base + tb - kHdr;
    if (n) store_block(d, min(n, 64u), t);
    if (n > 64u) store_block(d + 64, n - 64u, t + 16);
}

// decode's checks on the 42 header bytes (m = the message's first 11 LE words): 2 HEADER, 3
// CHUNK_ID, 0 fine (Message.cpp:144-159, 340-352); ttl = the header's BE32 seconds
__device__ __forceinline__ uint32_t check_header(const uint32_t* m, uint64_t Lm, const uint8_t* id, uint32_t& ttl) {
    const uint32_t ver = m[0] & 0xffu, type = (m[0] >> 8) & 0xffu;
    ttl = bswap32(half_up(m, 0));
    const uint32_t len = bswap32(half_up(m, 1));
    uint32_t idd = 0u;
#pragma unroll
    for (int j = 0; j < 8; ++j) idd |= half_up(m, 2 + j) ^ ld32(id + 4 * j);
    if (ver < 1u || ver > 4u || type != 3u || (uint64_t)len != Lm - kHdr) return 2u;
    return idd ? 3u : 0u;
}

// ================================================================== open: cipher lane
// the header checks of a processed frame, posted for the mac lane (read after T2)
__device__ __forceinline__ void post_header(const ChunkFrameParams& p, const DuplexGeom& g, const CfLane& L,
                                            const uint32_t* m) {
    uint32_t ttl;
    L.hs_s[L.rl] = check_header(m, g.Lm, p.chunk_ids + 32ull * g.rec, ttl);
    L.ttl_s[L.rl] = ttl;
}

// PF: the next stage is prefetched into registers across the barrier (see chunk_frames_kernel)
template <bool PF>
__device__ __forceinline__ void cf_open_cipher(const ChunkFrameParams& p, const DuplexGeom& g, const CfLane& L) {
    const uint32_t rec = g.rec, Ts = g.Ts(), r = g.r(), Tmax = L.Tmax;
    const uint64_t tb = g.tb();
    const bool valid = g.valid, chunked = L.chunked;
    const uint8_t* src = p.d.in + g.ib + kWire;
    uint8_t* dpt = p.d.out + g.ob;
    // the stored ciphertext goes to the same offsets of another arena: one per-lane pointer serves both
    const bool keep_ct = p.data_out != nullptr;
    const int64_t ct_delta = keep_ct ? (int64_t)(reinterpret_cast<uintptr_t>(p.data_out) - reinterpret_cast<uintptr_t>(p.d.out)) : 0;

    uint32_t nw[3], ck[8], cn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // nonce = the frame's first 12 bytes (SessionManager.cpp:815-822)
        nw[i] = valid ? ld32(p.d.in + g.ib + 4 * i) : 0u;
        cn[i] = chunked ? ld32(p.chunk_nonces + 12ull * rec + 4 * i) : 0u;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) ck[i] = chunked ? ld32(p.chunk_keys + 32ull * rec + 4 * i) : 0u;
    // ChachaRecord's per-record column precomputation (12 words) is rebuilt for every pair of
    // blocks instead of kept: two of them do not fit beside a stage at three waves per SIMD.
    // The empty asm makes the nonce words opaque, so the rebuild is not hoisted back out of the
    // stage loop.
    auto blocks2 = [](const uint32_t* k, uint32_t* n, uint32_t ca, uint32_t cb, uint32_t* a, uint32_t* b) {
#pragma unroll
        for (int i = 0; i < 3; ++i) asm volatile("" : "+v"(n[i]));
        ChachaRecord R;
        chacha_record_init(R, k, n);
        chacha_block2(R, ca, cb, a, b);
    };
    // derive_counter (CryptoManager.cpp:8-13): LE32(chunk_id[0..3]), u32 wrap
    const uint32_t c0 = chunked ? ld32(p.chunk_ids + 32ull * rec) : 0u;

    // K = the last 44 bytes of chunk keystream block 2s-1 (the carry), then blocks 2s and 2s+1:
    // message byte j of stage s takes K byte 2 + j
    uint32_t K[43];
#pragma unroll
    for (int i = 0; i < 11; ++i) K[i] = 0u;
    // the header's verdict and ttl wait in LDS for the mac lane, not in registers
    L.hs_s[L.rl] = 2u;
    L.ttl_s[L.rl] = 0u;
    auto load_run = [&](uint32_t s, uint32_t* d) {
        const uint4* q = reinterpret_cast<const uint4*>(src + (uint64_t)kRun * s);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint4 v = q[i];
            d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
        }
    };
    // !PF: a stage's loads are issued first and land while its session keystream, which does
    // not depend on them, is computed; other waves of the SIMD cover the rest of the latency
    uint32_t pf[PF ? 32 : 1];
    if (PF && Ts > 0) load_run(0, pf);
    for (uint32_t s = 0; s < Tmax; ++s) {
        if (s < Ts) {
            uint32_t x[32];
            if (PF) {
#pragma unroll
                for (int i = 0; i < 32; ++i) x[i] = pf[PF ? i : 0];
                if (s + 1 < Ts) load_run(s + 1, pf);
            } else {
                load_run(s, x);
            }
            {
                uint32_t ka[16], kb[16];
                blocks2(L.kw, nw, 2u * s, 2u * s + 1u, ka, kb);
#pragma unroll
                for (int i = 0; i < 16; ++i) { x[i] ^= ka[i]; x[16 + i] ^= kb[i]; }
            }
            L.put_row(L.row(L.msg, s), x);  // message bytes for the mac lane
            if (s == 0 && chunked) post_header(p, g, L, x);
            if (chunked) {
                if (keep_ct) store_stage(dpt + ct_delta, s, x);  // the chunk ciphertext the node stores
                blocks2(ck, cn, c0 + 2u * s, c0 + 2u * s + 1u, K + 11, K + 27);
#pragma unroll
                for (int i = 0; i < 32; ++i) x[i] ^= half_up(K, i);
#pragma unroll
                for (int i = 0; i < 11; ++i) K[i] = K[32 + i];
                L.put_row(L.row(L.pt, s), x);  // plaintext (at its message position) for the sha lane
                store_stage(dpt, s, x);
            }
        }
        ENET_DX_BARRIER();  // stage s is in msg / pt [s & 1]
    }

    // ---- ragged end: r message bytes and the MAC
    const uint32_t tin = r + 32u;
    uint32_t w[48];
#pragma unroll
    for (int i = 0; i < 48; ++i) w[i] = 0u;
    if (valid) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (tin > 64u * k) {
                const uint32_t nk = min(64u, tin - 64u * k);
                load_block(src + tb + 64u * k, nk, w + 16 * k, true);  // 16 header bytes lie in front
            }
        }
        {
            uint32_t ka[16], kb[16];
            blocks2(L.kw, nw, 2u * Ts, 2u * Ts + 1u, ka, kb);
#pragma unroll
            for (int i = 0; i < 16; ++i) { w[i] ^= ka[i]; w[16 + i] ^= kb[i]; }
        }
        if (tin > 128u) {
            uint32_t kc[16];
            ChachaRecord R;
            chacha_record_init(R, L.kw, nw);
            chacha_block(R, 2u * Ts + 2u, kc);
#pragma unroll
            for (int i = 0; i < 8; ++i) w[32 + i] ^= kc[i];
        }
        // message tail || MAC to the mac lane
        L.put_row(L.row(L.msg, Tmax), w);
#pragma unroll
        for (int c = 0; c < 2; ++c)
            *reinterpret_cast<uint4*>(L.xchunk(c)) = make_uint4(w[32 + 4 * c], w[33 + 4 * c], w[34 + 4 * c], w[35 + 4 * c]);
        if (Ts == 0 && chunked) post_header(p, g, L, w);
        if (chunked && (Ts > 0 ? r > 0u : r > kHdr)) {
            if (keep_ct) store_tail(dpt + ct_delta, tb, r, w);
            blocks2(ck, cn, c0 + 2u * Ts, c0 + 2u * Ts + 1u, K + 11, K + 27);
#pragma unroll
            for (int i = 0; i < 32; ++i) w[i] ^= half_up(K, i);
            L.put_row(L.row(L.pt, Tmax), w);
            store_tail(dpt, tb, r, w);
        }
    }
    // the plaintext and ciphertext stores are complete before the mac lane may zero them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ENET_DX_BARRIER();  // T1
    ENET_DX_BARRIER();  // T2
}

// ================================================================== open: sha lane
// SHA-256(plaintext) against the manifest's chunk_hash (receive_chunk, Node.cpp:1644-1655).  The
// plaintext arrives at its message position: data block k is message bytes [64 k + 42, 64 k +
// 106), so stage s completes blocks 2s-1 (22 carried bytes + 42) and 2s.
__device__ __forceinline__ void cf_sha_lane(const ChunkFrameParams& p, const DuplexGeom& g, const CfLane& L) {
    const uint32_t Ts = g.Ts(), r = g.r(), Tmax = L.Tmax;
    const bool chunked = L.chunked;
    uint32_t st[8], x[16];
    sha256_init(st);
    // W = the stage before's words 26..31 (its last 24 bytes), then this stage's 32 words, then 0
    uint32_t W[39];
#pragma unroll
    for (int i = 0; i < 39; ++i) W[i] = 0u;
    for (uint32_t s = 0; s < Tmax; ++s) {
        ENET_DX_BARRIER();
        if (s < Ts && chunked) {
            L.get_row(L.row(L.pt, s), W + 6, 0, 8);
            if (s > 0) {
#pragma unroll
                for (int j = 0; j < 16; ++j) x[j] = bswap32(half_up(W, j));
                sha256_compress(st, x);
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) x[j] = bswap32(half_up(W, 16 + j));
            sha256_compress(st, x);
#pragma unroll
            for (int j = 0; j < 6; ++j) W[j] = W[32 + j];
        }
    }
    ENET_DX_BARRIER();  // T1: the ragged end is in the slot
    uint32_t diff = 0u;
    if (chunked) {
        if (Ts > 0 ? r > 0u : r > kHdr) L.get_row(L.row(L.pt, Tmax), W + 6, 0, 8);
        // what is left of the plaintext: 22 carried bytes + r (after whole stages), or r - 42
        const uint32_t n = Ts > 0 ? 22u + r : r - kHdr;
        if (Ts == 0) {  // no carried bytes: the data starts at message byte 42, word 16 of W
#pragma unroll
            for (int j = 0; j < 39; ++j) W[j] = j + 16 < 39 ? W[j + 16] : 0u;
        }
        const uint64_t bits = (g.Lm - kHdr) * 8ull;
        const uint32_t nb = sha256_tail_blocks(n);  // n <= 149: 1..3 blocks
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if ((uint32_t)k < nb) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const uint32_t b = 64u * k + 4u * i;
                    const uint32_t v = 16 * k + i < 38 ? bswap32(half_up(W, 16 * k + i)) : 0u;
                    const uint32_t m = b + 4u <= n ? 0xffffffffu : (b >= n ? 0u : 0xffffffffu << (8u * (4u - (n - b))));
                    x[i] = (v & m) | ((n >> 2) == (b >> 2) ? 0x80000000u >> (8u * (n & 3u)) : 0u);
                }
                if ((uint32_t)k == nb - 1u) {
                    x[14] = (uint32_t)(bits >> 32);
                    x[15] = (uint32_t)bits;
                }
                sha256_compress(st, x);
            }
        }
        const uint8_t* e = p.chunk_hashes + 32ull * g.rec;
#pragma unroll
        for (int j = 0; j < 8; ++j) diff |= bswap32(st[j]) ^ ld32(e + 4 * j);
    }
    L.sha_s[L.rl] = diff;
    ENET_DX_BARRIER();  // T2
}

// ================================================================== mac lane (both directions)
// HMAC-SHA256_Ks(m) (HmacSha256.cpp:11-39).  seal: the MAC goes behind the message tail in the
// slot for the cipher lane to encrypt.  open: compare with the decrypted MAC (HmacSha256::verify,
// HmacSha256.cpp:41-54), gather the other lanes' findings, write status / ttl, zero a failed record.
template <bool OPEN>
__device__ __forceinline__ void cf_mac_lane(const ChunkFrameParams& p, const DuplexGeom& g, const CfLane& L) {
    const uint32_t rec = g.rec, Ts = g.Ts(), r = g.r(), Tmax = L.Tmax;
    const bool live = g.live, valid = g.valid;
    uint32_t kb[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) kb[i] = bswap32(L.kw[i]);
    uint32_t st[8], x[16];
    // session-keyed frames: the session's midstates replace the ipad / opad compressions
    const uint32_t* ms = (p.d.mid && live) ? p.d.mid + 16ull * L.sid : nullptr;
    if (ms) {
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = ms[i];
    } else {
        hmac_key_state(st, kb, kHmacIpad);
    }
    for (uint32_t s = 0; s < Tmax; ++s) {
        ENET_DX_BARRIER();
        if (s < Ts) {
            const uint8_t* row = L.row(L.msg, s);
#pragma unroll
            for (int hb = 0; hb < 2; ++hb) {
                uint32_t v[32];
                L.get_row(row, v, 4 * hb, 4 * hb + 4);
#pragma unroll
                for (int j = 0; j < 16; ++j) x[j] = bswap32(v[16 * hb + j]);
                sha256_compress(st, x);
            }
        }
    }
    ENET_DX_BARRIER();  // T1: the ragged end is in the slot
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // MAC as LE words of its bytes
    if (valid) {
        const uint64_t bits = (64ull + g.Lm) * 8ull;
        uint32_t tail[32];
        const uint8_t* trow = L.row(L.msg, Tmax);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if ((uint32_t)k < sha256_tail_blocks(r)) {
                if (k < 2) L.get_row(trow, tail, 4 * k, 4 * k + 4);
                sha256_tail_block(k, tail, r, bits, x);
                sha256_compress(st, x);
            }
        }
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
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = bswap32(st[i]);
    }
    if (!OPEN) {
        if (valid) {
            for (uint32_t i = 0; i < 32u; ++i) *L.slot_byte(r + i) = (uint8_t)(d[i >> 2] >> (8u * (i & 3u)));
        }
        finish_record<false>(p.d, g, d, nullptr, nullptr, 0u);  // an unprocessed record's slot is zeroed
        ENET_DX_BARRIER();  // T2
    } else {
        uint32_t diff = valid ? 0u : 1u;
        if (valid) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint32_t v = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) v |= (uint32_t)*L.slot_byte(r + 4u * j + b) << (8 * b);
                diff |= v ^ d[j];
            }
            // the length field must give the body (SessionManager.cpp:770-796)
            const uint32_t be = bswap32(ld32(p.d.in + g.ib + 12));
            if ((uint64_t)be != g.Li - kWire) diff = 1u;
        }
        ENET_DX_BARRIER();  // T2: the header and hash findings are posted
        if (live) {
            const uint32_t hs = L.hs_s[L.rl], sd = L.sha_s[L.rl];
            const uint32_t status = diff ? 1u : hs ? hs : sd ? 4u : 0u;
            p.status[rec] = (uint8_t)status;
            if (p.ttl_out) p.ttl_out[rec] = status ? 0u : L.ttl_s[L.rl];
            if (status) {  // no plaintext and no stored ciphertext of a failed record
                zero_bytes(p.d.out + g.ob, g.Lo);
                if (p.data_out) zero_bytes(p.data_out + g.ob, g.Lo);
            }
        }
    }
}

// ================================================================== seal: cipher lane
__device__ __forceinline__ void cf_seal_cipher(const ChunkFrameParams& p, const DuplexGeom& g, const CfLane& L) {
    const uint32_t rec = g.rec, Ts = g.Ts(), r = g.r(), Tmax = L.Tmax;
    const uint64_t tb = g.tb();
    const bool live = g.live, valid = g.valid;
    const uint8_t* src = p.d.in + g.ib;          // data byte 0 = message byte 42
    uint8_t* dst = p.d.out + g.ob + kWire;       // body
    uint32_t nw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) nw[i] = live ? ld32(p.d.nonces + 12ull * rec + 4 * i) : 0u;
    ChachaRecord R;
    chacha_record_init(R, L.kw, nw);

    // the header as 10 LE words and a half (encode, Message.cpp:204-246; clamp_version, :17-25)
    uint32_t h[11];
    {
        uint32_t ver = (live && p.versions) ? p.versions[rec] : 4u;
        ver = ver < 1u ? 1u : (ver > 4u ? 4u : ver);
        const uint32_t tl = bswap32(live ? p.ttl[rec] : 0u), dl = bswap32((uint32_t)g.Li);
        uint32_t id[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) id[j] = live ? ld32(p.chunk_ids + 32ull * rec + 4 * j) : 0u;
        h[0] = ver | 0x300u | (tl << 16);
        h[1] = (tl >> 16) | (dl << 16);
        h[2] = (dl >> 16) | (id[0] << 16);
#pragma unroll
        for (int j = 1; j < 8; ++j) h[2 + j] = (id[j - 1] >> 16) | (id[j] << 16);
        h[10] = id[7] >> 16;
    }

    uint32_t pf[32];
    auto load_run = [&](uint32_t s) {
        if (s == 0) {  // header, then data bytes 0..85: 2 bytes, 5 x 16, 4
#pragma unroll
            for (int i = 0; i < 10; ++i) pf[i] = h[i];
            pf[10] = h[10] | ((uint32_t)src[0] << 16) | ((uint32_t)src[1] << 24);
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                const uint4 v = *reinterpret_cast<const uint4*>(src + 2 + 16 * i);
                pf[11 + 4 * i] = v.x; pf[12 + 4 * i] = v.y; pf[13 + 4 * i] = v.z; pf[14 + 4 * i] = v.w;
            }
            pf[31] = *reinterpret_cast<const uint32_t*>(src + 82);
        } else {
            const uint4* q = reinterpret_cast<const uint4*>(src + (uint64_t)kRun * s - kHdr);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint4 v = q[i];
                pf[4 * i] = v.x; pf[4 * i + 1] = v.y; pf[4 * i + 2] = v.z; pf[4 * i + 3] = v.w;
            }
        }
    };
    if (Ts > 0) load_run(0);
    for (uint32_t s = 0; s < Tmax; ++s) {
        if (s < Ts) {
            uint32_t x[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) x[i] = pf[i];
            if (s + 1 < Ts) load_run(s + 1);
            L.put_row(L.row(L.msg, s), x);  // message bytes for the mac lane
            {
                uint32_t ka[16], kb[16];
                chacha_block2(R, 2u * s, 2u * s + 1u, ka, kb);
#pragma unroll
                for (int i = 0; i < 16; ++i) { x[i] ^= ka[i]; x[16 + i] ^= kb[i]; }
            }
            uint4* o = reinterpret_cast<uint4*>(dst + (uint64_t)kRun * s);
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = make_uint4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
        }
        ENET_DX_BARRIER();
    }

    // ---- ragged end: r message bytes (header || data when the message has no whole stage)
    uint32_t w[48];
#pragma unroll
    for (int i = 0; i < 48; ++i) w[i] = 0u;
    uint32_t ks[48];
#pragma unroll
    for (int i = 32; i < 48; ++i) ks[i] = 0u;
    if (valid) {
        if (Ts == 0) {
            const uint32_t n = r - kHdr;  // data bytes, 0..85
            uint32_t t[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) t[i] = 0u;
            if (n) load_block(src, min(n, 64u), t, n >= 16u);
            if (n > 64u) load_block(src + 64, n - 64u, t + 16, true);
#pragma unroll
            for (int i = 0; i < 10; ++i) w[i] = h[i];
            w[10] = h[10] | (t[0] << 16);
#pragma unroll
            for (int j = 0; j < 21; ++j) w[11 + j] = half_up(t, j);
        } else if (r) {
            const uint8_t* q = src + tb - kHdr;  // at least 86 record bytes lie in front
            load_block(q, min(r, 64u), w, true);
            if (r > 64u) load_block(q + 64, r - 64u, w + 16, true);
        }
        chacha_block2(R, 2u * Ts, 2u * Ts + 1u, ks, ks + 16);
        if (r + 32u > 128u) chacha_block(R, 2u * Ts + 2u, ks + 32);
        L.put_row(L.row(L.msg, Tmax), w);  // T1: the message tail to the mac lane
    }
    ENET_DX_BARRIER();  // T1
    ENET_DX_BARRIER();  // T2: the MAC sits behind the message tail in the slot
    if (valid) {
        // body tail = message tail || MAC, one run of body bytes
        const uint32_t t = r + 32u;
        L.get_row(L.row(L.msg, Tmax), w, 0, 8);
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const uint4 v = *reinterpret_cast<const uint4*>(L.xchunk(c));
            w[32 + 4 * c] = v.x; w[33 + 4 * c] = v.y; w[34 + 4 * c] = v.z; w[35 + 4 * c] = v.w;
        }
#pragma unroll
        for (int j = 0; j < 40; ++j) w[j] ^= ks[j];
        store_block(dst + tb, min(t, 64u), w);
        if (t > 64u) store_block(dst + tb + 64, min(t - 64u, 64u), w + 16);
        if (t > 128u) store_block(dst + tb + 128, t - 128u, w + 32);
        // nonce(12) || BE32(|body|) (SessionManager.cpp:376-385)
        *reinterpret_cast<uint4*>(p.d.out + g.ob) = make_uint4(nw[0], nw[1], nw[2], bswap32((uint32_t)(g.Lm + 32u)));
    }
}

}  // namespace

// Two forms of the open kernel.  !WIDE: capped at 168 VGPRs, so three waves share a SIMD and a CU
// holds four workgroups, one wave of each role on every SIMD -- the form for many short frames,
// where the work of the three roles (cipher 2 x 15.5, mac 27, sha 27 ops/B) must spread evenly
// over the SIMDs.  WIDE: no cap (two waves per SIMD) and the cipher lane prefetches the next
// stage across the barrier, as duplex_kernel_wide -- the form for long frames, where a workgroup
// has a CU to itself and the stage latency is what counts.  The seal kernel fits the cap as it is.
template <bool OPEN, bool WIDE>
__global__ __launch_bounds__(OPEN ? 3 * kRecs : 2 * kRecs) __attribute__((amdgpu_waves_per_eu(WIDE ? 1 : 3)))
void chunk_frames_kernel(ChunkFrameParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t slabs[(OPEN ? 4 : 2) * kBuf];  // msg [2], then pt [2]
    __shared__ __attribute__((aligned(16))) uint8_t text[kRecs * 32];
    __shared__ uint32_t hs_s[kRecs], ttl_s[kRecs], sha_s[kRecs];
    __shared__ uint32_t tmax_s;

    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    CfLane L;
    L.rl = lane;

    // ---- geometry (every lane of a record computes it)
    DuplexGeom g = duplex_geom(p.d, blockIdx.x * kRecs + lane);
    uint64_t Lm;
    bool fits;
    if (!OPEN) {
        Lm = g.Li + kHdr;
        fits = g.Lo == g.Li + kHdr + 32u + kWire;
    } else {  // frames shorter than header + MAC fail (SessionManager.cpp:770-796, Message.cpp:315)
        const bool whole = g.Li >= 32ull + kWire;
        Lm = whole ? g.Li - 32u - kWire : 0;
        fits = whole && g.Lo == (Lm >= kHdr ? Lm - kHdr : 0u);
    }
    // an index outside the session table fails closed: no key or midstate past the table is read
    const uint32_t sraw = (p.d.session && g.live) ? p.d.session[g.rec] : 0u;
    const bool sbad = p.d.session && sraw >= p.d.n_sessions;
    L.sid = sbad ? 0u : sraw;
    duplex_geom_message(g, Lm, fits && !sbad);
    L.chunked = OPEN && g.valid && g.Lm >= kHdr;

    if (threadIdx.x == 0) tmax_s = 0;
    __syncthreads();
    if (wave == 0 && g.Ts()) atomicMax(&tmax_s, g.Ts());
    __syncthreads();
    L.Tmax = __builtin_amdgcn_readfirstlane(tmax_s);
    // length-graded issue priority, as duplex.hip: a workgroup lasts as long as its longest
    // record's serial hash chains
    if (L.Tmax >= 256) __builtin_amdgcn_s_setprio(3);
    else if (L.Tmax >= 64) __builtin_amdgcn_s_setprio(2);
    else if (L.Tmax >= 16) __builtin_amdgcn_s_setprio(1);

    L.msg = slabs;
    L.pt = slabs + (OPEN ? 2 * kBuf : 0);
    L.text = text;
    L.hs_s = hs_s;
    L.ttl_s = ttl_s;
    L.sha_s = sha_s;
    L.msw = ((lane >> 1) & 7u) ^ ((lane & 1u) << 2);
    L.xsw = ((lane >> 2) ^ (lane >> 3)) & 1u;
    {
        const uint8_t* kp = p.d.session ? p.d.keys + 32ull * L.sid : p.d.keys + (size_t)p.d.key_stride * g.rec;
#pragma unroll
        for (int i = 0; i < 8; ++i) L.kw[i] = g.live ? reinterpret_cast<const uint32_t*>(kp)[i] : 0u;
    }

    if (OPEN) {
        if (wave == 0) cf_open_cipher<WIDE>(p, g, L);
        else if (wave == 1) cf_mac_lane<true>(p, g, L);
        else cf_sha_lane(p, g, L);
    } else {
        if (wave == 0) cf_seal_cipher(p, g, L);
        else cf_mac_lane<false>(p, g, L);
    }
}

hipError_t launch_chunk_frames(bool open, const ChunkFrameParams& p, hipStream_t s) {
    if (p.d.n == 0) return hipSuccess;
    const dim3 g((p.d.n + kRecs - 1) / kRecs);
    // the caller's hint picks the open kernel's form (speed only): frames of 16 KiB and more, as
    // the long-record rule of launch_duplex
    if (!open) hipLaunchKernelGGL((chunk_frames_kernel<false, false>), g, dim3(2 * kRecs), 0, s, p);
    else if (p.d.max_len >= 16384u) hipLaunchKernelGGL((chunk_frames_kernel<true, true>), g, dim3(3 * kRecs), 0, s, p);
    else hipLaunchKernelGGL((chunk_frames_kernel<true, false>), g, dim3(3 * kRecs), 0, s, p);
    return hipGetLastError();
}

}  // namespace enet
