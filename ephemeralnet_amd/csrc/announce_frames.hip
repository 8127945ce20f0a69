// announce_frames.hip -- an `Announce` message's wire frame in one HBM pass (gfx950).
//
// The reference gossips a manifest as an `Announce` message inside a session frame
// (Node::deliver_manifest, Node.cpp:2512-2661; encode, Message.cpp:215-235; encode_signed,
// Message.cpp:305-311; SessionManager::send, SessionManager.cpp:362-387), after a proof-of-work
// search over a re-serialisation of the same fields (announce_pow_digest, Node.cpp:155-173;
// compute_announce_pow, :212-230):
//   m     = v || 0x01 || BE32(ttl) || BE32(E) || BE32(U) || BE32(A) || chunk_id(32) || peer_id(32)
//           || endpoint || uri || shards || [BE64(work_nonce) only when v == 4]
//   frame = nonce(12) || BE32(|m| + 32) || ChaCha20_{Ks,nonce,0}(m || HMAC_Ks(m))
//   pow   = SHA-256(BE64(32) || chunk_id || BE64(32) || peer_id || BE64(E) || endpoint || BE64(U)
//           || uri || BE64(A) || shards || BE64(ttl) || BE64(work_nonce))
// and the receiver opens the frame, parses m (decode reads the nonce for v >= 3,
// Message.cpp:284) and checks sender, manifest and proof of work (handle_transport_message /
// handle_announce, Node.cpp:2332-2357; verify_announce_pow, :1144-1151).
//
// The PoW stream holds the bytes of m[18 .. ) in the same order with five 8-byte length words
// spliced in: the byte distance between a field in the stream and in m is -10, -2, 6, 14, 22 --
// always 2 mod 4.  A stream word that lies inside one field is therefore a 16-bit funnel shift
// (v_alignbyte) of two aligned message words, whatever E, U and A are; only the words that touch
// a splice, the ttl / nonce words or the padding are assembled byte-wise (pow_stream_block).
//
// open  three lanes per record, 64 records per 192-thread workgroup: wave 0 "cipher" (one
//       keystream, counter 0), wave 1 "mac" (HMAC-SHA256 over m from the session's midstates),
//       wave 2 "pow" (parses the header, checks sender and manifest, hashes the PoW stream).
//       Stages are 128 message bytes.  The cipher lane hands every stage to the other two through
//       a four-slot LDS ring (message byte b lives in slot (b / 128) % 4), one barrier per stage:
//       PoW block k needs message bytes [64 k - 24, 64 k + 76), so after stage s the pow lane
//       absorbs blocks 2s - 1 and 2s out of slots s - 1 and s while the cipher lane fills slot
//       s + 1.  The ragged end goes through the slot after the record's last whole stage plus a
//       32-byte extension (the MAC).  The mac lane holds the frame verdict, the pow lane the
//       admission verdict and the parsed fields; a failed record's output and info are zeroed.
// seal  launch a (only at difficulty > 0 with attempts to spend): one workgroup per record; the
//       hashing template of pow_common.hpp is prepared straight from the field arenas (blocks
//       gathered by the same pow_stream_block, absorbed one at a time) and searched on the
//       ENET_POW_NODE schedule.  Launch b: two lanes per record (cipher, mac); stage bytes are
//       the 82 synthesized header bytes, then dwords gathered from the endpoint, uri and shard
//       arenas (byte-wise only across a field boundary), then the nonce.  Neither m nor the PoW
//       prefix exists in HBM.
// No load touches a byte outside the frame / the fields' ranges, no store one outside the
// record's output range.
#include "duplex_common.hpp"
#include "pow_common.hpp"

namespace enet {

namespace {

constexpr uint32_t kRun = kDxRun;
constexpr uint32_t kRecs = 64;               // records per workgroup: one wave per role
constexpr uint32_t kBuf = kRecs * kRun;      // one stage of the workgroup in one ring slot
constexpr uint32_t kFixed = kAnnounceFixed;  // 82
constexpr uint32_t kWire = 16;               // nonce(12) || BE32(|body|)
constexpr uint32_t kOpenSlots = 4, kSealSlots = 2;

// bytes [2 + 4 j, 6 + 4 j) of the LE byte string in w
__device__ __forceinline__ uint32_t half_up(const uint32_t* w, int j) {
    return __builtin_amdgcn_alignbyte(w[j + 1], w[j], 2);
}

// What the lanes of a record share beside its geometry.
struct AfLane {
    uint32_t sid, rl, Tmax;  // session index; the record's row; stages of the longest record
    uint32_t msw, xsw;       // 16-byte chunk swizzles of a 128-byte row / the 32-byte extension
    uint32_t smask;          // ring slots - 1
    uint32_t kw[8];          // session key, LE words
    uint8_t* msg;            // the ring [slots][kRecs][128]
    uint8_t* text;           // [kRecs][32]: bytes 128..159 of the ragged end (the MAC's overhang)
    uint32_t *hs_s, *diff_s; // per record: admission status (pow lane), frame verdict (mac lane)
    __device__ __forceinline__ uint8_t* row(uint32_t s) const { return msg + (s & smask) * kBuf + rl * kRun; }
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
    // message byte b in the ring (any b: the slot index wraps)
    __device__ __forceinline__ uint8_t* at(uint32_t b) const {
        return row(b >> 7) + 16u * (((b >> 4) & 7u) ^ msw) + (b & 15u);
    }
    // the aligned message word at byte b (b % 4 == 0)
    __device__ __forceinline__ uint32_t word(uint32_t b) const { return *reinterpret_cast<const uint32_t*>(at(b)); }
    __device__ __forceinline__ uint8_t* xchunk(int c) const { return text + rl * 32u + 16u * (c ^ xsw); }
    // byte i of the ragged end (slot Ts, then the extension)
    __device__ __forceinline__ uint8_t* slot_byte(uint32_t Ts, uint32_t i) const {
        return i < kRun ? row(Ts) + 16u * ((i >> 4) ^ msw) + (i & 15u)
                        : text + rl * 32u + 16u * (((i - kRun) >> 4) ^ xsw) + (i & 15u);
    }
};

// ================================================================== the PoW stream
// One record's announce fields as announce_pow_digest serialises them (120 + E + U + A bytes).
struct PowStream {
    uint32_t E, U, A, ttl, nhi, nlo;
    __device__ __forceinline__ uint64_t F() const { return (uint64_t)E + U + A; }
};

// a stream position relative to the block at p0, clamped far enough outside [0, 64]
__device__ __forceinline__ int32_t pow_rel(uint64_t abs, uint64_t p0) {
    const int64_t d = (int64_t)(abs - p0);
    return (int32_t)(d < -64 ? -64 : (d > 128 ? 128 : d));
}

// The 16 big-endian words of 64-byte block k of the padded PoW message
//   stream || 0x80 || 0... || BE64(bit length).
// SRC reads field bytes: src.run(f, p0, w) = the 16 words of a block that lies inside field f
// (0 chunk_id, 1 peer_id, 2 endpoint, 3 uri, 4 shards); src.word(f, p0, pj, lo, hi) = the word at
// stream position p0 + pj whose bytes [lo, hi) belong to field f (its other bytes are ignored).
// A word touches at most one field: the fields are 8 bytes apart.
template <class SRC>
__device__ __forceinline__ void pow_stream_block(const PowStream& S, uint64_t k, const SRC& src, uint32_t w[16]) {
    const uint64_t p0 = 64ull * k;
    const uint64_t e2 = 88ull + S.E, e3 = e2 + 8ull + S.U, e4 = e3 + 8ull + S.A;  // field ends
    const int32_t re0 = pow_rel(40, p0), re1 = pow_rel(80, p0), re2 = pow_rel(e2, p0), re3 = pow_rel(e3, p0),
                  re4 = pow_rel(e4, p0);
    const int32_t rs0 = pow_rel(8, p0), rs1 = pow_rel(48, p0), rs2 = pow_rel(88, p0), rs3 = pow_rel(e2 + 8, p0),
                  rs4 = pow_rel(e3 + 8, p0);
    {   // the block inside one field: no splice, no mask
        const bool b0 = 0 < re0, b1 = 0 < re1, b2 = 0 < re2, b3 = 0 < re3;
        const uint32_t f = b0 ? 0u : b1 ? 1u : b2 ? 2u : b3 ? 3u : 4u;
        const int32_t rs = b0 ? rs0 : b1 ? rs1 : b2 ? rs2 : b3 ? rs3 : rs4;
        const int32_t re = b0 ? re0 : b1 ? re1 : b2 ? re2 : b3 ? re3 : re4;
        if (rs <= 0 && re >= 64) {
            src.run(f, p0, w);
            return;
        }
    }
    // the low words of the BE64 splices (their high words are zero but the nonce's), then 0x80
    const int32_t c0 = pow_rel(4, p0), c1 = pow_rel(44, p0), c2 = pow_rel(84, p0), c3 = pow_rel(e2 + 4, p0),
                  c4 = pow_rel(e3 + 4, p0), c5 = pow_rel(e4 + 4, p0), c6 = pow_rel(e4 + 8, p0),
                  c7 = pow_rel(e4 + 12, p0), c8 = pow_rel(e4 + 16, p0);
    const uint64_t plen = e4 + 16ull, bits = plen * 8ull;
    const bool last = k == ((plen + 8ull) >> 6);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int32_t pj = 4 * j;
        const bool b0 = pj < re0, b1 = pj < re1, b2 = pj < re2, b3 = pj < re3;
        const uint32_t f = b0 ? 0u : b1 ? 1u : b2 ? 2u : b3 ? 3u : 4u;
        const int32_t rs = b0 ? rs0 : b1 ? rs1 : b2 ? rs2 : b3 ? rs3 : rs4;
        const int32_t re = b0 ? re0 : b1 ? re1 : b2 ? re2 : b3 ? re3 : re4;
        const int32_t lo = (rs > pj ? rs : pj) - pj, hi = (re < pj + 4 ? re : pj + 4) - pj;
        uint32_t v = 0u;
        if (hi > lo) {
            const uint32_t m = (0xffffffffu >> (8 * lo)) & (hi >= 4 ? 0xffffffffu : ~(0xffffffffu >> (8 * hi)));
            v = src.word(f, p0, pj, lo, hi) & m;
        }
        if (hi - lo < 4) {
            auto splice = [&](int32_t c, uint32_t V) {
                const int32_t sh = c - pj;
                return (sh <= -4 || sh >= 4) ? 0u : (sh >= 0 ? V >> (8 * sh) : V << (8 * -sh));
            };
            v |= splice(c0, 32u) | splice(c1, 32u) | splice(c2, S.E) | splice(c3, S.U) | splice(c4, S.A) |
                 splice(c5, S.ttl) | splice(c6, S.nhi) | splice(c7, S.nlo) | splice(c8, 0x80000000u);
        }
        w[j] = v;
    }
    if (last) {
        w[14] |= (uint32_t)(bits >> 32);
        w[15] |= (uint32_t)bits;
    }
}

// field bytes out of the decrypted message in the LDS ring: stream position p of field f is
// message byte p + 10 - 8 f
struct RingSource {
    const AfLane& L;
    __device__ __forceinline__ uint32_t word(uint32_t f, uint64_t p0, int32_t pj, int32_t, int32_t) const {
        const uint32_t a = (uint32_t)p0 + (uint32_t)pj + 8u - 8u * f;  // the aligned word below
        return bswap32(__builtin_amdgcn_alignbyte(L.word(a + 4u), L.word(a), 2));
    }
    __device__ __forceinline__ void run(uint32_t f, uint64_t p0, uint32_t w[16]) const {
        const uint32_t a = (uint32_t)p0 + 8u - 8u * f;
        uint32_t m[17];
#pragma unroll
        for (int j = 0; j < 17; ++j) m[j] = L.word(a + 4u * j);
#pragma unroll
        for (int j = 0; j < 16; ++j) w[j] = bswap32(half_up(m, j));
    }
};

// field bytes out of the caller's arenas (the search launch).  Every address here is workgroup-uniform, so the compiler would
// fetch it with scalar (SMEM) loads -- which ignore the low two address bits; the pointers are
// pinned in VGPRs so the loads are vector loads (unaligned-safe), as in pow_search_kernel.
struct ArenaSource {
    // bias = field 0's base minus its stream position; d<f> = what field f's bias adds to field
    // f - 1's.  (Sums of guarded terms, not a select chain over members: the compiler turns such
    // a chain into an indexed load from the struct, which then lives in scratch.)
    uint64_t bias, d1, d2, d3, d4;
    __device__ __forceinline__ const uint8_t* at(uint32_t f, uint64_t p) const {
        const uint64_t a = bias + (f >= 1u ? d1 : 0ull) + (f >= 2u ? d2 : 0ull) + (f >= 3u ? d3 : 0ull) +
                           (f >= 4u ? d4 : 0ull) + p;
        const uint8_t* q = reinterpret_cast<const uint8_t*>(a);
        asm volatile("" : "+v"(q));
        return q;
    }
    __device__ __forceinline__ uint32_t word(uint32_t f, uint64_t p0, int32_t pj, int32_t lo, int32_t hi) const {
        const uint8_t* q = at(f, p0 + (uint64_t)pj);
        if (lo == 0 && hi == 4) return bswap32(*reinterpret_cast<const uint32_t*>(q));
        uint32_t v = 0u;
#pragma unroll
        for (int b = 0; b < 4; ++b)
            if (b >= lo && b < hi) v |= (uint32_t)q[b] << (24 - 8 * b);
        return v;
    }
    __device__ __forceinline__ void run(uint32_t f, uint64_t p0, uint32_t w[16]) const {
        const uint4* q4 = reinterpret_cast<const uint4*>(at(f, p0));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 v = q4[i];
            w[4 * i] = bswap32(v.x); w[4 * i + 1] = bswap32(v.y);
            w[4 * i + 2] = bswap32(v.z); w[4 * i + 3] = bswap32(v.w);
        }
    }
};

struct ArenaBlocks {
    PowStream S;
    ArenaSource src;
    __device__ __forceinline__ void operator()(uint64_t k, uint32_t* w) const { pow_stream_block(S, k, src, w); }
};

// ================================================================== seal: a record's fields
// clamp_version (Message.cpp:17-25)
__device__ __forceinline__ uint32_t clamp_version(uint32_t v) { return v < 1u ? 1u : (v > 4u ? 4u : v); }

struct SealFields {
    bool ok;                     // indices inside their tables, offsets ordered, lengths 32-bit
    uint32_t v, E, U, A, ttl;
    const uint8_t *cid, *ep, *uri, *sh;
    __device__ __forceinline__ uint64_t F() const { return (uint64_t)E + U + A; }
    __device__ __forceinline__ uint64_t Lm() const { return (uint64_t)kFixed + F() + (v == 4u ? 8u : 0u); }
};

__device__ __forceinline__ SealFields seal_fields(const AnnounceFrameParams& p, uint32_t rec, bool live) {
    SealFields f{};
    f.v = clamp_version((live && p.versions) ? p.versions[rec] : 4u);
    if (!live) return f;
    const uint32_t mi = p.manifest ? p.manifest[rec] : rec, ei = p.endpoint ? p.endpoint[rec] : rec;
    if (mi >= p.manifests || ei >= p.endpoints) return f;
    const uint64_t u0 = p.uri_off[mi], u1 = p.uri_off[mi + 1], e0 = p.endpoint_off[ei], e1 = p.endpoint_off[ei + 1],
                   a0 = p.shard_off[rec], a1 = p.shard_off[rec + 1];
    if (u1 < u0 || e1 < e0 || a1 < a0) return f;
    const uint64_t U = u1 - u0, E = e1 - e0, A = a1 - a0;
    // the frame's length field is 32 bits wide: |m| + 32 must fit
    if ((U | E | A) >> 32 || U + E + A > 0xffffff00ull) return f;
    f.ok = true;
    f.E = (uint32_t)E; f.U = (uint32_t)U; f.A = (uint32_t)A;
    f.ttl = p.ttl[rec];
    f.cid = p.chunk_ids + 32ull * mi;
    f.ep = p.endpoint_bytes + e0;
    f.uri = p.uris + u0;
    f.sh = p.shards + a0;
    return f;
}

// What follows the 82 fixed bytes of a message to seal: endpoint || uri || shards || BE64(nonce)
// (v4 only), FL bytes in three arenas and a register pair.
struct FieldGather {
    // string position t of the endpoint lies at pe + t, of the uri at pe + du + t, of the shards
    // at pe + du + ds + t.  (Guarded sums, not select chains over members: see ArenaSource.)
    uint64_t pe, du, ds;
    int64_t E, U, A, N;  // the lengths of endpoint, uri, shards and the nonce (8 or 0)
    uint64_t nbe;        // byte i of BE64(nonce) = nbe >> 8 i
    __device__ __forceinline__ uint32_t byte(int64_t t) const {
        const int64_t b1 = E, b2 = b1 + U, b3 = b2 + A;
        if (t < 0 || t >= b3 + N) return 0u;
        if (t >= b3) return (uint32_t)(nbe >> (8 * (t - b3))) & 0xffu;
        const uint64_t a = pe + (t >= b1 ? du : 0ull) + (t >= b2 ? ds : 0ull) + (uint64_t)t;
        return *reinterpret_cast<const uint8_t*>(a);
    }
    // the LE word of bytes [t, t + 4) of the string, zero outside it: one dword load inside a
    // field, byte loads across a boundary
    __device__ __forceinline__ uint32_t word(int64_t t) const {
        const int64_t b1 = E, b2 = b1 + U, b3 = b2 + A;
        if (t + 4 <= 0 || t >= b3 + N) return 0u;
        const int64_t t0 = t < 0 ? 0 : t;
        const bool s1 = t0 >= b1, s2 = t0 >= b2, s3 = t0 >= b3;  // past the endpoint / uri / shards
        const int64_t lo = (s1 ? E : 0) + (s2 ? U : 0) + (s3 ? A : 0);
        const int64_t hi = E + (s1 ? U : 0) + (s2 ? A : 0) + (s3 ? N : 0);
        if (t >= lo && t + 4 <= hi) {
            if (s3) return (uint32_t)(nbe >> (8 * (t - b3)));
            const uint64_t a = pe + (s1 ? du : 0ull) + (s2 ? ds : 0ull) + (uint64_t)t;
            return *reinterpret_cast<const uint32_t*>(a);
        }
        return byte(t) | (byte(t + 1) << 8) | (byte(t + 2) << 16) | (byte(t + 3) << 24);
    }
    // 128 message bytes at message offset 128 s, zero past the message; h = the fixed bytes as
    // 20 LE words and a half
    __device__ __forceinline__ void run(uint32_t s, const uint32_t* h, uint32_t* x) const {
        const int64_t t = (int64_t)kRun * s - kFixed;
#pragma unroll
        for (int j = 0; j < 32; ++j) x[j] = word(t + 4 * j);
        if (s == 0) {
#pragma unroll
            for (int j = 0; j < 20; ++j) x[j] = h[j];
            x[20] = (x[20] & 0xffff0000u) | h[20];
        }
    }
};

__device__ __forceinline__ FieldGather field_gather(const SealFields& f, uint64_t nonce) {
    FieldGather G;
    const uint64_t pu = reinterpret_cast<uint64_t>(f.uri) - f.E, ps = reinterpret_cast<uint64_t>(f.sh) - f.E - f.U;
    G.pe = reinterpret_cast<uint64_t>(f.ep);
    G.du = pu - G.pe;
    G.ds = ps - pu;
    G.E = f.E; G.U = f.U; G.A = f.A; G.N = f.v == 4u ? 8 : 0;
    G.nbe = __builtin_bswap64(nonce);
    return G;
}

// ================================================================== open: cipher lane
__device__ __forceinline__ void af_open_cipher(const AnnounceFrameParams& p, const DuplexGeom& g, const AfLane& L) {
    const uint32_t Ts = g.Ts(), r = g.r(), Tmax = L.Tmax;
    const uint64_t tb = g.tb();
    const bool valid = g.valid;
    const uint8_t* src = p.d.in + g.ib + kWire;
    uint8_t* dst = p.d.out + g.ob;
    uint32_t nw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)  // nonce = the frame's first 12 bytes (SessionManager.cpp:815-822)
        nw[i] = valid ? ld32(p.d.in + g.ib + 4 * i) : 0u;
    ChachaRecord R;
    chacha_record_init(R, L.kw, nw);
    for (uint32_t s = 0; s < Tmax; ++s) {
        if (s < Ts) {
            uint32_t x[32];
            const uint4* q = reinterpret_cast<const uint4*>(src + (uint64_t)kRun * s);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint4 v = q[i];
                x[4 * i] = v.x; x[4 * i + 1] = v.y; x[4 * i + 2] = v.z; x[4 * i + 3] = v.w;
            }
            {   // the loads land while the keystream, which does not depend on them, is computed
                uint32_t ka[16], kb[16];
                chacha_block2(R, 2u * s, 2u * s + 1u, ka, kb);
#pragma unroll
                for (int i = 0; i < 16; ++i) { x[i] ^= ka[i]; x[16 + i] ^= kb[i]; }
            }
            L.put_row(L.row(s), x);
            uint4* o = reinterpret_cast<uint4*>(dst + (uint64_t)kRun * s);
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = make_uint4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
        }
        ENET_DX_BARRIER();  // stage s is in ring slot s % 4
    }
    // ---- ragged end: r message bytes and the MAC
    if (valid) {
        const uint32_t tin = r + 32u;
        uint32_t w[48];
#pragma unroll
        for (int i = 0; i < 48; ++i) w[i] = 0u;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (tin > 64u * k) {
                const uint32_t nk = min(64u, tin - 64u * k);
                load_block(src + tb + 64u * k, nk, w + 16 * k, true);  // 16 header bytes lie in front
            }
        }
        {
            uint32_t ka[16], kb[16];
            chacha_block2(R, 2u * Ts, 2u * Ts + 1u, ka, kb);
#pragma unroll
            for (int i = 0; i < 16; ++i) { w[i] ^= ka[i]; w[16 + i] ^= kb[i]; }
        }
        if (tin > 128u) {
            uint32_t kc[16];
            chacha_block(R, 2u * Ts + 2u, kc);
#pragma unroll
            for (int i = 0; i < 8; ++i) w[32 + i] ^= kc[i];
        }
        L.put_row(L.row(Ts), w);
#pragma unroll
        for (int c = 0; c < 2; ++c)
            *reinterpret_cast<uint4*>(L.xchunk(c)) = make_uint4(w[32 + 4 * c], w[33 + 4 * c], w[34 + 4 * c], w[35 + 4 * c]);
        if (r) store_block(dst + tb, min(r, 64u), w);
        if (r > 64u) store_block(dst + tb + 64, r - 64u, w + 16);
    }
    // the message stores are complete before the mac lane may zero them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    ENET_DX_BARRIER();  // T1
    ENET_DX_BARRIER();  // T2
}

// ================================================================== open: pow lane
// parse_announce_payload's view of the header (Message.cpp:75-121) and handle_announce's checks
// in their order; the PoW digest only where it decides.
__device__ __forceinline__ void af_pow_lane(const AnnounceFrameParams& p, const DuplexGeom& g, const AfLane& L) {
    const uint32_t Ts = g.Ts(), Tmax = L.Tmax, rec = g.rec;
    const uint32_t diff = p.difficulty;
    const RingSource src{L};
    PowStream S{};
    uint32_t ver = 0u, hs = 2u, st[8];
    bool hashing = false;
    sha256_init(st);
    auto parse = [&]() __attribute__((always_inline)) {  // the header is in slot 0: stage 0, or the ragged end of a short message
        uint32_t m[21];
#pragma unroll
        for (int j = 0; j < 21; ++j) m[j] = L.word(4u * j);
        ver = m[0] & 0xffu;
        const uint32_t type = (m[0] >> 8) & 0xffu;
        S.ttl = bswap32(half_up(m, 0));
        S.E = bswap32(half_up(m, 1));
        S.U = bswap32(half_up(m, 2));
        S.A = bswap32(half_up(m, 3));
        const uint64_t want = (uint64_t)kFixed + S.F() + (ver >= 3u ? 8u : 0u);
        const bool hdr = g.valid && ver >= 1u && ver <= 4u && type == 1u && want == g.Lm;
        uint32_t sd = 0u;
        if (hdr) {
#pragma unroll
            for (int j = 0; j < 8; ++j) sd |= half_up(m, 12 + j) ^ ld32(p.peer_ids + 32ull * rec + 4 * j);
        }
        hs = !hdr ? 2u : sd ? 3u : S.U == 0u ? 4u : 0u;
        hashing = hdr && ver >= 3u && diff != 0u;
    };
    auto absorb = [&](uint64_t k) __attribute__((always_inline)) {
        uint32_t w[16];
        pow_stream_block(S, k, src, w);
        sha256_compress(st, w);
    };
    for (uint32_t s = 0; s < Tmax; ++s) {
        ENET_DX_BARRIER();
        if (s < Ts) {
            if (s == 0) parse();
            if (hashing) {
                if (s > 0) absorb(2ull * s - 1ull);
                absorb(2ull * s);
            }
        }
    }
    ENET_DX_BARRIER();  // T1: the ragged end is in slot Ts
    if (Ts == 0) parse();
    uint32_t nlo = 0u, nhi = 0u;
    if (hs != 2u && ver >= 3u) {  // the nonce closes the message (read_u64, Message.cpp:116)
        const uint32_t at = (uint32_t)g.Lm - 8u;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            nhi |= (uint32_t)*L.at(at + b) << (24 - 8 * b);
            nlo |= (uint32_t)*L.at(at + 4 + b) << (24 - 8 * b);
        }
    }
    if (hashing) {
        S.nhi = nhi;
        S.nlo = nlo;
        const uint64_t plen = 120ull + S.F();
        const uint64_t nb = (plen + 72ull) >> 6;  // at most four blocks are left
        for (uint64_t k = Ts ? 2ull * Ts - 1ull : 0ull; k < nb; ++k) absorb(k);
        if (hs == 0u && digest_leading_zero_bits(st) < diff) hs = 5u;
    } else if (hs == 0u && diff != 0u) {
        hs = 5u;  // v1 / v2 carry no nonce (verify_announce_pow, Node.cpp:1148)
    }
    L.hs_s[L.rl] = hs;
    ENET_DX_BARRIER();  // T2: both verdicts are posted
    if (g.live) {
        const bool good = L.diff_s[L.rl] == 0u && hs == 0u;
        uint32_t* o = p.info + 8ull * rec;
        o[0] = good ? ver : 0u;
        o[1] = good ? S.ttl : 0u;
        o[2] = good ? S.E : 0u;
        o[3] = good ? S.U : 0u;
        o[4] = good ? S.A : 0u;
        o[5] = good ? nlo : 0u;
        o[6] = good ? nhi : 0u;
        o[7] = 0u;
    }
}

// ================================================================== mac lane (both directions)
// HMAC-SHA256_Ks(m) (HmacSha256.cpp:11-39).  seal: the MAC goes behind the message tail in the
// slot for the cipher lane to encrypt.  open: compare with the decrypted MAC (HmacSha256::verify,
// HmacSha256.cpp:41-54), post the verdict, then write status and zero a failed record.
// fail: seal only, the status of a record that is not sealed (0: it is).
template <bool OPEN>
__device__ __forceinline__ void af_mac_lane(const AnnounceFrameParams& p, const DuplexGeom& g, const AfLane& L,
                                            uint32_t fail) {
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
            const uint8_t* row = L.row(s);
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
        const uint8_t* trow = L.row(Ts);
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
            for (uint32_t i = 0; i < 32u; ++i) *L.slot_byte(Ts, r + i) = (uint8_t)(d[i >> 2] >> (8u * (i & 3u)));
        }
        if (live) {
            p.status[rec] = (uint8_t)fail;
            if (fail) {  // no frame and no nonce of a record that was not sealed
                zero_bytes(p.d.out + g.ob, g.Lo);
                p.work_nonce[rec] = 0ull;
            }
        }
        ENET_DX_BARRIER();  // T2
    } else {
        uint32_t diff = valid ? 0u : 1u;
        if (valid) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                uint32_t v = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) v |= (uint32_t)*L.slot_byte(Ts, r + 4u * j + b) << (8 * b);
                diff |= v ^ d[j];
            }
            // the length field must give the body (SessionManager.cpp:770-796)
            const uint32_t be = bswap32(ld32(p.d.in + g.ib + 12));
            if ((uint64_t)be != g.Li - kWire) diff = 1u;
        }
        L.diff_s[L.rl] = diff;
        ENET_DX_BARRIER();  // T2: both verdicts are posted
        if (live) {
            const uint32_t status = diff ? 1u : L.hs_s[L.rl];
            p.status[rec] = (uint8_t)status;
            if (status) zero_bytes(p.d.out + g.ob, g.Lo);  // no message of a failed record
        }
    }
}

// ================================================================== seal: cipher lane
__device__ __forceinline__ void af_seal_cipher(const AnnounceFrameParams& p, const DuplexGeom& g, const AfLane& L,
                                               const SealFields& f, uint64_t nonce) {
    const uint32_t rec = g.rec, Ts = g.Ts(), r = g.r(), Tmax = L.Tmax;
    const uint64_t tb = g.tb();
    const bool live = g.live, valid = g.valid;
    uint8_t* dst = p.d.out + g.ob + kWire;  // body
    uint32_t nw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) nw[i] = live ? ld32(p.d.nonces + 12ull * rec + 4 * i) : 0u;
    ChachaRecord R;
    chacha_record_init(R, L.kw, nw);

    // the 82 fixed bytes as 20 LE words and a half (encode, Message.cpp:215-229)
    uint32_t h[21];
    {
        const uint32_t tl = bswap32(f.ttl), el = bswap32(f.E), ul = bswap32(f.U), al = bswap32(f.A);
        // the local id is one address for the whole batch: a vector load, it may be unaligned
        const uint8_t* pid = p.peer_id;
        asm volatile("" : "+v"(pid));
        uint32_t id[16];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            id[j] = valid ? ld32(f.cid + 4 * j) : 0u;
            id[8 + j] = valid ? ld32(pid + 4 * j) : 0u;
        }
        h[0] = f.v | 0x100u | (tl << 16);
        h[1] = (tl >> 16) | (el << 16);
        h[2] = (el >> 16) | (ul << 16);
        h[3] = (ul >> 16) | (al << 16);
        h[4] = (al >> 16) | (id[0] << 16);
#pragma unroll
        for (int j = 1; j < 16; ++j) h[4 + j] = (id[j - 1] >> 16) | (id[j] << 16);
        h[20] = id[15] >> 16;
    }
    const FieldGather G = field_gather(f, nonce);
    for (uint32_t s = 0; s < Tmax; ++s) {
        if (s < Ts) {
            uint32_t x[32];
            G.run(s, h, x);
            L.put_row(L.row(s), x);  // message bytes for the mac lane
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
    // ---- ragged end: r message bytes
    uint32_t w[48], ks[48];
#pragma unroll
    for (int i = 0; i < 48; ++i) { w[i] = 0u; ks[i] = 0u; }
    if (valid) {
        G.run(Ts, h, w);  // zero past the message
        chacha_block2(R, 2u * Ts, 2u * Ts + 1u, ks, ks + 16);
        if (r + 32u > 128u) chacha_block(R, 2u * Ts + 2u, ks + 32);
        L.put_row(L.row(Ts), w);  // T1: the message tail to the mac lane
    }
    ENET_DX_BARRIER();  // T1
    ENET_DX_BARRIER();  // T2: the MAC sits behind the message tail in the slot
    if (valid) {
        // body tail = message tail || MAC, one run of body bytes
        const uint32_t t = r + 32u;
        L.get_row(L.row(Ts), w, 0, 8);
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

// the workgroup's longest record in stages, and the length-graded issue priority of duplex.hip
__device__ __forceinline__ uint32_t af_tmax(uint32_t* tmax_s, uint32_t wave, uint32_t Ts) {
    if (threadIdx.x == 0) *tmax_s = 0;
    __syncthreads();
    if (wave == 0 && Ts) atomicMax(tmax_s, Ts);
    __syncthreads();
    const uint32_t Tmax = __builtin_amdgcn_readfirstlane(*tmax_s);
    if (Tmax >= 256) __builtin_amdgcn_s_setprio(3);
    else if (Tmax >= 64) __builtin_amdgcn_s_setprio(2);
    else if (Tmax >= 16) __builtin_amdgcn_s_setprio(1);
    return Tmax;
}

// session index (an index outside the table fails closed: no key or midstate past it is read)
__device__ __forceinline__ bool af_session(const DuplexParams& d, const DuplexGeom& g, AfLane& L) {
    const uint32_t sraw = (d.session && g.live) ? d.session[g.rec] : 0u;
    const bool sbad = d.session && sraw >= d.n_sessions;
    L.sid = sbad ? 0u : sraw;
    return !sbad;
}

__device__ __forceinline__ void af_lane_setup(const DuplexParams& d, const DuplexGeom& g, AfLane& L, uint32_t lane) {
    L.msw = ((lane >> 1) & 7u) ^ ((lane & 1u) << 2);
    L.xsw = ((lane >> 2) ^ (lane >> 3)) & 1u;
    const uint8_t* kp = d.session ? d.keys + 32ull * L.sid : d.keys + (size_t)d.key_stride * g.rec;
#pragma unroll
    for (int i = 0; i < 8; ++i) L.kw[i] = g.live ? reinterpret_cast<const uint32_t*>(kp)[i] : 0u;
}

}  // namespace

__global__ __launch_bounds__(3 * kRecs) void announce_open_kernel(AnnounceFrameParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kOpenSlots * kBuf];
    __shared__ __attribute__((aligned(16))) uint8_t text[kRecs * 32];
    __shared__ uint32_t hs_s[kRecs], diff_s[kRecs];
    __shared__ uint32_t tmax_s;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    AfLane L;
    L.rl = lane;
    DuplexGeom g = duplex_geom(p.d, blockIdx.x * kRecs + lane);
    // frames shorter than header + MAC fail (SessionManager.cpp:770-796, Message.cpp:315)
    const bool whole = g.Li >= 32ull + kWire;
    const uint64_t Lm = whole ? g.Li - 32u - kWire : 0;
    const bool sok = af_session(p.d, g, L);
    duplex_geom_message(g, Lm, whole && g.Lo == Lm && sok);
    L.Tmax = af_tmax(&tmax_s, wave, g.Ts());
    L.msg = ring;
    L.text = text;
    L.smask = kOpenSlots - 1u;
    L.hs_s = hs_s;
    L.diff_s = diff_s;
    af_lane_setup(p.d, g, L, lane);
    if (wave == 0) af_open_cipher(p, g, L);
    else if (wave == 1) af_mac_lane<true>(p, g, L, 0u);
    else af_pow_lane(p, g, L);
}

__global__ __launch_bounds__(2 * kRecs) void announce_seal_kernel(AnnounceFrameParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kSealSlots * kBuf];
    __shared__ __attribute__((aligned(16))) uint8_t text[kRecs * 32];
    __shared__ uint32_t tmax_s;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    AfLane L;
    L.rl = lane;
    DuplexGeom g = duplex_geom(p.d, blockIdx.x * kRecs + lane);  // in_off = out_off: Li = Lo
    const SealFields f = seal_fields(p, g.rec, g.live && g.ordered);
    const bool sok = af_session(p.d, g, L);
    const uint64_t Lm = f.Lm();
    // 1 FRAME: an index outside its table or a slot of the wrong size; else what the search left
    uint32_t fail = (f.ok && sok && g.Lo == Lm + 32u + kWire) ? 0u : 1u;
    if (!fail && p.searched && g.live) fail = p.status[g.rec];
    duplex_geom_message(g, Lm, fail == 0u);
    // v < 4 carries no nonce (encode, Message.cpp:221); at difficulty 0 the nonce is 0
    // (compute_announce_pow, Node.cpp:213-216) unless the caller supplied it (max_attempts == 0)
    const bool given = g.valid && f.v == 4u && (p.searched || p.max_attempts == 0);
    const uint64_t nonce = given ? p.work_nonce[g.rec] : 0ull;
    L.Tmax = af_tmax(&tmax_s, wave, g.Ts());
    L.msg = ring;
    L.text = text;
    L.smask = kSealSlots - 1u;
    L.hs_s = nullptr;
    L.diff_s = nullptr;
    af_lane_setup(p.d, g, L, lane);
    if (wave == 0) {
        af_seal_cipher(p, g, L, f, nonce);
    } else {
        if (g.valid && !given) p.work_nonce[g.rec] = 0ull;
        af_mac_lane<false>(p, g, L, fail);
    }
}

// compute_announce_pow for one record per workgroup: the nonce into work_nonce, 0 / 5 (none within
// max_attempts) / 1 (an index outside its table) into status.  v < 4 records are not searched.
__global__ __launch_bounds__(1024) void announce_pow_kernel(AnnounceFrameParams p) {
    extern __shared__ uint64_t smem[];
    const uint32_t tid = threadIdx.x;
    const uint32_t rec = p.d.order ? p.d.order[blockIdx.x] : blockIdx.x;
    const SealFields f = seal_fields(p, rec, true);
    if (!f.ok || f.v != 4u) {
        if (tid == 0) {
            p.work_nonce[rec] = 0ull;
            p.status[rec] = f.ok ? 0 : 1;
        }
        return;
    }
    PowStream S{};
    S.E = f.E; S.U = f.U; S.A = f.A; S.ttl = f.ttl;
    ArenaSource src;
    {
        auto bias = [](const uint8_t* base, uint64_t start) { return reinterpret_cast<uint64_t>(base) - start; };
        const uint64_t b0 = bias(f.cid, 8), b1 = bias(p.peer_id, 48), b2 = bias(f.ep, 88),
                       b3 = bias(f.uri, 96ull + f.E), b4 = bias(f.sh, 104ull + f.E + f.U);
        src.bias = b0; src.d1 = b1 - b0; src.d2 = b2 - b1; src.d3 = b3 - b2; src.d4 = b4 - b3;
    }
    PowTemplate T;
    pow_prepare_blocks(112ull + S.F(), ArenaBlocks{S, src}, T);
    pow_uniform(T);
    const PowFound found = pow_search_run(T, p.difficulty, 0u, p.max_attempts, 0, smem);
    if (tid == 0) {
        p.work_nonce[rec] = found.nonce;
        p.status[rec] = found.ok ? 0 : 5;
    }
}

hipError_t launch_announce_frames(bool open, const AnnounceFrameParams& p, hipStream_t s) {
    if (p.d.n == 0) return hipSuccess;
    const dim3 g((p.d.n + kRecs - 1) / kRecs);
    if (open) {
        hipLaunchKernelGGL(announce_open_kernel, g, dim3(3 * kRecs), 0, s, p);
        return hipGetLastError();
    }
    AnnounceFrameParams q = p;
    q.searched = p.difficulty != 0 && p.max_attempts != 0;
    if (q.searched) {
        const uint32_t waves = pow_search_waves(p.d.n, p.max_attempts);
        const size_t lds = pow_search_lds_words(0, waves) * sizeof(uint64_t);
        hipLaunchKernelGGL(announce_pow_kernel, dim3(p.d.n), dim3(64 * waves), lds, s, q);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(announce_seal_kernel, g, dim3(2 * kRecs), 0, s, q);
    return hipGetLastError();
}

}  // namespace enet
