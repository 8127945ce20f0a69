// control_frames.hip -- `Request` / `Acknowledge` wire frames and receive-side frame triage (gfx950).
//
// The two messages that open and close a chunk transfer (Node::request_chunk, Node.cpp:1748-1756;
// send_chunk_request_direct, :532-550; handle_chunk's ack, :2305-2317; send_negative_ack, :930-949;
// encode, Message.cpp:236-252; encode_signed, :305-311; SessionManager::send,
// SessionManager.cpp:362-387), with v = clamp_version(version) (Message.cpp:17-25):
//   Request      m = v || 0x02 || chunk_id(32) || requester(32)                |m| = 66
//   Acknowledge  m = v || 0x04 || accepted(1) || chunk_id(32) || peer_id(32)   |m| = 67
//   frame = nonce(12) || BE32(|m| + 32) || ChaCha20_{Ks,nonce,0}(m || HMAC_Ks(m))   114 / 115 bytes
// A frame is two keystream blocks and, from the session's HMAC midstates, three SHA-256
// compressions (66 + 9 > 64: two inner, one outer).  ONE lane does a whole frame in registers; 64
// frames per one-wave workgroup.
//
// Packed 114- / 115-byte frames land at every byte alignment, so no lane touches its frame in HBM:
// the workgroup moves its frames between HBM and LDS rows (33-word stride: lane-per-row reads and
// row-per-half-wave writes are both conflict-free) as dword rows -- thread t carries dword t % 32 of
// two records per pass, at the frame's own (unaligned) byte address, and the last 2 or 3 bytes ride
// in one dword window that ENDS at the frame's end (rewriting bytes of the dword before it with
// the same values).  No load touches a byte outside the frame, no store one outside the record's
// output range.
//
// seal      m is synthesized from kind, version, accepted, chunk id and the local id (no input
//           arena), signed, encrypted and laid into the lane's row; m never exists in memory.
// open      the lane decrypts and authenticates its row, parses m and writes ids / info / status
//           (SoA).  A frame of any other length still gets the exact verdict (FRAME before HEADER
//           needs its HMAC): the same lane code walks its 64-byte blocks, from the row up to 128
//           bytes and from HBM (16-byte loads) beyond; every well-formed frame is one block and a
//           34- / 35-byte end, so the walk's loop runs once unless such a frame is in the wave.
// classify  one keystream block (counter 0) per frame, 16 header bytes + one body dword read by
//           the lane (18 bytes used); per-class ballots, one atomic range reservation per class
//           and 256-record workgroup, indices ascending inside the workgroup's block.
#include "duplex_common.hpp"

namespace enet {

namespace {

constexpr uint32_t kRecs = kControlRecsPerWG;  // one wave, one lane per frame
constexpr uint32_t kWire = 16;                 // nonce(12) || BE32(|body|)
constexpr uint32_t kRowWords = 32, kRowStride = 33;
constexpr uint32_t kReq = 2, kAck = 4, kReqLen = 66, kAckLen = 67;
constexpr uint32_t kClassRecs = 256, kClasses = 5;

// clamp_version (Message.cpp:17-25)
__device__ __forceinline__ uint32_t clamp_version(uint32_t v) { return v < 1u ? 1u : (v > 4u ? 4u : v); }

// The record's session key as LE words; false: the session index lies outside the table (no key
// or midstate past it is read, the record fails closed).
__device__ __forceinline__ bool ct_key(const DuplexParams& d, const DuplexGeom& g, uint32_t& sid, uint32_t kw[8]) {
    const uint32_t sraw = (d.session && g.live) ? d.session[g.rec] : 0u;
    const bool sbad = d.session && sraw >= d.n_sessions;
    sid = sbad ? 0u : sraw;
    const uint8_t* kp = d.session ? d.keys + 32ull * sid : d.keys + (size_t)d.key_stride * g.rec;
#pragma unroll
    for (int i = 0; i < 8; ++i) kw[i] = g.live ? reinterpret_cast<const uint32_t*>(kp)[i] : 0u;
    return !sbad;
}

// the state after the key block ^ pad: the session's midstate, or computed in the lane
__device__ __forceinline__ void ct_hmac_state(const DuplexParams& d, uint32_t sid, const uint32_t (&kb)[8],
                                              uint32_t pad, uint32_t st[8]) {
    if (d.mid) {
        const uint32_t* ms = d.mid + 16ull * sid + (pad == kHmacOpad ? 8u : 0u);
#pragma unroll
        for (int i = 0; i < 8; ++i) st[i] = ms[i];
    } else {
        hmac_key_state(st, kb, pad);
    }
}

// Rows in: record rl's first len_s[rl] bytes (0: none; otherwise 48..128) at in + base_s[rl].
__device__ __forceinline__ void rows_load(const uint8_t* in, const uint64_t* base_s, const uint32_t* len_s,
                                          uint32_t* rows) {
    const uint32_t j = threadIdx.x & 31u;
#pragma unroll 4
    for (uint32_t it = 0; it < kRecs / 2; ++it) {
        const uint32_t rl = 2u * it + (threadIdx.x >> 5);
        const uint32_t L = len_s[rl], nd = L >> 2, tail = L & 3u;
        const uint8_t* p = in + base_s[rl];
        if (j < nd) rows[rl * kRowStride + j] = *reinterpret_cast<const uint32_t*>(p + 4u * j);
        else if (j == nd && tail) rows[rl * kRowStride + j] = *reinterpret_cast<const uint32_t*>(p + L - 4u) >> (8u * (4u - tail));
    }
}

// Rows out: record rl's len_s[rl] bytes (0: none; otherwise 114 / 115) to out + base_s[rl].
__device__ __forceinline__ void rows_store(uint8_t* out, const uint64_t* base_s, const uint32_t* len_s,
                                           const uint32_t* rows) {
    const uint32_t j = threadIdx.x & 31u;
#pragma unroll 4
    for (uint32_t it = 0; it < kRecs / 2; ++it) {
        const uint32_t rl = 2u * it + (threadIdx.x >> 5);
        const uint32_t L = len_s[rl], nd = L >> 2, tail = L & 3u;
        uint8_t* p = out + base_s[rl];
        const uint32_t* row = rows + rl * kRowStride;
        if (j < nd) *reinterpret_cast<uint32_t*>(p + 4u * j) = row[j];
        else if (j == nd && tail) *reinterpret_cast<uint32_t*>(p + L - 4u) = __builtin_amdgcn_alignbyte(row[nd], row[nd - 1], tail);
    }
}

}  // namespace

// ================================================================== seal
__global__ __launch_bounds__(kRecs) void control_seal_kernel(ControlFrameParams p) {
    __shared__ uint32_t rows[kRecs * kRowStride];
    __shared__ uint64_t base_s[kRecs];
    __shared__ uint32_t len_s[kRecs];
    const uint32_t lane = threadIdx.x;
    DuplexGeom g = duplex_geom(p.d, blockIdx.x * kRecs + lane);  // in_off = out_off: Li = Lo
    const uint32_t kind = g.live ? p.kinds[g.rec] : kReq;
    const uint32_t v = clamp_version((g.live && p.versions) ? p.versions[g.rec] : 4u);
    const bool known = kind == kReq || kind == kAck;
    const uint32_t Lm = kind == kReq ? kReqLen : kAckLen;
    uint32_t sid, kw[8];
    const bool sok = ct_key(p.d, g, sid, kw);
    // 2 HEADER: no such kind (so no length to fit); 1 FRAME: the slot's size or the session index
    const uint32_t fail = !known ? 2u : (sok && g.ordered && g.Lo == (uint64_t)Lm + 32u + kWire) ? 0u : 1u;
    duplex_geom_message(g, Lm, fail == 0u);
    base_s[lane] = g.ob;
    len_s[lane] = g.valid ? (uint32_t)g.Lo : 0u;
    if (g.live) {
        p.status[g.rec] = (uint8_t)fail;
        if (fail) zero_bytes(p.d.out + g.ob, g.Lo);  // no frame of a record that was not sealed
    }
    if (g.valid) {
        // accepted (Ack only): NULL -> 0 (send_negative_ack); accept_zero inverts the table's sense
        // so that a status[] (0 = good) can be passed as it is (handle_chunk, Node.cpp:2305-2317)
        uint32_t acc = 0u;
        if (kind == kAck && p.accepted) acc = ((p.accepted[g.rec] != 0) != (p.accept_zero != 0)) ? 1u : 0u;
        // id = chunk_id || local id, 16 LE words; m = header (sh bytes) || id
        uint32_t id[17];
        {
            const uint32_t* c = reinterpret_cast<const uint32_t*>(p.chunk_ids + 32ull * g.rec);
            const uint32_t* l = reinterpret_cast<const uint32_t*>(p.peer_id);
#pragma unroll
            for (int j = 0; j < 8; ++j) { id[j] = c[j]; id[8 + j] = l[j]; }
            id[16] = 0u;
        }
        const uint32_t sh = kind == kReq ? 2u : 3u;
        uint32_t mm[17];
        mm[0] = v | (kind << 8) | (acc << 16) | (id[0] << (8u * sh));
#pragma unroll
        for (int j = 1; j < 17; ++j) mm[j] = __builtin_amdgcn_alignbyte(id[j], id[j - 1], 4u - sh);
        // HMAC_Ks(m) (HmacSha256.cpp:11-39): two inner compressions, one outer
        uint32_t kb[8], st[8], x[16], d[9];
#pragma unroll
        for (int i = 0; i < 8; ++i) kb[i] = bswap32(kw[i]);
        ct_hmac_state(p.d, sid, kb, kHmacIpad, st);
#pragma unroll
        for (int i = 0; i < 16; ++i) x[i] = bswap32(mm[i]);
        sha256_compress(st, x);
        {
            uint32_t tail[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) tail[i] = i == 0 ? mm[16] : 0u;
            sha256_tail_block(0, tail, sh, (64ull + Lm) * 8ull, x);
            sha256_compress(st, x);
        }
        {
            uint32_t inner[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) inner[i] = st[i];
            ct_hmac_state(p.d, sid, kb, kHmacOpad, st);
            hmac_outer_finish(st, inner);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) d[i] = bswap32(st[i]);
        d[8] = 0u;
        // body = m || MAC as 25 LE words, under keystream blocks 0 and 1
        uint32_t nw[3], ka[16], kc[16];
#pragma unroll
        for (int i = 0; i < 3; ++i) nw[i] = reinterpret_cast<const uint32_t*>(p.d.nonces + 12ull * g.rec)[i];
        ChachaRecord R;
        chacha_record_init(R, kw, nw);
        chacha_block2(R, 0u, 1u, ka, kc);
        uint32_t* row = rows + lane * kRowStride;
        row[0] = nw[0]; row[1] = nw[1]; row[2] = nw[2];
        row[3] = bswap32(Lm + 32u);  // SessionManager.cpp:376-385
#pragma unroll
        for (int i = 0; i < 16; ++i) row[4 + i] = mm[i] ^ ka[i];
        row[20] = ((mm[16] & (0xffffffffu >> (8u * (4u - sh)))) | (d[0] << (8u * sh))) ^ kc[0];
#pragma unroll
        for (int j = 1; j < 9; ++j) row[20 + j] = __builtin_amdgcn_alignbyte(d[j], d[j - 1], 4u - sh) ^ kc[j];
    }
    __syncthreads();
    rows_store(p.d.out, base_s, len_s, rows);
}

// ================================================================== open
__global__ __launch_bounds__(kRecs) void control_open_kernel(ControlFrameParams p) {
    __shared__ uint32_t rows[kRecs * kRowStride];
    __shared__ uint64_t base_s[kRecs];
    __shared__ uint32_t len_s[kRecs];
    const uint32_t lane = threadIdx.x;
    DuplexGeom g = duplex_geom(p.d, blockIdx.x * kRecs + lane);  // out_off = in_off
    // frames shorter than header + MAC fail (SessionManager.cpp:770-796, Message.cpp:315)
    const bool whole = g.Li >= 32ull + kWire;
    uint32_t sid, kw[8];
    const bool sok = ct_key(p.d, g, sid, kw);
    duplex_geom_message(g, whole ? g.Li - 32u - kWire : 0u, whole && sok);
    const bool staged = g.valid && g.Li <= 4ull * kRowWords;
    base_s[lane] = g.ib;
    len_s[lane] = staged ? (uint32_t)g.Li : 0u;
    __syncthreads();
    rows_load(p.d.in, base_s, len_s, rows);
    __syncthreads();

    uint32_t status = 1u, ver = 0u, type = 0u, acc = 0u, match = 0u;
    uint32_t cid[8], pid[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { cid[j] = 0u; pid[j] = 0u; }
    if (g.valid) {
        const uint32_t* row = rows + lane * kRowStride;
        const uint8_t* src = p.d.in + g.ib;
        // 64-byte block b of the body, n bytes of it: from the row, or past 128 bytes from HBM
        auto body = [&](uint64_t b, uint32_t n, uint32_t* w) __attribute__((always_inline)) {
            if (staged) {
#pragma unroll
                for (uint32_t i = 0; i < 16; ++i) {
                    const uint32_t at = 4u + 16u * (uint32_t)b + i;
                    w[i] = at < kRowWords ? row[at] : 0u;
                }
            } else {
                load_block(src + kWire + 64ull * b, n, w, true);  // 16 header bytes lie in front
            }
        };
        uint32_t hw[4];  // nonce = the frame's first 12 bytes (SessionManager.cpp:815-822), length
        if (staged) {
#pragma unroll
            for (int i = 0; i < 4; ++i) hw[i] = row[i];
        } else {
            const uint4 q = *reinterpret_cast<const uint4*>(src);
            hw[0] = q.x; hw[1] = q.y; hw[2] = q.z; hw[3] = q.w;
        }
        // the length field must give the body (SessionManager.cpp:770-796)
        uint32_t diff = (uint64_t)bswap32(hw[3]) != g.Li - kWire ? 1u : 0u;
        ChachaRecord R;
        chacha_record_init(R, kw, hw);
        uint32_t kb[8], st[8], x[16];
#pragma unroll
        for (int i = 0; i < 8; ++i) kb[i] = bswap32(kw[i]);
        ct_hmac_state(p.d, sid, kb, kHmacIpad, st);
        uint32_t mm[17];
#pragma unroll
        for (int i = 0; i < 17; ++i) mm[i] = 0u;
        const uint64_t nfull = g.Lm >> 6;  // 1 for every Request and Acknowledge
        for (uint64_t b = 0; b < nfull; ++b) {
            uint32_t ks[16];
            body(b, 64u, x);
            chacha_block(R, (uint32_t)b, ks);
#pragma unroll
            for (int i = 0; i < 16; ++i) x[i] ^= ks[i];
            if (b == 0) {
#pragma unroll
                for (int i = 0; i < 16; ++i) mm[i] = x[i];
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) x[i] = bswap32(x[i]);
            sha256_compress(st, x);
        }
        // the end: r message bytes and the MAC
        const uint32_t r = (uint32_t)g.Lm & 63u, tin = r + 32u;
        uint32_t w[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) w[i] = 0u;
        {
            uint32_t ks[16];
            body(nfull, min(tin, 64u), w);
            chacha_block(R, (uint32_t)nfull, ks);
#pragma unroll
            for (int i = 0; i < 16; ++i) w[i] ^= ks[i];
        }
        if (tin > 64u) {
            uint32_t ks[16];
            body(nfull + 1u, tin - 64u, w + 16);
            chacha_block(R, (uint32_t)nfull + 1u, ks);
#pragma unroll
            for (int i = 0; i < 16; ++i) w[16 + i] ^= ks[i];
        }
        mm[16] = w[0];
        uint32_t mac[8];
        extract_bytes<32, 8>(w, r, mac);
        const uint64_t bits = (64ull + g.Lm) * 8ull;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if ((uint32_t)k < sha256_tail_blocks(r)) {
                sha256_tail_block(k, w, r, bits, x);
                sha256_compress(st, x);
            }
        }
        {
            uint32_t inner[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) inner[i] = st[i];
            ct_hmac_state(p.d, sid, kb, kHmacOpad, st);
            hmac_outer_finish(st, inner);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) diff |= mac[i] ^ bswap32(st[i]);  // HmacSha256::verify, HmacSha256.cpp:41-54
        // decode (Message.cpp:134-143, 160-170): version, type and the class's exact length
        ver = mm[0] & 0xffu;
        type = (mm[0] >> 8) & 0xffu;
        const bool hdr = ver >= 1u && ver <= 4u &&
                         ((type == kReq && g.Lm == kReqLen) || (type == kAck && g.Lm == kAckLen));
        status = diff ? 1u : hdr ? 0u : 2u;
        if (status == 0u) {
            const uint32_t sh = type == kReq ? 2u : 3u;
            acc = (type == kAck && ((mm[0] >> 16) & 0xffu) != 0u) ? 1u : 0u;
            uint32_t sd = p.sender_ids ? 0u : 1u;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                cid[j] = __builtin_amdgcn_alignbyte(mm[j + 1], mm[j], sh);
                pid[j] = __builtin_amdgcn_alignbyte(mm[j + 9], mm[j + 8], sh);
                if (p.sender_ids) sd |= pid[j] ^ reinterpret_cast<const uint32_t*>(p.sender_ids + 32ull * g.rec)[j];
            }
            match = sd == 0u ? 1u : 0u;
        }
    }
    if (g.live) {
        const bool good = status == 0u;
        p.status[g.rec] = (uint8_t)status;
        uint4* co = reinterpret_cast<uint4*>(p.chunk_ids_out + 32ull * g.rec);
        co[0] = make_uint4(cid[0], cid[1], cid[2], cid[3]);
        co[1] = make_uint4(cid[4], cid[5], cid[6], cid[7]);
        if (p.peer_ids_out) {
            uint4* po = reinterpret_cast<uint4*>(p.peer_ids_out + 32ull * g.rec);
            po[0] = make_uint4(pid[0], pid[1], pid[2], pid[3]);
            po[1] = make_uint4(pid[4], pid[5], pid[6], pid[7]);
        }
        reinterpret_cast<uint32_t*>(p.info)[g.rec] = good ? (ver | (type << 8) | (acc << 16) | (match << 24)) : 0u;
    }
}

// ================================================================== classify
__global__ __launch_bounds__(kClassRecs) void frame_classify_kernel(ControlFrameParams p) {
    __shared__ uint32_t cnt_s[kClassRecs / 64][kClasses], base_s[kClassRecs / 64][kClasses];
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    DuplexGeom g = duplex_geom(p.d, blockIdx.x * kClassRecs + threadIdx.x);  // out_off = in_off
    uint32_t sid, kw[8];
    const bool sok = ct_key(p.d, g, sid, kw);
    uint32_t kind = 0u;  // BAD: what every open rejects as FRAME without looking at the body
    if (g.live && g.ordered && sok && g.Li >= 32ull + kWire) {
        const uint8_t* src = p.d.in + g.ib;
        const uint4 q = *reinterpret_cast<const uint4*>(src);
        const uint32_t c0 = *reinterpret_cast<const uint32_t*>(src + kWire);  // Li >= 48: inside the frame
        if ((uint64_t)bswap32(q.w) == g.Li - kWire) {
            const uint32_t nw[3] = {q.x, q.y, q.z};
            ChachaRecord R;
            chacha_record_init(R, kw, nw);
            uint32_t ks[16];
            chacha_block(R, 0u, ks);
            const uint32_t m0 = c0 ^ ks[0];
            const uint32_t ver = m0 & 0xffu, type = (m0 >> 8) & 0xffu;
            const uint64_t Lm = g.Li - 32u - kWire;
            // the least each decode takes (Message.cpp:75-121, 134-170); for Request and
            // Acknowledge the fused open wants the exact length
            const bool fits = type == 1u ? Lm >= kAnnounceFixed + (ver >= 3u ? 8u : 0u)
                            : type == kReq ? Lm == kReqLen
                            : type == 3u ? Lm >= kChunkFrameHeader
                            : type == kAck ? Lm == kAckLen : false;
            kind = (ver >= 1u && ver <= 4u && fits) ? type : 5u;
        }
    }
    if (g.live) p.kind[g.rec] = (uint8_t)kind;
    uint32_t rank = 0u;
#pragma unroll
    for (uint32_t k = 1; k <= kClasses; ++k) {
        const uint64_t mask = __ballot(kind == k);
        if (kind == k) rank = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) cnt_s[wave][k - 1] = (uint32_t)__popcll(mask);
    }
    __syncthreads();
    if (threadIdx.x < kClasses) {  // one range reservation per class for the whole workgroup
        uint32_t total = 0u;
        for (uint32_t w = 0; w < kClassRecs / 64; ++w) {
            base_s[w][threadIdx.x] = total;
            total += cnt_s[w][threadIdx.x];
        }
        const uint32_t b = total ? atomicAdd(p.counts + threadIdx.x, total) : 0u;
        for (uint32_t w = 0; w < kClassRecs / 64; ++w) base_s[w][threadIdx.x] += b;
    }
    __syncthreads();
    if (kind) p.lists[(uint64_t)(kind - 1u) * p.d.n + base_s[wave][kind - 1u] + rank] = g.rec;
}

hipError_t launch_control_frames(ControlOp op, const ControlFrameParams& p, hipStream_t s) {
    if (p.d.n == 0) return hipSuccess;
    if (op == CT_CLASSIFY) {
        if (hipError_t e = hipMemsetAsync(p.counts, 0, kClasses * sizeof(uint32_t), s); e != hipSuccess) return e;
        hipLaunchKernelGGL(frame_classify_kernel, dim3((p.d.n + kClassRecs - 1) / kClassRecs), dim3(kClassRecs), 0, s, p);
        return hipGetLastError();
    }
    const dim3 g((p.d.n + kRecs - 1) / kRecs);
    if (op == CT_SEAL) hipLaunchKernelGGL(control_seal_kernel, g, dim3(kRecs), 0, s, p);
    else hipLaunchKernelGGL(control_open_kernel, g, dim3(kRecs), 0, s, p);
    return hipGetLastError();
}

}  // namespace enet
