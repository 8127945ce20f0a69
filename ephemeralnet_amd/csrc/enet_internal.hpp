// enet_internal.hpp -- launch-side declarations shared by the kernel TUs and the C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "long_route.hpp"  // kMaxLanesPerRecord, RecMode, kSegMin, kSegTileBytes, SegEntry

namespace enet {

constexpr int kWG = 256;           // threads per workgroup (4 waves of 64)

// Kernel parameters for the ChaCha20 / AEAD record engine (passed by value).
struct RecParams {
    uint32_t n;
    const uint64_t* in_off;
    const uint64_t* out_off;
    const uint8_t* in;
    uint8_t* out;
    const uint8_t* keys;
    uint32_t key_stride;
    const uint8_t* nonces;
    const uint32_t* counters;  // MODE_XOR start counters (nullable -> 0)
    uint32_t counter_stride;   // words between records' counters (0 -> 1; 8 = LE32 of 32-B ids)
    const uint8_t* aad;        // nullable
    const uint64_t* aad_off;   // nullable
    const uint8_t* tag_in;     // open: expected tags
    uint8_t* tag_out;          // seal: produced tags
    uint8_t* ok;               // open: verdicts
    const uint32_t* order;     // nullable
    // frame mode (MODE_XOR over in || mac): when non-null, bytes [len_in, len_in+32) of the
    // virtual input come from append[32*rec]
    const uint8_t* append;
    // uniform batch: every record is exactly uniform_len bytes in and out (0 = not uniform)
    uint64_t uniform_len;
    int coop;  // uniform-batch staging variant: 0 none, 1 register prefetch (default), 5 lockstep
    // COOP 1 with one lane per record and L % 128 != 0: stage whole aligned 128-byte lines
    // (COOP 4; needs 4-byte-aligned record starts and in / out starts equal mod 128)
    int coop_lines;
    int nt_stores;  // non-temporal whole-line output stores (ENET_NT_STORES=0 disables)
    int lockstep;   // staging 1: lockstep keystream in 512-thread workgroups (ENET_LOCKSTEP=0 disables)
    int stream;     // uniform batches with L % (128 P) == 0: the streaming kernel (stream.hip;
                    // ENET_STREAM=0 disables)
    int dbg;        // streaming kernel timing probes (ENET_STREAM_DBG bitmask, tools only; wrong
                    // output): 1 no HBM traffic, 2 no keystream, 4 no Poly1305, 64 no stores,
                    // 128 no DMA, 256 clock stamps
    int var;        // streaming kernel code variant (ENET_STREAM_VAR, tuning)
    uint32_t rec_base;  // first record index of this launch (record = group + rec_base)
    // wire frames (frame modes only): every frame starts with a hdr-byte header
    // nonce(12) || BE32(|body|) (SessionManager.cpp:376-387).  Seal writes it in front of the
    // body; open reads the nonce from it.
    uint32_t hdr;
    // records the sequence-parallel path (segments.hip) claimed: skip[pos] != 0 -> the record at
    // position pos of the launch is not this kernel's (nullable; [n] bytes; set only for one
    // per-lane launch over the whole batch, rec_base == 0)
    const uint8_t* skip;
};

// lanes: 1, 2, 4, 8 or 16 lanes per record.
hipError_t launch_records(int mode, const RecParams& p, uint32_t lanes, hipStream_t s);
// records handed to launches of each kind so far (record_route.hpp RecordKind order; records.hip)
void record_route_counts(uint64_t out[5]);
// The streaming kernel (stream.hip): whole 512-thread workgroups of a uniform batch
// (record_route.hpp decides which batches).
hipError_t launch_stream(int mode, const RecParams& p, uint32_t lanes, uint32_t blocks, hipStream_t s);

struct ShaParams {
    uint32_t n;
    const uint8_t* in;
    const uint64_t* off;
    uint8_t* digest;           // [n][32], or an arena when dest_off != null
    const uint64_t* dest_off;  // nullable: digest i goes to digest + dest_off[i] + len_i
    // HMAC: when keys != null the lane computes HMAC(key_i, msg_i) (HmacSha256.cpp:11-39)
    const uint8_t* keys;
    const uint64_t* key_off;   // nullable: fixed 32-byte keys
    uint32_t key_stride;       // 32 or 0 (shared key) when key_off == null
    const uint8_t* expect;     // verify: expected MACs [n][32] (nullable -> compute only)
    uint8_t* ok;               // verify verdicts
    const uint64_t* guard_off; // verify: records whose guard length is < 32 fail (Message.cpp:315)
    uint8_t* zero_on_fail;     // verify: arena (indexed like `in`) to zero for failed records
    int and_ok;                // verify: ok[i] &= (mac matches) instead of ok[i] = ...
    // verify on wire frames: guard_off indexes the frames in wire_in; a frame shorter than
    // wire_hdr + 32 or whose BE32 length field differs from its body length fails
    const uint8_t* wire_in;
    uint32_t wire_hdr;
    const uint32_t* order;     // nullable
};
hipError_t launch_sha(const ShaParams& p, hipStream_t s);

// One-pass cipher + hash over ANY batch (duplex.hip): every record length, every alignment, any
// order.  A cipher lane and a hash lane per record; the message crosses HBM once.
enum DuplexKind : int {
    DK_FRAME = 0,  // frames: body = ChaCha20_{K,N,0}(m || HMAC_K(m)), [hdr] in front
    DK_CHUNK = 1,  // chunk store / fetch: ChaCha20 from LE32(chunk_id) + SHA-256(m)
    DK_AEADH = 2,  // RFC 8439 AEAD (counter 1, Poly1305 over the ciphertext) + HMAC_K(m)
};
constexpr uint32_t kDuplexRecsPerWG = 256;
struct DuplexParams {
    uint32_t n;
    const uint8_t* in;
    const uint64_t* in_off;
    uint8_t* out;
    const uint64_t* out_off;
    const uint8_t* keys;
    uint32_t key_stride;
    const uint8_t* nonces;     // [rec][12]; wire open (hdr 16) reads the frame header instead
    const uint32_t* order;     // nullable: position -> record (e.g. length-sorted)
    uint32_t hdr;              // frames: 0 or 16 (nonce || BE32 body length)
    const uint8_t* chunk_ids;  // chunks: start counter LE32(id[0..3])
    uint8_t* digests;          // chunk store: SHA-256(m)
    const uint8_t* expect;     // chunk fetch: expected SHA-256(m)
    uint8_t* macs;             // frame open: decrypted MACs; AEADH seal: HMAC_K(m)
    const uint8_t* macs_in;    // AEADH open: expected HMAC_K(m)
    uint8_t* tags;             // AEADH seal: Poly1305 tags
    const uint8_t* tags_in;    // AEADH open: expected tags
    uint8_t* ok;               // open / fetch verdicts
    int uniform;               // host hint: every record the same length (scheduling only)
    uint32_t max_len;          // host hint: longest record (scheduling only; 0 = unknown)
    int prio;                  // issue priority: 0 = length-graded (default), -1 = none,
                               // 1 = hash waves first, 2 = cipher waves first
    // session-keyed frames (nullable): record i uses key keys[32 * session[i]] and the session's
    // HMAC midstates mid[16 * session[i]] (inner state, outer state) instead of absorbing
    // key ^ ipad / key ^ opad itself
    const uint32_t* session;
    const uint32_t* mid;
    uint32_t n_sessions;  // session[i] >= n_sessions: the frame never authenticates
};
hipError_t launch_duplex(int kind, bool open, const DuplexParams& p, hipStream_t s);
// chunk / AEAD+HMAC kinds with each record's work split over cipher, schedule and rounds waves
// (duplex_split.hip): a shorter serial chain for long records
hipError_t launch_duplex_split(int kind, bool open, const DuplexParams& p, hipStream_t s);
// -1 auto (split when the longest record is >= 16 KiB), 0 never, 1 always (chunk / AEADH kinds)
int duplex_split_mode();

// Chunk transfer frames (chunk_frames.hip): a `Chunk` message (Message.cpp:204-246) inside a wire
// frame, sealed from / opened to the stored chunk in one pass.  d carries the arenas, offsets,
// order, the session keys (per record, or the table with session / mid / n_sessions) and, for
// seal, the frame nonces; the rest are [n] device arrays at any alignment unless noted.
constexpr uint32_t kChunkFrameHeader = 42;  // version, type, BE32 ttl, BE32 |data|, chunk_id(32)
struct ChunkFrameParams {
    DuplexParams d;
    const uint8_t* chunk_ids;     // [n][32]: seal puts it in the header, open expects it there
    const uint32_t* ttl;          // seal: seconds (4-byte aligned)
    const uint8_t* versions;      // seal, nullable: clamped to 1..4; NULL = 4
    const uint8_t* chunk_keys;    // open [n][32]
    const uint8_t* chunk_nonces;  // open [n][12]
    const uint8_t* chunk_hashes;  // open [n][32]: SHA-256(plaintext) the manifest promises
    uint8_t* data_out;            // open, nullable: the chunk ciphertext, at out_off
    uint32_t* ttl_out;            // open, nullable (4-byte aligned)
    uint8_t* status;              // open: 0 ok, 1 FRAME, 2 HEADER, 3 CHUNK_ID, 4 HASH
};
hipError_t launch_chunk_frames(bool open, const ChunkFrameParams& p, hipStream_t s);

// Announce frames (announce_frames.hip): an `Announce` message (Message.cpp:215-235) inside a wire
// frame.  Seal gathers the message from the manifest / endpoint / shard arenas and, at difficulty
// > 0, searches the announce proof of work first (compute_announce_pow, Node.cpp:212-230); open
// undoes the frame and runs handle_announce's admission checks (Node.cpp:2332-2357, :1144-1151).
// d carries the output arena and offsets, order, the session keys and, for seal, the frame
// nonces; seal reads no input arena (d.in_off = d.out_off, d.in unused).
constexpr uint32_t kAnnounceFixed = 82;  // version, type, BE32 ttl / E / U / A, chunk_id, peer_id
struct AnnounceFrameParams {
    DuplexParams d;
    // seal: the enet_announce_fields of the C ABI
    uint32_t manifests, endpoints;
    const uint8_t *chunk_ids, *uris, *endpoint_bytes, *shards, *peer_id, *versions;
    const uint64_t *uri_off, *endpoint_off, *shard_off;
    const uint32_t *manifest, *endpoint, *ttl;
    uint64_t max_attempts;
    uint64_t* work_nonce;      // [n]: found by the search, or the caller's when max_attempts == 0
    int searched;              // the seal kernel: the search launch ran and left status / work_nonce
    // open
    const uint8_t* peer_ids;   // [n][32]: the sessions' peers
    uint32_t* info;            // [n][8]: version, ttl, E, U, A, nonce low, nonce high, 0
    uint32_t difficulty;
    uint8_t* status;           // ENET_AF_* of enet_crypto.h
};
hipError_t launch_announce_frames(bool open, const AnnounceFrameParams& p, hipStream_t s);

// Request / Acknowledge frames and frame triage (control_frames.hip).  d carries the arenas,
// offsets, order and the session keys as for the chunk and announce frames (seal: in_off = out_off,
// d.in unused; open and classify: out_off = in_off, d.out unused).  The id tables, info, lists
// and counts are 4-byte aligned (checked by the C ABI).
constexpr uint32_t kControlRecsPerWG = 64;
enum ControlOp : int { CT_SEAL = 0, CT_OPEN = 1, CT_CLASSIFY = 2 };
struct ControlFrameParams {
    DuplexParams d;
    // seal
    const uint8_t* kinds;       // [n]: 2 Request, 4 Acknowledge
    const uint8_t* chunk_ids;   // [n][32]
    const uint8_t* peer_id;     // [32] the local id
    const uint8_t* accepted;    // [n], nullable -> 0
    int accept_zero;            // the wire byte is accepted[i] == 0 instead of != 0
    const uint8_t* versions;    // [n], nullable -> 4; clamped to 1..4
    // open
    const uint8_t* sender_ids;  // [n][32], nullable
    uint8_t* chunk_ids_out;     // [n][32]
    uint8_t* peer_ids_out;      // [n][32], nullable
    uint8_t* info;              // [n][4]: version, type, accepted, sender_match
    uint8_t* status;            // seal / open: ENET_CT_* of enet_crypto.h
    // classify
    uint8_t* kind;              // [n]: ENET_FK_*
    uint32_t* lists;            // [5][n]
    uint32_t* counts;           // [5]
};
hipError_t launch_control_frames(ControlOp op, const ControlFrameParams& p, hipStream_t s);

// waves per searching workgroup: enough that a grid of n jobs holds ~4 waves per SIMD (1024
// SIMDs), at most 16 (1024 threads), never more lanes than attempts
inline uint32_t pow_search_waves(uint32_t n, uint64_t max_attempts) {
    uint32_t waves = 1;
    while (waves < 16 && (uint64_t)n * waves < 4096 && 64ull * waves < max_attempts) waves <<= 1;
    return waves;
}

// Proof-of-work search / check (pow.hip): SHA-256(prefix_i || BE64(candidate)).
struct PowParams {
    uint32_t n;
    const uint8_t* prefixes;
    const uint64_t* off;
    const uint8_t* difficulty;     // per job, 0 -> nonce 0 / valid
    uint32_t schedule;             // 0 = start + attempt (Node.cpp), 1 = mt19937_64 stream (StoreProof.cpp)
    uint64_t max_attempts;
    uint64_t ring;                 // LDS candidate ring (power of two >= 64*waves + 312; 0 for schedule 0)
    uint64_t* nonces;              // search: found nonce
    uint64_t* attempts;            // search: attempt index of the nonce (nullable)
    uint8_t* found;                // search: found flag; check: valid flag
    const uint64_t* check_nonces;  // check: nonce per job
};
hipError_t launch_pow_search(const PowParams& p, uint32_t waves, hipStream_t s);
hipError_t launch_pow_check(const PowParams& p, hipStream_t s);

// HMAC-SHA256 midstates of n 32-byte keys: mid[16 i .. 16 i + 8) = state after (key ^ ipad),
// mid[16 i + 8 .. 16 i + 16) = state after (key ^ opad) (sha.hip)
hipError_t launch_hmac_midstates(uint32_t n, const uint8_t* keys, uint32_t* mid, hipStream_t s);

// KeyManager::derive_key for many sessions (sha.hip)
hipError_t launch_session_keys(uint32_t n, const uint8_t* secrets, const uint64_t* counters,
                               const int64_t* ticks, uint8_t* out, hipStream_t s);

// ---- device session table (handshake.hip): the enet_session_table of the C ABI, by value
struct SessionTableParams {
    uint32_t sessions;
    uint8_t* secrets;        // [S][32]
    uint8_t* keys;           // [S][32]
    uint32_t* mid;           // [S][16], the launch_hmac_midstates layout
    uint64_t* counters;      // [S]
    int64_t* last_rotation;  // [S]
    uint8_t* live;           // [S]
};
// verdicts (ENET_HS_* of enet_crypto.h)
enum : uint8_t { ENET_DEV_HS_BAD_PUBLIC = 0, ENET_DEV_HS_OK = 1, ENET_DEV_HS_BAD_POW = 2, ENET_DEV_HS_BAD_SLOT = 3 };
struct HandshakeParams {
    SessionTableParams table;
    uint32_t n;
    const uint8_t* peer_ids;        // [n][32], read only when difficulty != 0
    const uint32_t* remote_public;  // [n]
    const uint64_t* work_nonce;     // [n], nullable when difficulty == 0
    const uint32_t* slot;           // [n], nullable -> i
    const uint8_t* local_id;        // [32]
    uint32_t local_private, local_public, difficulty;
    int64_t now;
    uint8_t* verdict;               // [n]
};
// Node::perform_handshake's crypto for n peers into the table; rows and local_id 4-byte aligned,
// slots of one batch distinct (checked / documented by the C ABI)
hipError_t launch_handshake_accept(const HandshakeParams& p, hipStream_t s);
// KeyManager::rotate_if_needed over the whole table; rotated [S]
hipError_t launch_session_rotate(const SessionTableParams& t, int64_t now, int64_t interval, uint8_t* rotated,
                                 hipStream_t s);
// KeyExchange::compute_public / derive_shared_secret for n keypairs; remotes, public_out and
// secret_out nullable
hipError_t launch_key_exchange(uint32_t n, const uint32_t* privates, const uint32_t* remotes, uint32_t* public_out,
                               uint8_t* secret_out, hipStream_t s);

// Shamir split / combine of 32-byte secrets over GF(2^8)/0x11D (shamir.hip); 1 <= threshold <=
// share_count <= 255, the 32-byte-row buffers 4-byte aligned (checked by the C ABI)
hipError_t launch_shamir_split(uint32_t n, const uint8_t* secrets, const uint8_t* coeffs, uint32_t threshold,
                               uint32_t share_count, uint8_t* shares, hipStream_t s);
hipError_t launch_shamir_combine(uint32_t n, uint32_t threshold, const uint8_t* indices, const uint8_t* values,
                                 uint8_t* secrets_out, uint8_t* ok, hipStream_t s);

// ---- sequence-parallel path for long records (segments.hip)
// (SegEntry, a claimed record's entry, is in long_route.hpp beside the scratch layout)
constexpr uint64_t kSegMaxLen = 1ull << 35;  // 32-bit Poly1305 block positions inside a record
struct SegParams {
    int mode;                  // MODE_XOR / MODE_SEAL / MODE_OPEN
    uint32_t n;
    const uint64_t* in_off;
    const uint64_t* out_off;
    const uint8_t* in;
    uint8_t* out;
    const uint8_t* keys;
    uint32_t key_stride;
    const uint8_t* nonces;
    const uint32_t* counters;  // MODE_XOR start counters (nullable -> 0)
    uint32_t counter_stride;
    const uint8_t* aad;
    const uint64_t* aad_off;
    const uint8_t* tag_in;
    uint8_t* tag_out;
    uint8_t* ok;
    const uint32_t* order;     // nullable: the records to plan are order[0 .. n) (a subset)
    // scratch (stream-ordered, long_records.cpp seg_begin)
    unsigned long long* hdr;   // count << 40 | tiles claimed
    SegEntry* entries;         // [entry_cap]
    uint8_t* claimed;          // [n]: claimed[pos] != 0 -> the record at position pos of the launch
                               // (order[pos], or pos) is the tiles'; indexed by POSITION, so n
                               // bytes hold it whatever indices the order names
    uint32_t* partials;        // [tile_cap][8]
    uint32_t entry_cap, tile_cap;
    uint64_t long_min;
};
hipError_t launch_seg(const SegParams& p, uint32_t plan_blocks, uint32_t tile_blocks, hipStream_t s);
// ChaCha20 over a batch whose hints say every record is L >= kSegMin bytes: one launch of n *
// ceil(L / 64 KiB) tile workgroups; records whose real length differs are run whole by their
// tile-0 workgroup (p.n, offsets, arenas, keys, nonces, counters used; no scratch)
hipError_t launch_seg_uniform_xor(const SegParams& p, uint64_t L, hipStream_t s);
// RFC 8439 seal / open over such a batch, one launch (segments.hip seg_uniform_aead_kernel):
// p.partials [n * T][8] scratch; arrivals [n][seg_uniform_arrival_words()] zero at launch (reset
// by the kernel)
hipError_t launch_seg_uniform_aead(const SegParams& p, uint64_t L, uint32_t* arrivals, hipStream_t s);
uint32_t seg_uniform_arrival_words();
// dst[width * list[k] + b] = src[width * k + b], k < m, b < width
hipError_t launch_scatter(const uint8_t* src, const uint32_t* list, uint32_t m, uint8_t* dst, uint32_t width,
                          hipStream_t s);

// ---- long chunks: SHA-256 on host threads (chunk_hybrid.cpp)
// digests[32 k] = SHA-256 of record list[k] of the batch at `base` (device memory, or host memory
// the device maps), off = a HOST copy of its offsets; `ready` (nullable): an event the copies wait
// for.  0 or -1 (err set).
int host_hash_records(const uint8_t* base, const uint64_t* off, const uint32_t* list, uint32_t m,
                      hipEvent_t ready, uint32_t threads, uint8_t* digests, std::string& err);

uint32_t choose_lanes(uint32_t n, uint64_t total_bytes, uint32_t max_len);
uint32_t staging_variant();
// the text enet_last_error() returns on this host thread
void set_last_error(const std::string& what);

}  // namespace enet
