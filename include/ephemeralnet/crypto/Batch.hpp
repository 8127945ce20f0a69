// Batch.hpp -- crypto::batch: the many-records-per-call form of the reference API, for callers
// that collect work across sessions / chunks (batched session-frame codec, store
// pipeline).  Host memory in, host memory out (see below).  Device-resident callers use the C ABI
// (enet_crypto.h) directly.
#pragma once

#include <array>
#include <chrono>
#include <cstdint>
#include <future>
#include <optional>
#include <span>
#include <string>
#include <string_view>
#include <vector>

#include "ephemeralnet/crypto/CryptoTypes.hpp"
#include "ephemeralnet/crypto/ChaCha20.hpp"
#include "ephemeralnet/crypto/Shamir.hpp"

namespace ephemeralnet::crypto::batch {

struct Sealed {
    std::vector<std::uint8_t> data;
    std::array<std::uint8_t, 16> tag{};
};

// Every call below takes host memory and runs on the MI355X of the calling thread's device
// through the host-memory batch runtime: the records are gathered by host worker threads into
// pinned, device-mapped staging, chunk by chunk, while earlier chunks run on the device and
// later results are scattered back -- never a pageable hipMemcpy.  Outputs come either as one
// vector per record (the reference's own shape) or, for throughput, written into ONE
// caller-provided contiguous span: record i at packed_offsets(inputs, delta)[i], where delta is
// the op's length change (0 cipher / AEAD, +48 wire seal, -48 wire open, clamped at 0).
ENET_CXX_API std::vector<std::uint64_t> packed_offsets(std::span<const std::span<const std::uint8_t>> records,
                                                       std::int64_t delta);

// ChaCha20::apply for many records (counters[i] = start counter; empty span = all 0).
ENET_CXX_API std::vector<std::vector<std::uint8_t>> chacha20_apply(
    std::span<const Key> keys, std::span<const Nonce> nonces,
    std::span<const std::span<const std::uint8_t>> inputs, std::span<const std::uint32_t> counters);
ENET_CXX_API void chacha20_apply(std::span<const Key> keys, std::span<const Nonce> nonces,
                                 std::span<const std::span<const std::uint8_t>> inputs,
                                 std::span<const std::uint32_t> counters, std::span<std::uint8_t> out);

// RFC 8439 ChaCha20-Poly1305 (no AAD) for many records.
ENET_CXX_API std::vector<Sealed> aead_seal(std::span<const Key> keys,
                                           std::span<const Nonce> nonces,
                                           std::span<const std::span<const std::uint8_t>> plaintexts);
// Returns one entry per record; an empty optional-like flag vector `ok` says which verified.
ENET_CXX_API std::vector<std::vector<std::uint8_t>> aead_open(
    std::span<const Key> keys, std::span<const Nonce> nonces,
    std::span<const std::span<const std::uint8_t>> ciphertexts,
    std::span<const std::array<std::uint8_t, 16>> tags, std::vector<std::uint8_t>& ok);
// contiguous forms: ciphertexts / plaintexts packed into `out` (packed_offsets(.., 0)), tags[i],
// ok[i] (a failed record's plaintext is zeroed)
ENET_CXX_API void aead_seal(std::span<const Key> keys, std::span<const Nonce> nonces,
                            std::span<const std::span<const std::uint8_t>> plaintexts, std::span<std::uint8_t> out,
                            std::span<std::array<std::uint8_t, 16>> tags);
ENET_CXX_API void aead_open(std::span<const Key> keys, std::span<const Nonce> nonces,
                            std::span<const std::span<const std::uint8_t>> ciphertexts,
                            std::span<const std::array<std::uint8_t, 16>> tags, std::span<std::uint8_t> out,
                            std::span<std::uint8_t> ok);

// Vector-per-record outputs into caller-owned vectors that may be reused from call to call: `out`
// is resized to one entry per record and every entry is assigned its result, keeping its
// capacity -- a caller that keeps its result vectors (a relay's per-session buffers) pays no
// allocation per record.  The forms above that return fresh vectors allocate every record; with
// the system allocator that costs more than the crypto (host runtime).
ENET_CXX_API void chacha20_apply(std::span<const Key> keys, std::span<const Nonce> nonces,
                                 std::span<const std::span<const std::uint8_t>> inputs,
                                 std::span<const std::uint32_t> counters, std::vector<std::vector<std::uint8_t>>& out);
ENET_CXX_API void aead_seal(std::span<const Key> keys, std::span<const Nonce> nonces,
                            std::span<const std::span<const std::uint8_t>> plaintexts, std::vector<Sealed>& out);
ENET_CXX_API void aead_open(std::span<const Key> keys, std::span<const Nonce> nonces,
                            std::span<const std::span<const std::uint8_t>> ciphertexts,
                            std::span<const std::array<std::uint8_t, 16>> tags,
                            std::vector<std::vector<std::uint8_t>>& out, std::vector<std::uint8_t>& ok);

// SHA-256 digests of many messages (Sha256::digest).
ENET_CXX_API std::vector<std::array<std::uint8_t, 32>> sha256(
    std::span<const std::span<const std::uint8_t>> messages);

// Session frame bodies: ChaCha20_{K,N,0}(m || HMAC_K(m)) (Message.cpp:305-311 +
// SessionManager.cpp:362-374) and the inverse with MAC verification.
ENET_CXX_API std::vector<std::vector<std::uint8_t>> frame_seal(
    std::span<const std::array<std::uint8_t, 32>> session_keys, std::span<const Nonce> nonces,
    std::span<const std::span<const std::uint8_t>> messages);
ENET_CXX_API std::vector<std::vector<std::uint8_t>> frame_open(
    std::span<const std::array<std::uint8_t, 32>> session_keys, std::span<const Nonce> nonces,
    std::span<const std::span<const std::uint8_t>> bodies, std::vector<std::uint8_t>& ok);

// Chunk store pipeline (Node.cpp:1414-1417): chunk_hash = SHA-256(chunk) and the chunk sealed by
// CryptoManager::encrypt_with_key(key, chunk_id, chunk); chunk_ids empty = derive each id from
// content (security::derive_chunk_id, as the daemon does, ControlServer.cpp:1101).
struct StoredChunk {
    std::vector<std::uint8_t> data;
    std::array<std::uint8_t, 32> chunk_hash{};
};
ENET_CXX_API std::vector<StoredChunk> chunk_store(std::span<const Key> keys,
                                                  std::span<const Nonce> nonces,
                                                  std::span<const std::span<const std::uint8_t>> chunks,
                                                  std::span<const ChunkId> chunk_ids);
// Fetch side (Node.cpp:1641-1655): decrypt_with_key, then keep the plaintext only when its
// SHA-256 equals the manifest's chunk_hash (ok[i] = 1); failed entries come back zeroed.
ENET_CXX_API std::vector<std::vector<std::uint8_t>> chunk_fetch(
    std::span<const Key> keys, std::span<const Nonce> nonces, std::span<const ChunkId> chunk_ids,
    std::span<const std::span<const std::uint8_t>> ciphertexts,
    std::span<const std::array<std::uint8_t, 32>> chunk_hashes, std::vector<std::uint8_t>& ok);

// Shamir key shares for many 32-byte secrets (Shamir::split / Shamir::combine,
// src/crypto/Shamir.cpp:114-163), one device pass per call (enet_shamir_*_batch).
// shamir_split: result[i] = the share_count shares of secrets[i], indices 1 .. share_count, any
// `threshold` of which give the secret back.  The polynomial coefficients are a ChaCha20 keystream
// under a key drawn from std::random_device per call (the reference draws every coefficient byte
// from std::random_device, :127,141).  std::invalid_argument as Shamir::split.
ENET_CXX_API std::vector<std::vector<ShamirShare>> shamir_split(
    std::span<const std::array<std::uint8_t, 32>> secrets, std::uint8_t threshold, std::uint8_t share_count);
// shamir_combine: result[i] from the first `threshold` entries of shares[i], in their order.
// std::invalid_argument when threshold is 0 or a record has fewer shares.  ok[i] = 0 and a zero
// result when two of those entries have the same index (the reference throws there unless the
// values are zero; a batch fails closed per record instead).
ENET_CXX_API std::vector<std::array<std::uint8_t, 32>> shamir_combine(
    std::span<const std::vector<ShamirShare>> shares, std::uint8_t threshold, std::vector<std::uint8_t>& ok);

// The node's store step with the key sharing included (Node::store_chunk, Node.cpp:1414-1428):
// a fresh key per chunk (CryptoManager::generate_key; here a ChaCha20 keystream under a
// std::random_device key), chunk_store under those keys and the split of the keys, on one stream.
// The keys themselves are not returned: any `threshold` of a chunk's shares are its key.
struct SharedChunk {
    StoredChunk chunk;
    std::vector<ShamirShare> shares;
};
ENET_CXX_API std::vector<SharedChunk> chunk_store_shared(std::span<const Nonce> nonces,
                                                         std::span<const std::span<const std::uint8_t>> chunks,
                                                         std::span<const ChunkId> chunk_ids, std::uint8_t threshold,
                                                         std::uint8_t share_count);
// ... and the fetch step (Node::receive_chunk / fetch_chunk, Node.cpp:1632-1655): the first
// `threshold` shares of every chunk are combined on the device and chunk_fetch runs on the same
// stream with the combined keys where they lie -- no key crosses to the host.  ok[i] = 1 only
// when the shares combined (no duplicate index) AND the plaintext's SHA-256 equals
// chunk_hashes[i]; failed entries come back zeroed.
ENET_CXX_API std::vector<std::vector<std::uint8_t>> chunk_fetch_shared(
    std::span<const std::vector<ShamirShare>> shares, std::uint8_t threshold, std::span<const Nonce> nonces,
    std::span<const ChunkId> chunk_ids, std::span<const std::span<const std::uint8_t>> ciphertexts,
    std::span<const std::array<std::uint8_t, 32>> chunk_hashes, std::vector<std::uint8_t>& ok);

// Whole wire frames nonce(12) || BE32(|body|) || ChaCha20_{K,N,0}(m || HMAC_K(m)) -- what
// SessionManager::send writes (SessionManager.cpp:362-387) -- and their inverse, which takes the
// nonce from the frame and rejects frames whose length field disagrees with the body.
ENET_CXX_API std::vector<std::vector<std::uint8_t>> wire_seal(
    std::span<const std::array<std::uint8_t, 32>> session_keys, std::span<const Nonce> nonces,
    std::span<const std::span<const std::uint8_t>> messages);
ENET_CXX_API std::vector<std::vector<std::uint8_t>> wire_open(
    std::span<const std::array<std::uint8_t, 32>> session_keys,
    std::span<const std::span<const std::uint8_t>> frames, std::vector<std::uint8_t>& ok);
// contiguous forms: frames packed into `frames` (packed_offsets(messages, 48)); messages packed
// into `messages` (packed_offsets(frames, -48)), ok[i] (a failed message is zeroed)
ENET_CXX_API void wire_seal(std::span<const std::array<std::uint8_t, 32>> session_keys,
                            std::span<const Nonce> nonces, std::span<const std::span<const std::uint8_t>> messages,
                            std::span<std::uint8_t> frames);
ENET_CXX_API void wire_open(std::span<const std::array<std::uint8_t, 32>> session_keys,
                            std::span<const std::span<const std::uint8_t>> frames, std::span<std::uint8_t> messages,
                            std::span<std::uint8_t> ok);
// ... into reusable caller-owned vectors (see chacha20_apply above)
ENET_CXX_API void wire_seal(std::span<const std::array<std::uint8_t, 32>> session_keys,
                            std::span<const Nonce> nonces, std::span<const std::span<const std::uint8_t>> messages,
                            std::vector<std::vector<std::uint8_t>>& frames);
ENET_CXX_API void wire_open(std::span<const std::array<std::uint8_t, 32>> session_keys,
                            std::span<const std::span<const std::uint8_t>> frames,
                            std::vector<std::vector<std::uint8_t>>& messages, std::vector<std::uint8_t>& ok);
// The same frames from a table of session keys: frame i belongs to session_table[session[i]]
// (bytes identical to wire_seal / wire_open with session_keys[i] = session_table[session[i]]).
// The HMAC key-block midstates are computed once per table entry on the device
// (enet_hmac_midstates, enet_wire_*_batch_sessions).  Throws std::invalid_argument for a size
// mismatch or a session index outside the table.
ENET_CXX_API std::vector<std::vector<std::uint8_t>> wire_seal_sessions(
    std::span<const std::array<std::uint8_t, 32>> session_table, std::span<const std::uint32_t> session,
    std::span<const Nonce> nonces, std::span<const std::span<const std::uint8_t>> messages);
ENET_CXX_API std::vector<std::vector<std::uint8_t>> wire_open_sessions(
    std::span<const std::array<std::uint8_t, 32>> session_table, std::span<const std::uint32_t> session,
    std::span<const std::span<const std::uint8_t>> frames, std::vector<std::uint8_t>& ok);

// Chunk transfer frames (enet_chunk_frame_*_batch): a stored chunk onto the wire and off it in one
// device pass each.  chunk_frames_seal is Node::dispatch_upload's crypto (Node.cpp:1254-1297):
// frame i = the wire frame, under session_table[session[i]] and nonces[i], of the signed Chunk
// message version || 0x03 || BE32(ttl_seconds[i]) || BE32(|stored[i]|) || chunk_ids[i] || stored[i]
// (Message.cpp:204-246, 305-311; SessionManager.cpp:362-387); versions empty = 4, else clamped
// to 1..4.  chunk_frames_open is the receive side (SessionManager.cpp:760-822, Message.cpp:313-328,
// 144-159, Node::receive_chunk, Node.cpp:1615-1677): the frame is opened, its header checked
// against chunk_ids[i], the data decrypted under chunk_keys[i] / chunk_nonces[i] and
// SHA-256(plaintext) compared with chunk_hashes[i].  status = the first check that failed; a
// failed frame comes back with empty plaintext and stored and ttl 0.  A Chunk message with bytes
// after its data reports Header (decode would accept it; encode never writes one).  Throws
// std::invalid_argument for a size mismatch or a session index outside the table.
enum class ChunkFrameStatus : std::uint8_t { Ok = 0, Frame = 1, Header = 2, ChunkId = 3, Hash = 4 };
struct OpenedChunk {
    ChunkFrameStatus status = ChunkFrameStatus::Frame;
    std::uint32_t ttl_seconds = 0;
    std::vector<std::uint8_t> plaintext;  // what receive_chunk returns
    std::vector<std::uint8_t> stored;     // the chunk ciphertext the node keeps (chunk_store_.put, Node.cpp:1665)
};
ENET_CXX_API std::vector<std::vector<std::uint8_t>> chunk_frames_seal(
    std::span<const std::array<std::uint8_t, 32>> session_table, std::span<const std::uint32_t> session,
    std::span<const Nonce> nonces, std::span<const ChunkId> chunk_ids, std::span<const std::uint32_t> ttl_seconds,
    std::span<const std::span<const std::uint8_t>> stored, std::span<const std::uint8_t> versions = {});
ENET_CXX_API std::vector<OpenedChunk> chunk_frames_open(
    std::span<const std::array<std::uint8_t, 32>> session_table, std::span<const std::uint32_t> session,
    std::span<const std::span<const std::uint8_t>> frames, std::span<const ChunkId> chunk_ids,
    std::span<const Key> chunk_keys, std::span<const Nonce> chunk_nonces,
    std::span<const std::array<std::uint8_t, 32>> chunk_hashes);

// Announce frames (enet_announce_frame_*_batch): the gossip of a manifest, batched.
// announce_frames_seal is Node::deliver_manifest's crypto (Node.cpp:2512-2661) for many peers at
// once: the announce proof of work (compute_announce_pow, :212-230; at most max_attempts
// candidates, searched only for version-4 records and difficulty > 0; max_attempts == 0: the
// announces' own work_nonce is used), then frame i = the wire frame, under
// session_table[session[i]] and nonces[i], of the signed Announce message encode writes
// (Message.cpp:215-235: the version clamped to 1..4, the nonce only for version 4).  The caller
// keeps deliver_manifest's guard (difficulty > 0 needs version >= 3, Node.cpp:2639).  Every
// announce of one call carries the same peer_id, the local id.  A record without a nonce within
// max_attempts comes back with status Pow, an empty frame and nonce 0.
// announce_frames_open is the receive side (decode_signed -> handle_announce, Node.cpp:2332-2357):
// the frame is opened, the message parsed (decode expects the nonce for version >= 3, so a
// version-3 announce made by encode reports Header), peer_id compared with peers[i], an empty URI
// refused and the proof of work checked at `difficulty` (0: none asked; version < 3 fails any
// other, :1144-1151).  status = the first check that failed, in that order; a failed frame comes
// back with empty fields.  An Announce with bytes after its payload reports Header (decode would
// accept it; encode never writes one).  ttl is 32 bits wide: all the wire carries.  Throws
// std::invalid_argument for a size mismatch, a session index outside the table or differing
// peer_ids in one seal.
enum class AnnounceStatus : std::uint8_t { Ok = 0, Frame = 1, Header = 2, Sender = 3, NoManifest = 4, Pow = 5 };
struct AnnounceFields {
    ChunkId chunk_id{};
    PeerId peer_id{};
    std::string endpoint;
    std::uint32_t ttl_seconds = 0;
    std::string manifest_uri;
    std::vector<std::uint8_t> assigned_shards;
    std::uint8_t version = 4;
    std::uint64_t work_nonce = 0;
};
struct SealedAnnounces {
    std::vector<std::vector<std::uint8_t>> frames;
    std::vector<std::uint64_t> work_nonce;
    std::vector<AnnounceStatus> status;
};
struct OpenedAnnounce {
    AnnounceStatus status = AnnounceStatus::Frame;
    AnnounceFields fields;
};
inline constexpr std::uint64_t kNodePowAttempts = 500'000;  // kMaxAnnouncePowAttempts, Node.cpp:40
ENET_CXX_API SealedAnnounces announce_frames_seal(
    std::span<const std::array<std::uint8_t, 32>> session_table, std::span<const std::uint32_t> session,
    std::span<const Nonce> nonces, std::span<const AnnounceFields> announces, std::uint8_t difficulty,
    std::uint64_t max_attempts = kNodePowAttempts);
ENET_CXX_API std::vector<OpenedAnnounce> announce_frames_open(
    std::span<const std::array<std::uint8_t, 32>> session_table, std::span<const std::uint32_t> session,
    std::span<const std::span<const std::uint8_t>> frames, std::span<const PeerId> peers, std::uint8_t difficulty);

// Request / Acknowledge frames and frame triage (enet_control_frame_*_batch,
// enet_frame_classify_batch): the messages that open and close a chunk transfer, batched.
// control_frames_seal is Node::request_chunk's and handle_chunk's / send_negative_ack's crypto
// (Node.cpp:1748-1756, 532-550, 2305-2317, 930-949) for many peers at once: frame i = the wire
// frame, under session_table[session[i]] and nonces[i], of the signed message encode writes
// (Message.cpp:236-252; the version clamped to 1..4) -- version || 0x02 || chunk_id || local_id
// for a Request (114 bytes), version || 0x04 || accepted || chunk_id || local_id for an
// Acknowledge (115 bytes).  A record whose kind is neither comes back with status Header and an
// empty frame.
// control_frames_open is the receive side (decode_signed): status = the first failed check --
// Frame: what the general open rejects; Header: a version outside 1..4, another type, or a
// message that is not exactly 66 / 67 bytes (decode would accept trailing bytes; encode never
// writes them).  sender_match reports whether the message's requester / peer_id equals
// senders[i] (senders may be left empty: false); it is not enforced -- the reference acts on the
// transport's sender (handle_request, Node.cpp:2255-2284; handle_acknowledge, :2320-2330).  A
// failed frame comes back with zeroed fields.
// classify_frames is the triage of a mixed receive batch (receive loop,
// SessionManager.cpp:760-822; handle_transport_message, Node.cpp:2160-2179): one keystream block
// per frame, nothing authenticated; Bad = what every open rejects without reading the body, Other
// = for the general open.  A frame a fused open would accept is always given that open's kind.
// All three throw std::invalid_argument for a size mismatch or a session index outside the table;
// empty in gives empty out.
enum class ControlKind : std::uint8_t { Request = 2, Acknowledge = 4 };
enum class ControlStatus : std::uint8_t { Ok = 0, Frame = 1, Header = 2 };
enum class FrameKind : std::uint8_t { Bad = 0, Announce = 1, Request = 2, Chunk = 3, Acknowledge = 4, Other = 5 };
struct ControlFields {
    ControlKind kind = ControlKind::Request;
    ChunkId chunk_id{};
    bool accepted = false;  // Acknowledge only
    std::uint8_t version = 4;
};
struct SealedControls {
    std::vector<std::vector<std::uint8_t>> frames;
    std::vector<ControlStatus> status;
};
struct OpenedControl {
    ControlStatus status = ControlStatus::Frame;
    std::uint8_t version = 0;
    std::uint8_t type = 0;  // 2 Request, 4 Acknowledge
    bool accepted = false;
    ChunkId chunk_id{};
    PeerId peer_id{};
    bool sender_match = false;
};
ENET_CXX_API SealedControls control_frames_seal(
    std::span<const std::array<std::uint8_t, 32>> session_table, std::span<const std::uint32_t> session,
    std::span<const Nonce> nonces, std::span<const ControlFields> controls, const PeerId& local_id);
ENET_CXX_API std::vector<OpenedControl> control_frames_open(
    std::span<const std::array<std::uint8_t, 32>> session_table, std::span<const std::uint32_t> session,
    std::span<const std::span<const std::uint8_t>> frames, std::span<const PeerId> senders = {});
ENET_CXX_API std::vector<FrameKind> classify_frames(
    std::span<const std::array<std::uint8_t, 32>> session_table, std::span<const std::uint32_t> session,
    std::span<const std::span<const std::uint8_t>> frames);

// Cross-session frame queues.  SessionManager runs one detached reader
// thread per session (SessionManager.cpp:332-333, receive_loop :703-854) and sends from whatever
// thread calls Node::send_secure (:337-388), one ChaCha20 + HMAC per frame on that thread.  Here
// every thread hands its frame to a shared queue instead: the submitting thread reserves a slot in
// the queue's current PASS -- pinned, device-mapped staging -- and copies its frame, key and nonce
// straight into it (no lock on that path); a worker thread closes the pass once it is large enough,
// when frames stop arriving (30 us gap) or 250 us after its first frame, runs ONE wire-frame
// kernel over it on the MI355X
// (the kernel writes the pinned pass and reads it, or for a large pass -- 640+ frames sealing,
// 512+ opening -- a device copy of its input side), and every submitter copies its own result out
// of the pass (FrameTicket::get) or reads it in place (FrameTicket::view).  Passes grow with the offered load; several are in
// flight at once (max_inflight workers).  Results are matched by slot, so sessions never see each
// other's frames; bytes are identical to the per-frame reference path.
// Routing (enet_scalar_set_policy): blocking seal() / open() run on the calling thread's host
// engine under ENET_SCALAR_AUTO (default) and ENET_SCALAR_HOST -- one blocked caller per frame
// never builds a batch at which the device pays -- and through the queue under ENET_SCALAR_DEVICE.
// Non-blocking submit() / seal_async() / open_async() (a relay draining a socket buffer keeps
// many frames in flight) go through the queue under DEVICE, and under AUTO when the device is
// present and the submitting thread holds >= 320 submitted, uncollected frames (the measured
// crossover where the device queue overtakes the host engine in frames/s); on the
// host engine otherwise and under HOST.  A pass the device cannot run
// is finished on the host engine (never an exception into a session thread).
struct FrameQueueOptions {
    std::size_t max_frames = 4096;                     // at most this many frames per pass
    std::size_t max_bytes = 8u << 20;                  // ... and this many input bytes (a frame of
                                                       // the maximum payload always fits)
    std::chrono::microseconds max_delay{0};            // 0: a pass closes at max_frames / 4 or
                                                       // max_bytes / 4, after a 30 us arrival gap,
                                                       // or 250 us after its first frame; > 0: at
                                                       // the size limits or this long after its
                                                       // first frame
    std::size_t max_inflight = 8;                      // device passes in flight at once (one
                                                       // worker thread + HIP stream each; 1-16)
    int device = 0;                                    // HIP device of the device passes
};
struct FrameQueueStats {
    std::uint64_t frames = 0;   // frames served
    std::uint64_t flushes = 0;  // batched passes (frames / flushes = mean batch)
    std::uint64_t host_flushes = 0;  // passes served by the host engine (policy, no device, failure)
    std::uint64_t evicted = 0;  // results copied out of a pass to free it for new frames
    double pass_us = 0;         // mean wall time of a device pass (close -> results ready)
    double kernel_us = 0;       // ... of which the kernel (launch to completion)
    double worker_cpu_s = 0;    // CPU time of the queue's worker threads
    std::uint64_t cas_retries = 0;  // reservations that found their pass full and moved on
};

// One submitted frame's result.  Move-only; get() blocks until the pass carrying the frame has
// run and returns the sealed frame / opened message (nullopt as seal() / open()); the ticket is
// empty afterwards.  A ticket may outlive its queue.
class ENET_CXX_API FrameTicket {
public:
    struct State;
    FrameTicket() noexcept = default;
    explicit FrameTicket(State* s) noexcept : s_(s) {}
    FrameTicket(FrameTicket&& o) noexcept : s_(o.s_) { o.s_ = nullptr; }
    FrameTicket& operator=(FrameTicket&& o) noexcept;
    FrameTicket(const FrameTicket&) = delete;
    FrameTicket& operator=(const FrameTicket&) = delete;
    ~FrameTicket();
    bool valid() const noexcept { return s_ != nullptr; }
    bool ready() const noexcept;  // get() would not block
    std::optional<std::vector<std::uint8_t>> get();
    // The same into a caller-owned vector, keeping its capacity (a session's send / receive
    // buffer: no allocation per frame): true and `out` = the result, or false (nullopt above;
    // `out` cleared)
    bool get(std::vector<std::uint8_t>& out);
    // Zero-copy: blocks like get(); on success `out` views the result where it lies (the queue's
    // pinned pass, or the ticket's own buffer) and stays valid until release(), get() or the
    // ticket's destruction.  Hold a view briefly (a relay's socket write): its pass cannot be
    // reused meanwhile.  false where get() returns nullopt.  Release every view before the
    // queue is destroyed.
    bool view(std::span<const std::uint8_t>& out);
    void release() noexcept;  // ends the ticket and its view; the ticket is empty afterwards

private:
    State* s_ = nullptr;
};

// Send side: nonce(12) || BE32(|body|) || ChaCha20_{K,nonce,0}(m || HMAC_K(m)), the frame
// SessionManager::send writes (SessionManager.cpp:362-387).  Nonces: 12 random bytes per frame
// (the reference draws them from std::random_device, SessionManager.cpp:365-371; here from a
// per-thread ChaCha20 keystream keyed from std::random_device, re-keyed every 2^20 nonces).
class ENET_CXX_API FrameQueue {
public:
    static constexpr std::size_t kMaxPayloadSize = 1024 * 1024;  // SessionManager.cpp:87
    FrameQueue();
    explicit FrameQueue(FrameQueueOptions options);
    ~FrameQueue();
    FrameQueue(const FrameQueue&) = delete;
    FrameQueue& operator=(const FrameQueue&) = delete;

    // Seal one message for one session; blocks until done.  nullopt when the signed payload
    // (message + 32-byte MAC) exceeds kMaxPayloadSize, as SessionManager::send returns false
    // (:358-360).
    std::optional<std::vector<std::uint8_t>> seal(const std::array<std::uint8_t, 32>& session_key,
                                                  std::span<const std::uint8_t> message);
    // Non-blocking seal: the message is copied into the queue before this returns.
    FrameTicket submit(const std::array<std::uint8_t, 32>& session_key, std::span<const std::uint8_t> message);
    // DEPRECATED (ABI 1.2): the same as a std::future with std::launch::deferred -- get() / wait()
    // collect the result on the calling thread, but wait_for / wait_until return
    // std::future_status::deferred and never report readiness.  Before ABI 1.2 the future became
    // ready when its pass had run; a caller that polls futures must move to submit() and
    // FrameTicket::ready() / view() (a promise per frame cost ~0.45 us of CPU per frame, DESIGN.md
    // section 6).  Kept for source compatibility of get()-style callers.
    [[deprecated("poll with submit() + FrameTicket::ready(); the returned future is deferred")]]
    std::future<std::optional<std::vector<std::uint8_t>>> seal_async(const std::array<std::uint8_t, 32>& session_key,
                                                                      std::vector<std::uint8_t> message);
    // Explicit batching (a sender that collects frames itself): push queues a message (false =
    // too large, nothing queued), flush() seals every pushed message in one pass and returns the
    // wire frames in push order.  Thread-safe; independent of the queue above.
    bool push(const std::array<std::uint8_t, 32>& session_key, std::span<const std::uint8_t> message);
    std::size_t size() const;
    std::vector<std::vector<std::uint8_t>> flush();
    FrameQueueStats stats() const;

private:
    struct Impl;
    Impl* impl_;
};

// Receive side: the inverse for frames read off any session's socket (receive_loop :744-822 +
// decode_signed, Message.cpp:313-328): nullopt when the frame is shorter than its header, its
// BE32 length disagrees with the body or exceeds kMaxPayloadSize, the body is shorter than the
// MAC, or the HMAC does not verify; otherwise the message (the body minus its 32-byte MAC).
class ENET_CXX_API FrameReceiveQueue {
public:
    FrameReceiveQueue();
    explicit FrameReceiveQueue(FrameQueueOptions options);
    ~FrameReceiveQueue();
    FrameReceiveQueue(const FrameReceiveQueue&) = delete;
    FrameReceiveQueue& operator=(const FrameReceiveQueue&) = delete;

    std::optional<std::vector<std::uint8_t>> open(const std::array<std::uint8_t, 32>& session_key,
                                                  std::span<const std::uint8_t> frame);
    // Non-blocking open (see FrameQueue::submit / seal_async).
    FrameTicket submit(const std::array<std::uint8_t, 32>& session_key, std::span<const std::uint8_t> frame);
    // DEPRECATED (ABI 1.2): a deferred future, as FrameQueue::seal_async.
    [[deprecated("poll with submit() + FrameTicket::ready(); the returned future is deferred")]]
    std::future<std::optional<std::vector<std::uint8_t>>> open_async(const std::array<std::uint8_t, 32>& session_key,
                                                                     std::vector<std::uint8_t> frame);
    FrameQueueStats stats() const;

private:
    struct Impl;
    Impl* impl_;
};

// Proof of work.  Every PoW in the reference hashes
// SHA-256(prefix || BE64(nonce)) and takes the first nonce, in attempt order, with >= difficulty
// leading zero bits.  Node: compute_announce_pow / compute_handshake_pow (Node.cpp:212-230,
// 269-292; candidates start + attempt).  Store: security::compute_store_pow (StoreProof.cpp;
// successive mt19937_64 outputs) -- see also ephemeralnet/security/StoreProof.hpp.
enum class PowSchedule : int { Node = 0, Store = 1 };
struct PowResult {
    bool found{false};
    std::uint64_t nonce{0};
    std::uint64_t attempts{0};  // index of the nonce in attempt order (max_attempts if not found)
};
// difficulty[i] as given (no clamp; 0 -> nonce 0); one device pass for the whole batch
ENET_CXX_API std::vector<PowResult> pow_search(std::span<const std::span<const std::uint8_t>> prefixes,
                                               std::span<const std::uint8_t> difficulty,
                                               PowSchedule schedule, std::uint64_t max_attempts);
// announce_pow_valid / handshake_pow_valid / store_pow_valid without the clamp; 1 = valid
ENET_CXX_API std::vector<std::uint8_t> pow_check(std::span<const std::span<const std::uint8_t>> prefixes,
                                                 std::span<const std::uint64_t> nonces,
                                                 std::span<const std::uint8_t> difficulty);
// Node.cpp:155-171 (announce_pow_digest without the nonce): BE64-length-prefixed chunk_id,
// peer_id, endpoint, manifest_uri, assigned_shards, then BE64(ttl seconds)
ENET_CXX_API std::vector<std::uint8_t> announce_pow_prefix(const ChunkId& chunk_id, const PeerId& peer_id,
                                                           std::string_view endpoint,
                                                           std::string_view manifest_uri,
                                                           std::span<const std::uint8_t> assigned_shards,
                                                           std::int64_t ttl_seconds);
// Node.cpp:233-245 (handshake_pow_digest without the nonce)
ENET_CXX_API std::vector<std::uint8_t> handshake_pow_prefix(const PeerId& initiator, const PeerId& responder,
                                                            std::uint32_t initiator_public);

// Drop-ins for Node.cpp's file-local searches compute_announce_pow (Node.cpp:212-230) and
// compute_handshake_pow (:269-292): same start (mt19937_64 seeded by the nonce-0 digest), same
// attempt order and 500'000-attempt cap (Node.cpp:40,43), same nonce.  difficulty 0 -> nonce 0,
// true.  Not found -> false and nonce_out untouched.  One device search replaces up to 500'000
// host Sha256 constructions; a maintainer makes the Node.cpp helpers forward here.
// (kNodePowAttempts: above, beside announce_frames_seal.)
ENET_CXX_API bool compute_announce_pow(const ChunkId& chunk_id, const PeerId& peer_id, std::string_view endpoint,
                                       std::string_view manifest_uri,
                                       std::span<const std::uint8_t> assigned_shards, std::int64_t ttl_seconds,
                                       std::uint8_t difficulty, std::uint64_t& nonce_out);
ENET_CXX_API bool compute_handshake_pow(const PeerId& initiator, const PeerId& responder,
                                        std::uint32_t initiator_public, std::uint8_t difficulty,
                                        std::uint64_t& nonce_out);

// KeyManager::derive_key (KeyManager.cpp:74-92) for many sessions:
// HMAC-SHA256(secret_i, BE64(counter_i) || BE64(ticks_i)), ticks in ns since the steady_clock epoch
ENET_CXX_API std::vector<std::array<std::uint8_t, 32>> session_keys(std::span<const Key> secrets,
                                                                    std::span<const std::uint64_t> counters,
                                                                    std::span<const std::int64_t> ticks);

// KeyExchange::compute_public / derive_shared_secret (src/network/KeyExchange.cpp:22-48) for many
// keypairs in one device pass (enet_key_exchange_batch): publics[i] = 5^privates[i] mod 2^31-1 and,
// when `remotes` is not empty (then one per private), secrets[i] = derive_shared_secret(privates[i],
// remotes[i]).  std::invalid_argument for a size mismatch.
struct KeyExchangeResult {
    std::vector<std::uint32_t> publics;
    std::vector<Key> secrets;  // empty when no remotes were given
};
ENET_CXX_API KeyExchangeResult key_exchange(std::span<const std::uint32_t> privates,
                                            std::span<const std::uint32_t> remotes);

// The crypto of Node::perform_handshake (src/core/Node.cpp:1872-1926) for many peers in one device
// pass (enet_handshake_accept_batch on a table of requests.size() slots that lives for the call):
// per request, in the reference's order, KeyExchange::validate_public, handshake_pow_valid at
// `difficulty` (0 = no check: the initiator's side) with `local_id` as the responder, then
// derive_shared_secret(local_private, remote_public) and the session key
// HMAC(secret, make_handshake_material(local public, remote_public)).  An accepted result
// (verdict == HandshakeVerdict::Ok) feeds KeyManager unchanged:
//   register_session_with_material(peer_id, r.shared_secret, make_handshake_material(..), now)
// leaves current_key(peer_id) == r.session_key, which is also what
// SessionManager::register_peer_key takes.  A rejected result carries zero bytes.  Host-vector
// callers keep their own peer -> session maps, cooldowns and reputation: nothing is deduplicated
// here, and two requests of one peer are simply two results.  Device-resident callers use the C
// ABI's session table, where the keys never leave the device.
enum class HandshakeVerdict : std::uint8_t { BadPublic = 0, Ok = 1, BadPow = 2, BadSlot = 3 };
struct HandshakeRequest {
    PeerId peer_id{};
    std::uint32_t remote_public{0};
    std::uint64_t work_nonce{0};
};
struct HandshakeResult {
    HandshakeVerdict verdict{HandshakeVerdict::BadPublic};
    Key shared_secret{};
    std::array<std::uint8_t, 32> session_key{};
};
ENET_CXX_API std::vector<HandshakeResult> handshake_accept(const PeerId& local_id, std::uint32_t local_private,
                                                           std::uint8_t difficulty,
                                                           std::chrono::steady_clock::time_point now,
                                                           std::span<const HandshakeRequest> requests);

}  // namespace ephemeralnet::crypto::batch
