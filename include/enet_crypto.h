/*
 * enet_crypto.h -- C ABI of the MI355X bulk crypto engine for EphemeralNet.
 *
 * The reference crypto (ShardianLabs/EphemeralNet src/crypto) is a set of static C++20 member
 * functions taking one record per call.  This ABI is the batched, device-side
 * form of exactly those operations: every entry point below names the reference interface it
 * replaces (file:line).  The C++ API in include/ephemeralnet/crypto/ keeps the reference
 * signatures and is implemented on top of these calls (libenet_crypto.so exports both).
 *
 * Conventions
 *   - All buffer pointers are DEVICE pointers (hipMalloc'd, or any device-accessible memory)
 *     unless a comment says otherwise.  `stream` is a hipStream_t (NULL = legacy default).
 *   - Calls are asynchronous on `stream`; nothing is synchronised inside them (safe to capture in
 *     a hipGraph).  The caller keeps ownership of every buffer.  The one allocation: batches
 *     holding records of >= 256 KiB (ENET_SEG_MIN; enet_set_seg_min) take the sequence-parallel
 *     path, whose small scratch (a header, one entry per long record, one byte per record, 32 B
 *     per 64 KiB tile) is stream-ordered memory from a library-private pool
 *     (hipMallocFromPoolAsync / hipFreeAsync on `stream`).
 *   - Records are described SoA: a byte arena plus uint64 offsets[n+1]; record i is
 *     arena[offsets[i] .. offsets[i+1]).  Input and output arenas have their own offsets so
 *     length-changing ops (frames: +32-byte MAC) and in-place ops (out == in) both work.
 *   - keys / nonces / counters / tags / ok arrays must be 4-byte aligned.  Arena offsets may
 *     be arbitrary; 16-byte-aligned record starts run fastest.
 *   - Return 0 on success, a negative ENET_E* code otherwise.  Nothing throws across the ABI.
 *   - Thread-safe: calls on different streams may run concurrently from any host thread.
 */
#ifndef ENET_CRYPTO_H
#define ENET_CRYPTO_H

#include <stddef.h>
#include <stdint.h>

#ifndef ENET_API
#define ENET_API __attribute__((visibility("default")))
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define ENET_OK 0
#define ENET_EINVAL (-1)   /* bad argument (null pointer, misalignment, n too large) */
#define ENET_EHIP (-2)     /* a HIP runtime call or kernel launch failed */
#define ENET_ENODEV (-3)   /* no usable gfx950 device */
#define ENET_ENOMEM (-4)   /* allocation failed (host-side helpers only) */

/* A batch of independent records (SoA, device pointers). */
typedef struct enet_records {
    uint32_t count;             /* n records */
    const uint64_t* in_offsets; /* [n+1] byte offsets into `in` */
    const uint64_t* out_offsets;/* [n+1] byte offsets into `out` (may be == in_offsets) */
    const uint8_t* in;          /* input arena */
    uint8_t* out;               /* output arena (may be == in for in-place operation) */
    const uint8_t* keys;        /* [n][32] ChaCha20 keys, or [1][32] when key_stride == 0 */
    uint32_t key_stride;        /* 32 = per-record key (per-peer sessions), 0 = one shared key */
    const uint8_t* nonces;      /* [n][12] 96-bit nonces */
    const uint32_t* order;      /* optional [count] record indices to process, in this order
                                   (e.g. longest first, or one length class of a larger batch);
                                   NULL = 0..count-1.  Indices address offsets/keys/nonces/tags/ok
                                   of the full batch, so results stay position-indexed; an index
                                   may be >= count, and records the order does not name are left
                                   untouched.  With a subset the two hints below describe the
                                   NAMED records: their sum and their maximum. */
    uint64_t total_bytes_hint;  /* host-known sum of input lengths, 0 = unknown (scheduling) */
    uint32_t max_len_hint;      /* host-known max record length, 0 = unknown (scheduling) */
    /* The hints only choose kernels and launch shapes.  total == count * max declares a uniform
       batch (record i at in_offsets[0] + i * max); every workgroup of the uniform paths checks
       its records' real offsets against that layout and takes the per-lane path over the real
       offsets on any mismatch, so wrong hints cost speed, never bytes
       (tests/test_gpu_parity.py::test_lying_hints_give_correct_bytes). */
} enet_records;

/* ---- ChaCha20 (reference: ChaCha20::apply, src/crypto/ChaCha20.cpp:98-121,
 *      include/ephemeralnet/crypto/ChaCha20.hpp:20-24)
 * out_i = in_i XOR keystream(key_i, nonce_i, counters[i], counters[i]+1, ...) with the
 * reference's uint32 counter wrap (ChaCha20.cpp:110).  counters == NULL means all zero
 * (SessionManager.cpp:374/822 frames); CryptoManager passes LE32(chunk_id)
 * (CryptoManager.cpp:8-13, see enet_chunk_counter). */
ENET_API int enet_chacha20_xor_batch(const enet_records* r, const uint32_t* counters, void* stream);

/* ---- RFC 8439 AEAD_CHACHA20_POLY1305 (promised by the reference README.md:49, not
 *      implemented there -- SURVEY.md 0.1).  Keystream = ChaCha20::apply(counter = 1), one-time
 *      Poly1305 key = block(counter = 0).  aad/aad_offsets may be NULL (no AAD).
 * seal: out_i = ciphertext, tags[i] = 16-byte tag.
 * open: out_i = plaintext, ok[i] = 1 if the tag verified, else 0 and out_i is zeroed. */
ENET_API int enet_aead_seal_batch(const enet_records* r, const uint8_t* aad, const uint64_t* aad_offsets,
                         uint8_t* tags, void* stream);
ENET_API int enet_aead_open_batch(const enet_records* r, const uint8_t* aad, const uint64_t* aad_offsets,
                         const uint8_t* tags, uint8_t* ok, void* stream);

/* ---- SHA-256 (reference: Sha256::digest, src/crypto/Sha256.cpp:128-132)
 * digests[i] = SHA-256(in[offsets[i]..offsets[i+1])).  Used for chunk ids / manifest hashes
 * (StoreProof.cpp:75-78, Node.cpp:1414, Node.cpp:1652). */
ENET_API int enet_sha256_batch(uint32_t n, const uint8_t* in, const uint64_t* offsets, uint8_t* digests,
                      void* stream);

/* ---- HMAC-SHA256 (reference: HmacSha256::compute / verify, src/crypto/HmacSha256.cpp:11-54)
 * Key of record i = keys[key_offsets[i] .. key_offsets[i+1]) (keys over 64 B are hashed first,
 * HmacSha256.cpp:15-17); key_offsets == NULL means fixed 32-byte keys at keys + 32*i, or one
 * shared 32-byte key when key_stride == 0.
 * compute: macs[i] = HMAC(key_i, msg_i).
 * verify : ok[i] = (HMAC(key_i, msg_i) == macs[i]) (constant-time OR-accumulate, :47-53). */
ENET_API int enet_hmac_sha256_batch(uint32_t n, const uint8_t* keys, const uint64_t* key_offsets,
                           uint32_t key_stride, const uint8_t* in, const uint64_t* offsets,
                           uint8_t* macs, void* stream);
ENET_API int enet_hmac_sha256_verify_batch(uint32_t n, const uint8_t* keys, const uint64_t* key_offsets,
                                  uint32_t key_stride, const uint8_t* in,
                                  const uint64_t* offsets, const uint8_t* macs, uint8_t* ok,
                                  void* stream);

/* ---- Session frame body (reference: protocol::encode_signed, src/protocol/Message.cpp:305-311
 *      followed by SessionManager::send, src/network/SessionManager.cpp:362-374; CLI twin
 *      send_protocol_message, src/main.cpp:1141-1147).
 * seal: out_i = ChaCha20_{key_i, nonce_i, ctr 0}(in_i || HMAC-SHA256_{key_i}(in_i)),
 *       |out_i| = |in_i| + 32 (out_offsets must say so).  Keys are the 32-byte session keys.
 * open (SessionManager.cpp:815-822 then Message.cpp:313-328): out_i = first |in_i|-32 bytes of
 *       the decryption (out_offsets must say |in_i|-32, or 0 when |in_i| < 32), macs[i] = the
 *       decrypted 32-byte MAC ([n][32] device buffer), ok[i] = MAC verified (records shorter
 *       than 32 bytes fail, Message.cpp:315); on failure out_i is zeroed.  The 16-byte wire
 *       header nonce || BE32(len) (SessionManager.cpp:376-387) is host framing. */
/* One pass over HBM for any lengths / alignment / order (duplex kernel).  A record whose output
 * length is not as stated is not processed: its output range is zeroed (and ok[i] = 0). */
ENET_API int enet_frame_seal_batch(const enet_records* r, void* stream);
ENET_API int enet_frame_open_batch(const enet_records* r, uint8_t* macs, uint8_t* ok, void* stream);

/* ---- Whole wire frames (the batched session-frame codec): the frame body
 *      above plus the 16-byte header, in one pass -- what SessionManager::send puts on the socket
 *      (src/network/SessionManager.cpp:362-387) and what receive_loop takes off it (:760-822).
 * seal: in_i = encoded message m_i, out_i = nonce_i(12) || BE32(|m_i|+32) || ChaCha20_{key_i,
 *       nonce_i, 0}(m_i || HMAC_{key_i}(m_i)); out_offsets must give |out_i| = |m_i| + 48.
 * open: in_i = a received frame; the nonce comes from the frame (r->nonces is ignored, may be
 *       NULL); out_i = m_i (out_offsets must give |in_i| - 48), macs/ok as frame_open.  ok[i] = 0
 *       also when the frame is shorter than 48 bytes or its length field differs from its body
 *       length; failed messages are zeroed. */
ENET_API int enet_wire_seal_batch(const enet_records* r, void* stream);
ENET_API int enet_wire_open_batch(const enet_records* r, uint8_t* macs, uint8_t* ok, void* stream);
/* Session-keyed frame batches (a relay's frames come from fewer sessions than
 * frames).  keys = the sessions' 32-byte keys as a table ([sessions][32], key_stride ignored),
 * session[i] = the session of frame i, mid = the table's HMAC midstates from
 * enet_hmac_midstates ([sessions][16] uint32).  Same bytes as enet_wire_seal_batch /
 * enet_wire_open_batch with keys[i] = table[session[i]]; every frame skips the two key-block
 * compressions of its HMAC (2 of 27 for a 1 500-byte message).  A session[i] >= sessions
 * (device-resident, so not checked on the host) never reads past the table and fails closed:
 * seal zeroes that frame's whole output slot (nothing is encrypted under another session's key),
 * open reports ok[i] = 0 and zeroes the message.  enet_hmac_midstates: for each of
 * n keys the SHA-256 states after (key || 0^32) ^ ipad and ^ opad (HmacSha256.cpp:11-39). */
ENET_API int enet_hmac_midstates(const uint8_t* keys, uint32_t n, uint32_t* mid, void* stream);
ENET_API int enet_wire_seal_batch_sessions(const enet_records* r, const uint32_t* session,
                                           uint32_t sessions, const uint32_t* mid, void* stream);
ENET_API int enet_wire_open_batch_sessions(const enet_records* r, const uint32_t* session,
                                           uint32_t sessions, const uint32_t* mid, uint8_t* macs,
                                           uint8_t* ok, void* stream);

/* ---- AEAD with a fused HMAC-SHA256 integrity tag ("AEAD plus fused
 *      HMAC-SHA256 tag and verify"): ONE pass over HBM per direction (duplex kernel: Poly1305
 *      in the cipher lanes, HMAC in the hash lanes on the same SIMDs).  in/out offsets
 *      equal-length; mixed lengths are balanced best with `order` = longest first.  The HMAC covers the plaintext under the record's 32-byte
 *      key, exactly what the reference signs before encrypting (encode_signed,
 *      src/protocol/Message.cpp:305-311, HmacSha256.cpp:11-39).
 * seal: out_i = ChaCha20-Poly1305 ciphertext, tags[i] = Poly1305 tag, macs[i] = HMAC_K(pt_i).
 * open: out_i = plaintext, ok[i] = Poly1305 tag verified AND HMAC verified (HmacSha256.cpp:41-54);
 *       on failure out_i is zeroed. */
ENET_API int enet_aead_hmac_seal_batch(const enet_records* r, uint8_t* tags, uint8_t* macs,
                                       void* stream);
ENET_API int enet_aead_hmac_open_batch(const enet_records* r, const uint8_t* tags,
                                       const uint8_t* macs, uint8_t* ok, void* stream);

/* ---- Chunk store / fetch pipeline (Node::store_chunk, src/core/Node.cpp:1414-1417,
 *      Node::fetch_chunk's decrypt + hash check, :1641-1655).  in/out offsets equal-length.
 * store: chunk_hashes[i] (device [n][32], 4-byte aligned) = SHA-256(in_i) -- the manifest
 *        chunk_hash, and derive_chunk_id (src/security/StoreProof.cpp:75-78);
 *        out_i = ChaCha20(key_i, nonce_i, LE32(chunk_id_i[0..3]), in_i) (encrypt_with_key,
 *        CryptoManager.cpp:38-46) where chunk_id_i = chunk_ids[i], or the fresh chunk_hashes[i]
 *        when chunk_ids == NULL (the daemon derives ids from content, ControlServer.cpp:1101).
 * fetch: out_i = ChaCha20(key_i, nonce_i, LE32(chunk_ids[i][0..3]), in_i); ok[i] =
 *        SHA-256(out_i) == chunk_hashes[i]; on mismatch out_i is zeroed (no plaintext).
 * With chunk_ids given: one pass over HBM (hash and cipher together) for any lengths;
 * content-derived ids need the digest first (two passes).  Long chunks (a stored file is one chunk
 * of up to 32 MiB, Config.hpp:62) hash on host threads while the device ciphers them across every
 * CU: see enet_set_host_hash_min -- such a call is synchronous. */
ENET_API int enet_chunk_store_batch(const enet_records* r, const uint8_t* chunk_ids,
                                    uint8_t* chunk_hashes, void* stream);
ENET_API int enet_chunk_fetch_batch(const enet_records* r, const uint8_t* chunk_ids,
                                    const uint8_t* chunk_hashes, uint8_t* ok, void* stream);

/* ---- Chunk transfer frames: a stored chunk onto the wire and off it in one pass each
 *      (additive to ABI 1.4: enet_abi_version() is unchanged, no existing call changes).
 * Upload (Node::dispatch_upload, src/core/Node.cpp:1254-1297) wraps the stored ciphertext in a
 * `Chunk` message (encode, src/protocol/Message.cpp:204-246; every version 1..4 writes the same
 * 42-byte header), signs it (encode_signed, Message.cpp:305-311) and sends it as a session frame
 * (SessionManager::send, src/network/SessionManager.cpp:362-387):
 *   m_i     = version || 0x03 || BE32(ttl_i) || BE32(|data_i|) || chunk_id_i(32) || data_i
 *   frame_i = nonce_i(12) || BE32(|m_i| + 32) || ChaCha20_{Ks_i, nonce_i, 0}(m_i || HMAC_{Ks_i}(m_i))
 *   data_i  = ChaCha20_{Kc_i, Nc_i, LE32(chunk_id_i[0..3])}(plaintext_i)   (enet_chunk_store_batch)
 * The receiver (receive_loop, SessionManager.cpp:760-822; decode_signed, Message.cpp:313-328;
 * decode, Message.cpp:144-159; Node::handle_chunk -> receive_chunk, Node.cpp:2286-2299,
 * 1615-1677) decrypts the frame, checks the HMAC, parses the header, decrypts data under the
 * chunk key, compares SHA-256(plaintext) with manifest.chunk_hash, stores the ciphertext
 * (chunk_store_.put, Node.cpp:1665) and returns the plaintext.
 * Session keys for both calls: session != NULL -- r->keys is the [sessions][32] table, session[i]
 * the frame's session and mid the table's enet_hmac_midstates, as in enet_wire_*_batch_sessions;
 * session == NULL -- r->keys / r->key_stride give each record's key as in enet_wire_seal_batch
 * (sessions and mid are ignored).  order, total_bytes_hint and max_len_hint keep their
 * enet_records meaning (hints cost speed, never bytes).  All array arguments are device pointers
 * ([n] entries, indexed by record): chunk_keys may be the output of enet_shamir_combine_batch.
 * seal: in_i = data_i, read in place at any alignment; out_i = frame_i, out_offsets must give
 *       |out_i| = |data_i| + 90 (16 + 42 + 32); r->nonces = the frame nonces; chunk_ids [n][32];
 *       ttl [n] uint32 seconds; versions [n] uint8, NULL = 4, clamped to 1..4 (clamp_version,
 *       Message.cpp:17-25).  Same bytes as enet_wire_seal_batch[_sessions] over m_i.  A record
 *       whose output length does not fit or whose session index is outside the table has its
 *       whole output slot zeroed.
 * open: in_i = a received frame (the nonce is read from it; r->nonces is ignored, may be NULL);
 *       chunk_ids / chunk_keys / chunk_nonces / chunk_hashes [n][32|32|12|32] = what the caller's
 *       manifest expects; out_i = plaintext_i, out_offsets must give |in_i| - 90 (0 for a frame
 *       shorter than 90 bytes); data_out (nullable; same out_offsets) = data_i; ttl_out [n]
 *       uint32 (nullable); status [n] uint8 = the first check that failed:
 *         0 ENET_CF_OK
 *         1 ENET_CF_FRAME     frame shorter than 48 bytes, length field != body length, HMAC
 *                             mismatch, session index outside the table, or the output length
 *                             does not fit (what gives enet_wire_open_batch ok = 0)
 *         2 ENET_CF_HEADER    |m| < 42, version outside 1..4, type != 0x03, or BE32 data length
 *                             != |m| - 42
 *         3 ENET_CF_CHUNK_ID  the message's chunk id != chunk_ids[i]
 *         4 ENET_CF_HASH      SHA-256(plaintext_i) != chunk_hashes[i]
 *       On any non-zero status the record's plaintext range, its data_out range and ttl_out[i]
 *       are zero when the call returns.  Records `order` does not name are untouched.
 *       One deliberate difference: decode accepts a Chunk message with bytes after data (its only
 *       length check is remaining < expected, Message.cpp:151); this call reports
 *       ENET_CF_HEADER for such a frame (encode never produces one) and the caller falls back to
 *       enet_wire_open_batch_sessions.
 * One launch each; open reads every frame byte from HBM once and runs both ciphers and both
 * hashes of a record concurrently (three lanes per record).  Frames are at most 1 MiB
 * (SessionManager.cpp:87).  NULL r, status, chunk_ids, chunk_keys, chunk_nonces or chunk_hashes:
 * ENET_EINVAL. */
enum { ENET_CF_OK = 0, ENET_CF_FRAME = 1, ENET_CF_HEADER = 2, ENET_CF_CHUNK_ID = 3, ENET_CF_HASH = 4 };
ENET_API int enet_chunk_frame_seal_batch(const enet_records* r, const uint32_t* session, uint32_t sessions,
                                         const uint32_t* mid, const uint8_t* chunk_ids, const uint32_t* ttl,
                                         const uint8_t* versions, void* stream);
ENET_API int enet_chunk_frame_open_batch(const enet_records* r, const uint32_t* session, uint32_t sessions,
                                         const uint32_t* mid, const uint8_t* chunk_ids,
                                         const uint8_t* chunk_keys, const uint8_t* chunk_nonces,
                                         const uint8_t* chunk_hashes, uint8_t* data_out, uint32_t* ttl_out,
                                         uint8_t* status, void* stream);

/* ---- proof of work
 * Every PoW in the reference hashes SHA-256(prefix || BE64(candidate)) and accepts the FIRST
 * candidate, in attempt order, whose digest has >= difficulty leading zero bits:
 *   ENET_POW_NODE  (0): compute_announce_pow / compute_handshake_pow (src/core/Node.cpp:212-230,
 *                       269-292): candidate(a) = start + a, start = first std::mt19937_64 output
 *                       seeded with BE64(SHA-256(prefix || BE64(0))[0..8]) (:200-209, :247-256);
 *   ENET_POW_STORE (1): security::compute_store_pow (src/security/StoreProof.cpp:124-146):
 *                       candidate(a) = a-th std::mt19937_64 output seeded with
 *                       LE64(SHA-256(prefix || BE64(0))[0..8]).
 * Prefix serialisations: StoreProof.cpp:39-52 (chunk_id || BE64 size || BE32 len || hint) and
 * Node.cpp:155-171 / 233-245 (BE64-length-prefixed fields); see crypto::batch::*_pow_prefix.
 * prefixes/prefix_offsets: arena + [n+1] offsets; difficulty: [n] bits (0 -> nonce 0, found;
 * callers clamp as the reference does, StoreProof.cpp:128-130).  Outputs: nonces [n],
 * attempts [n] (nullable: index of the nonce in attempt order, or max_attempts), found [n]. */
#define ENET_POW_NODE 0
#define ENET_POW_STORE 1
ENET_API int enet_pow_search_batch(uint32_t n, const uint8_t* prefixes,
                                   const uint64_t* prefix_offsets, const uint8_t* difficulty,
                                   int schedule, uint64_t max_attempts, uint64_t* nonces,
                                   uint64_t* attempts, uint8_t* found, void* stream);
/* store_pow_valid / announce_pow_valid / handshake_pow_valid (StoreProof.cpp:109-121,
 * Node.cpp:193-198, 247-255) without the clamp: ok[i] = lzb(SHA-256(prefix_i || BE64(nonces[i])))
 * >= difficulty[i] (difficulty 0 -> 1). */
ENET_API int enet_pow_check_batch(uint32_t n, const uint8_t* prefixes,
                                  const uint64_t* prefix_offsets, const uint64_t* nonces,
                                  const uint8_t* difficulty, uint8_t* ok, void* stream);

/* ---- announce frames: batched PoW + seal, and one-pass admission
 * The gossip of a manifest is an `Announce` message per assigned peer and endpoint
 * (Node::broadcast_manifest -> deliver_manifest, src/core/Node.cpp:2512-2661): a proof-of-work
 * search (compute_announce_pow, :212-230), encode + encode_signed (src/protocol/Message.cpp:215-235,
 * 305-311) and the session frame.  With E, U, A the lengths of endpoint, manifest URI and assigned
 * shards and v the version after clamp_version (1..4):
 *   m_i     = v || 0x01 || BE32(ttl) || BE32(E) || BE32(U) || BE32(A) || chunk_id(32) || peer_id(32)
 *             || endpoint || uri || shards || [BE64(work_nonce) only when v == 4]
 *   frame_i = nonce_i(12) || BE32(|m_i| + 32) || ChaCha20_{Ks_i, nonce_i, 0}(m_i || HMAC_{Ks_i}(m_i))
 *   pow_i   = SHA-256(BE64(32) || chunk_id || BE64(32) || peer_id || BE64(E) || endpoint || BE64(U)
 *             || uri || BE64(A) || shards || BE64(ttl) || BE64(work_nonce))        (Node.cpp:155-173)
 * The receiver (handle_transport_message -> decode_signed -> handle_announce, Node.cpp:2160-2179,
 * 2332-2357) opens the frame, checks the HMAC, parses m, then checks peer_id == sender, a non-empty
 * URI and announce_pow_valid (:193-198, :1144-1151).  Two quirks of the reference are kept: encode
 * writes the nonce only for v == 4 but decode expects it for v >= 3 (Message.cpp:221, 284), so a
 * v3 announce made by encode never decodes; v1 / v2 carry no nonce and fail the PoW check whenever
 * difficulty > 0.
 * Session keys for both calls: as in enet_chunk_frame_*_batch (session != NULL: r->keys is the
 * table, mid its midstates; session == NULL: per-record keys).  count, out / out_offsets, order
 * and the hints keep their enet_records meaning.  All arrays are device pointers.
 * seal: r->in / r->in_offsets are ignored; r->nonces = the frame nonces; out_i = frame_i,
 *       out_offsets must give |out_i| = |m_i| + 48.  The fields come through index tables because
 *       one manifest goes to many peers: record i takes chunk id and URI of manifest
 *       f->manifest[i], the endpoint f->endpoint[i] (NULL tables: i), its own shard list and ttl;
 *       f->peer_id is the local id; ttl is uint32 because that is all the wire carries (the
 *       receiver's digest sees the truncated value).  Neither m nor the PoW prefix is written to
 *       device memory.  At most two launches, no synchronisation, no allocation, no scratch:
 *       the search (one workgroup per record, first-found order, ENET_POW_NODE schedule) runs only
 *       when difficulty > 0 and max_attempts > 0, and only for v == 4 records; v < 4 records are
 *       sealed as encode writes them, without a nonce (work_nonce[i] = 0) -- deliver_manifest's
 *       "difficulty > 0 needs v >= 3" guard (Node.cpp:2639) stays with the caller.  difficulty ==
 *       0: nonce 0, as compute_announce_pow.  max_attempts == 0: work_nonce[] is INPUT (a search
 *       done earlier), nothing is searched, whatever the difficulty.  work_nonce [n] (8-byte
 *       aligned) otherwise receives the nonces.  status [n]:
 *         0 ENET_AF_OK
 *         1 ENET_AF_FRAME   the output length does not fit, or a session / manifest / endpoint
 *                           index is outside its table (or a field's offsets decrease)
 *         5 ENET_AF_POW     no nonce within max_attempts
 *       On a non-zero status the record's whole output slot is zero and work_nonce[i] = 0.
 * open: in_i = a received frame (the nonce is read from it; r->nonces may be NULL); peer_ids
 *       [n][32] = the peer of each frame's session; out_i = m_i, out_offsets must give |in_i| - 48
 *       (0 for shorter frames); info [n][8] uint32 (4-byte aligned) = {v, ttl, E, U, A, nonce low,
 *       nonce high, 0}: the fields lie in out_i at 82, 82 + E and 82 + E + U.  status [n] = the
 *       first check that failed, in the reference's order:
 *         0 ENET_AF_OK
 *         1 ENET_AF_FRAME        what gives enet_wire_open_batch ok = 0: frame < 48 bytes, length
 *                                field != body length, HMAC mismatch, session index outside the
 *                                table, or the output length does not fit
 *         2 ENET_AF_HEADER       version outside 1..4, type != 0x01, or |m| != 82 + E + U + A
 *                                (+ 8 if v >= 3), summed in 64 bits (parse_announce_payload,
 *                                Message.cpp:75-121)
 *         3 ENET_AF_SENDER       the message's peer_id != peer_ids[i] (Node.cpp:2341)
 *         4 ENET_AF_NO_MANIFEST  U == 0 (:2347)
 *         5 ENET_AF_POW          difficulty > 0 and (v < 3 or leading zero bits of pow < difficulty)
 *       On any non-zero status the record's out range and info[i] are zero when the call returns.
 *       Records `order` does not name are untouched.  One deliberate difference, as for Chunk
 *       frames: decode accepts bytes after the payload (remaining < expected_size is its only
 *       length check), this call reports ENET_AF_HEADER and the caller falls back to
 *       enet_wire_open_batch_sessions.
 *       One launch; every frame byte is read from HBM once (cipher, mac and pow lane per record).
 * ENET_EINVAL, with nothing launched: NULL r, f, status, work_nonce / info, peer_ids or a NULL
 * required table of f; difficulty > 255; misaligned info / work_nonce / ttl / index tables.
 * count == 0 is a no-op whatever else is passed. */
enum { ENET_AF_OK = 0, ENET_AF_FRAME = 1, ENET_AF_HEADER = 2, ENET_AF_SENDER = 3, ENET_AF_NO_MANIFEST = 4,
       ENET_AF_POW = 5 };
typedef struct enet_announce_fields {
    uint32_t manifests;               /* M */
    const uint8_t* chunk_ids;         /* [M][32] */
    const uint8_t* uris;              /* URI arena */
    const uint64_t* uri_offsets;      /* [M+1] */
    const uint32_t* manifest;         /* [n] index into the M manifests, NULL: i */
    uint32_t endpoints;               /* Ep */
    const uint8_t* endpoint_bytes;    /* endpoint arena */
    const uint64_t* endpoint_offsets; /* [Ep+1] */
    const uint32_t* endpoint;         /* [n] index into the Ep endpoints, NULL: i */
    const uint8_t* shards;            /* assigned-shard arena, per record */
    const uint64_t* shard_offsets;    /* [n+1] */
    const uint8_t* peer_id;           /* [32] the local id */
    const uint32_t* ttl;              /* [n] seconds */
    const uint8_t* versions;          /* [n], NULL = 4, clamped to 1..4 */
} enet_announce_fields;
ENET_API int enet_announce_frame_seal_batch(const enet_records* r, const uint32_t* session, uint32_t sessions,
                                            const uint32_t* mid, const enet_announce_fields* f,
                                            uint32_t difficulty, uint64_t max_attempts, uint64_t* work_nonce,
                                            uint8_t* status, void* stream);
ENET_API int enet_announce_frame_open_batch(const enet_records* r, const uint32_t* session, uint32_t sessions,
                                            const uint32_t* mid, const uint8_t* peer_ids, uint32_t difficulty,
                                            uint32_t* info, uint8_t* status, void* stream);

/* ---- Request / Acknowledge frames and receive-side frame triage
 *      (additive: enet_abi_version() is unchanged, no existing call changes).
 * A chunk transfer opens with a `Request` (Node::request_chunk, src/core/Node.cpp:1748-1756;
 * send_chunk_request_direct, :532-550) and closes with an `Acknowledge` (handle_chunk, :2305-2317;
 * send_negative_ack, :930-949).  With v = clamp_version(version) (src/protocol/Message.cpp:17-25;
 * encode, :236-252; payloads, :134-143 and :160-170; encode_signed, :305-311; SessionManager::send,
 * src/network/SessionManager.cpp:362-387):
 *   Request      m = v || 0x02 || chunk_id(32) || requester(32)                |m| = 66
 *   Acknowledge  m = v || 0x04 || accepted(1) || chunk_id(32) || peer_id(32)   |m| = 67
 *   frame = nonce(12) || BE32(|m| + 32) || ChaCha20_{Ks,nonce,0}(m || HMAC_Ks(m))   114 / 115 bytes
 * Session keys for all three calls: as in enet_chunk_frame_*_batch (session != NULL: r->keys is the
 * [sessions][32] table and mid its enet_hmac_midstates; session == NULL: per-record keys through
 * r->keys / r->key_stride, the HMAC pads computed per record).  count, order and the hints keep
 * their enet_records meaning.  All arrays are device pointers, [n] entries indexed by record; the
 * 32-byte id tables, info, lists and counts are 4-byte aligned.
 * seal: r->in / r->in_offsets are ignored; r->nonces = the frame nonces; out_i = frame_i and
 *       out_offsets must give |out_i| = 114 (Request) or 115 (Acknowledge).  kinds [n] uint8 =
 *       ENET_CTL_REQUEST / ENET_CTL_ACK; chunk_ids [n][32]; peer_id [32] = the local id (the
 *       requester of a Request, the peer_id of an Acknowledge); versions [n] uint8, NULL = 4,
 *       clamped to 1..4; accepted [n] uint8 (nullable, Acknowledge records only): NULL = 0
 *       (send_negative_ack); accept_zero == 0: the wire byte is accepted[i] != 0; accept_zero != 0:
 *       it is accepted[i] == 0, so the status[] of enet_chunk_frame_open_batch can be passed as it
 *       is (handle_chunk's accepted = plaintext.has_value(), Node.cpp:2305-2317).  status [n]:
 *         0 ENET_CT_OK
 *         1 ENET_CT_FRAME   the output length does not fit, or the session index is outside the table
 *         2 ENET_CT_HEADER  the kind is not 2 or 4 (checked first: no kind, no length to fit)
 *       On a non-zero status the record's whole output slot is zero.  One launch, no allocation, no
 *       synchronisation; m never exists in device memory.
 * open: in_i = a received frame (the nonce is read from it; r->nonces may be NULL); r->out /
 *       r->out_offsets are ignored and may be NULL.  Outputs are SoA: chunk_ids_out [n][32],
 *       peer_ids_out [n][32] (nullable; the requester / peer_id field), info [n][4] uint8 = {v, type,
 *       accepted, sender_match}: accepted = the wire byte != 0 (Message.cpp:160-170), 0 for a
 *       Request; sender_match = 1 when sender_ids ([n][32], nullable: the peer of each frame's
 *       session) is given and equals the message's requester / peer_id, else 0 -- reported, not
 *       enforced, because the reference acts on the transport's sender and never reads the
 *       payload's id (handle_request, Node.cpp:2255-2284; handle_acknowledge, :2320-2330).
 *       status [n] = the first failed check:
 *         0 ENET_CT_OK
 *         1 ENET_CT_FRAME   what gives enet_wire_open_batch ok = 0: frame < 48 bytes, length field
 *                           != body length, HMAC mismatch, session index outside the table
 *         2 ENET_CT_HEADER  version outside 1..4, type not 2 or 4, or |m| != 66 (Request) / 67
 *                           (Acknowledge)
 *       On a non-zero status the record's chunk id, peer id and info are zero.  Records `order` does
 *       not name are untouched.  One deliberate difference, as for Chunk and Announce frames:
 *       decode accepts trailing bytes (remaining < needed is its only check, Message.cpp:134-143,
 *       160-170); this call reports ENET_CT_HEADER and the caller falls back to
 *       enet_wire_open_batch_sessions.  One launch; every frame byte is read from HBM once.
 * classify: in_i = a received frame of unknown type; no mid is needed and nothing is authenticated:
 *       one ChaCha20 block (counter 0), the 16 header bytes and the first 2 body bytes per frame.
 *       kind [n] uint8:
 *         0 ENET_FK_BAD       L < 48, BE32(frame[12..16)) != L - 16 (SessionManager.cpp:770-796), or
 *                             the session index is outside the table: what every open call rejects
 *                             as FRAME without looking at the body
 *         1 ENET_FK_ANNOUNCE  v in 1..4, type 1, |m| = L - 48 >= 82 + (v >= 3 ? 8 : 0) (Message.cpp:75-121)
 *         2 ENET_FK_REQUEST   v in 1..4, type 2, |m| == 66
 *         3 ENET_FK_CHUNK     v in 1..4, type 3, |m| >= 42 (Message.cpp:144-159)
 *         4 ENET_FK_ACK       v in 1..4, type 4, |m| == 67
 *         5 ENET_FK_OTHER     everything else (types 5 and 6, other versions, |m| < 2, a length that
 *                             does not fit its class): for enet_wire_open_batch_sessions
 *       lists [5][n] uint32 (n = r->count) and counts [5] uint32: row k - 1 holds the indices of the
 *       frames of kind k, each index exactly once, BAD frames in no row; ascending inside each
 *       256-record block of the batch, the blocks in any order.  The call zeroes counts on the
 *       stream itself.  The host reads counts (20 bytes) and passes lists + (k - 1) * n as `order`
 *       and counts[k - 1] as `count` to the matching open on the same stream.
 *       PROPERTY: a frame for which enet_announce_frame_open_batch, enet_chunk_frame_open_batch or
 *       enet_control_frame_open_batch would return status 0 is always classified into that call's
 *       class -- every class test is implied by the open's own header check, so triage never costs
 *       a frame its fast path.  The reverse does not hold: a forged frame may land in a class and
 *       then get FRAME or HEADER from the open.
 * ENET_EINVAL, with nothing launched: NULL r, kinds, chunk_ids, peer_id, status, chunk_ids_out,
 * info, kind, lists or counts; misaligned id tables, info, lists or counts; the session / mid rules
 * of the chunk frames.  count == 0 is a no-op whatever else is passed. */
enum { ENET_CTL_REQUEST = 2, ENET_CTL_ACK = 4 };
enum { ENET_CT_OK = 0, ENET_CT_FRAME = 1, ENET_CT_HEADER = 2 };
enum { ENET_FK_BAD = 0, ENET_FK_ANNOUNCE = 1, ENET_FK_REQUEST = 2, ENET_FK_CHUNK = 3, ENET_FK_ACK = 4,
       ENET_FK_OTHER = 5 };
ENET_API int enet_control_frame_seal_batch(const enet_records* r, const uint32_t* session, uint32_t sessions,
                                           const uint32_t* mid, const uint8_t* kinds, const uint8_t* chunk_ids,
                                           const uint8_t* peer_id, const uint8_t* accepted, int accept_zero,
                                           const uint8_t* versions, uint8_t* status, void* stream);
ENET_API int enet_control_frame_open_batch(const enet_records* r, const uint32_t* session, uint32_t sessions,
                                           const uint32_t* mid, const uint8_t* sender_ids, uint8_t* chunk_ids_out,
                                           uint8_t* peer_ids_out, uint8_t* info, uint8_t* status, void* stream);
ENET_API int enet_frame_classify_batch(const enet_records* r, const uint32_t* session, uint32_t sessions,
                                       uint8_t* kind, uint32_t* lists, uint32_t* counts, void* stream);

/* ---- session key derivation
 * network::KeyManager::derive_key (src/network/KeyManager.cpp:74-92) for n sessions:
 * keys_out[i] = HMAC-SHA256(secrets[i], BE64(counters[i]) || BE64(ticks[i])), ticks = the
 * rotation time in ns since the steady_clock epoch (register_session uses counter 0, :15-30). */
ENET_API int enet_session_key_batch(uint32_t n, const uint8_t* secrets, const uint64_t* counters,
                                    const int64_t* ticks, uint8_t* keys_out, void* stream);

/* ---- Shamir key shares (reference: Shamir::split / Shamir::combine, src/crypto/Shamir.cpp:114-163,
 *      include/ephemeralnet/crypto/Shamir.hpp:12-25): the 32-byte chunk key is split when a chunk
 *      is stored (Node::store_chunk, src/core/Node.cpp:1428) and combined before it is decrypted
 *      (Node::receive_chunk / fetch_chunk, :1632-1642, :1804-1813; src/main.cpp:816-825).  Byte by
 *      byte over GF(2^8) with the reference's field -- reduction polynomial 0x11D, generator 2
 *      (Shamir.cpp:10-26), not the AES field -- multiplied without tables (the reference indexes
 *      log / exp tables by key bytes, :41-49).  `threshold` is uniform per call (the node's
 *      config value); callers group by threshold.
 * split:   shares [n][share_count][32], share j of record i has index j + 1 and is the record's
 *          polynomial at x = j + 1 (evaluate_polynomial, :68-80): constant term secrets[i] ([n][32]),
 *          degree-d coefficient (d = 1 .. threshold-1) the 32 caller-supplied random bytes at
 *          coeffs + ((i * (threshold-1) + d-1) * 32) -- the reference draws them from
 *          std::random_device (:127,141).  coeffs may be NULL when threshold == 1.
 * combine: Lagrange interpolation at 0 (interpolate, :82-110) over the FIRST `threshold` shares of
 *          each record in the caller's order, as the reference takes them (:161): indices
 *          [n][threshold], values [n][threshold][32]; secrets_out [n][32] is directly usable as
 *          enet_records.keys (key_stride 32) by a later call on the same stream; ok [n].  An index
 *          of 0 is legal (the share at x = 0 is the secret).  Two equal indices among a record's
 *          first `threshold` give ok[i] = 0 and 32 zero bytes (fail closed, as every open here).
 *          That is deliberately stricter than the reference in one corner: it throws "division by
 *          zero" there (:54-56) only if a value byte it would multiply is non-zero (:90-92), and
 *          returns a secret for duplicate all-zero shares.
 * secrets, coeffs, shares, values and secrets_out must be 4-byte aligned.  ENET_EINVAL (nothing
 * launched) unless 1 <= threshold <= share_count <= 255 (combine: threshold <= 255). */
ENET_API int enet_shamir_split_batch(uint32_t n, const uint8_t* secrets, const uint8_t* coeffs,
                                     uint32_t threshold, uint32_t share_count, uint8_t* shares,
                                     void* stream);
ENET_API int enet_shamir_combine_batch(uint32_t n, uint32_t threshold, const uint8_t* indices,
                                       const uint8_t* values, uint8_t* secrets_out, uint8_t* ok,
                                       void* stream);

/* ---- device session table: batched handshake admission and key rotation
 *      (additive to ABI 1.4: enet_abi_version() is unchanged, no existing call changes)
 * The crypto of Node::perform_handshake (src/core/Node.cpp:1872-1926) for many peers at once, and
 * KeyManager's rotation, with the session keys born and rotated in device memory: `keys` and `mid`
 * of the table are exactly the keys table and the enet_hmac_midstates of
 * enet_wire_seal_batch_sessions / enet_wire_open_batch_sessions (session index = slot), so a
 * later call on the same stream uses an admitted or rotated key with no upload and no midstate
 * pass.  All table arrays are device memory owned by the caller; secrets, keys and mid must be
 * 4-byte aligned, counters and last_rotation 8-byte aligned.  last_rotation is in ns since the
 * steady_clock epoch (the ticks of enet_session_key_batch). */
typedef struct enet_session_table {
    uint32_t sessions;       /* S */
    uint8_t* secrets;        /* [S][32] shared secrets (KeyExchange::derive_shared_secret) */
    uint8_t* keys;           /* [S][32] current session keys */
    uint32_t* mid;           /* [S][16] == enet_hmac_midstates(keys) */
    uint64_t* counters;      /* [S] rotation counters */
    int64_t* last_rotation;  /* [S] */
    uint8_t* live;           /* [S] 1 = the slot holds a session */
} enet_session_table;
enum { ENET_HS_BAD_PUBLIC = 0, ENET_HS_OK = 1, ENET_HS_BAD_POW = 2, ENET_HS_BAD_SLOT = 3 };
/* Record i, in the reference's order:
 *   1. KeyExchange::validate_public(remote_public[i]) (1 < c < 2^31-1), else ENET_HS_BAD_PUBLIC;
 *   2. when difficulty != 0, handshake_pow_valid (Node.cpp:232-256): leading zero bits of
 *      SHA-256(BE64(32) || peer_ids[i] || BE64(32) || local_id || BE64(remote_public[i]) ||
 *      BE64(work_nonce[i])) >= difficulty, else ENET_HS_BAD_POW.  difficulty == 0 skips the check
 *      (work_nonce and peer_ids may then be NULL); it is also the initiator's side, which admits
 *      the responder without a proof;
 *   3. slot[i] (NULL: i) < sessions, else ENET_HS_BAD_SLOT;
 *   4. secret = derive_shared_secret(local_private, remote_public[i]) (KeyExchange.cpp:34-48),
 *      key = HMAC-SHA256(secret, BE32(min(local_public, remote)) || BE32(max(..)))
 *      (make_handshake_material, Node.cpp:61-75; register_session_with_material,
 *      KeyManager.cpp:32-46), and the slot becomes {secret, key, midstates of key, counter 0,
 *      last_rotation now_ticks, live 1}; verdict[i] = ENET_HS_OK.
 * A rejected record writes its verdict only: its slot stays byte for byte as it was.
 * Caller contract: the slots of one batch are distinct (two records of one batch never name the
 * same slot); a slot that is already live is replaced, as contexts_[peer] = context does.
 * peer_ids [n][32] and local_id [32] must be 4-byte aligned.  ENET_EINVAL (nothing launched) for
 * a NULL required buffer, a misaligned one, difficulty > 255, or difficulty != 0 without
 * work_nonce / peer_ids.  n == 0 is a no-op. */
ENET_API int enet_handshake_accept_batch(const enet_session_table* t, uint32_t n, const uint8_t* peer_ids,
                                         const uint32_t* remote_public, const uint64_t* work_nonce,
                                         const uint32_t* slot, const uint8_t* local_id, uint32_t local_private,
                                         uint32_t local_public, uint32_t difficulty, int64_t now_ticks,
                                         uint8_t* verdict, void* stream);
/* KeyManager::rotate_if_needed + derive_key (KeyManager.cpp:56-92) over the whole table: slot s
 * with live[s] != 0 and now_ticks - last_rotation[s] >= interval_ticks gets counters[s] += 1
 * (uint64 wrap), last_rotation[s] = now_ticks, keys[s] = HMAC-SHA256(secrets[s], BE64(counter) ||
 * BE64(now_ticks)), fresh mid[s], and rotated[s] = 1; every other slot gets rotated[s] = 0 and is
 * not written.  rotated [S].  ENET_EINVAL for interval_ticks < 0; sessions == 0 is a no-op. */
ENET_API int enet_session_rotate_batch(const enet_session_table* t, int64_t now_ticks, int64_t interval_ticks,
                                       uint8_t* rotated, void* stream);
/* KeyExchange::compute_public / derive_shared_secret (KeyExchange.cpp:22-48) for n keypairs:
 * public_out[i] = 5^private_keys[i] mod 2^31-1; when remote_public is given,
 * secret_out[i] ([n][32], 4-byte aligned) = SHA-256(BE32((remote_public[i] mod P)^private_keys[i]
 * mod P)).  public_out or secret_out may be NULL (secret_out needs remote_public). */
ENET_API int enet_key_exchange_batch(uint32_t n, const uint32_t* private_keys, const uint32_t* remote_public,
                                     uint32_t* public_out, uint8_t* secret_out, void* stream);

/* ---- host-resident pipeline
 * The reference's crypto path starts and ends in host memory (socket / relay buffers,
 * SessionManager.cpp:362-387 and 815-822; chunk files, Node.cpp:1414-1417 and 1641-1655).  These
 * calls take an enet_records batch whose arenas, offsets, keys, nonces, counters, tags, MACs and
 * ok flags are all HOST pointers, cut it into chunks of about `chunk_bytes` on record boundaries
 * and run each chunk through one of `streams` slots (a HIP stream plus pinned, device-mapped
 * staging), chunks overlapped; inside a chunk of mixed lengths records are run longest first.
 * Arenas the device can address (enet_host_alloc, hipHostMalloc, registered memory) are worked
 * on in place; pageable arenas are gathered into / scattered out of the pinned staging by the
 * runtime's host worker threads (enet_host_stats).  See enet_host_set_mode for how the
 * kernels reach host memory.  `order` must be NULL.  Every call blocks until all outputs are in
 * host memory.  A pipeline owns its streams and staging (grown on demand) and serves one host
 * thread at a time. */
typedef struct enet_pipeline enet_pipeline;
/* device: HIP ordinal; chunk_bytes: 0 = 16 MiB (mixed-length batches with HMAC want larger
 * chunks: one lane hashes a whole record, so a chunk takes at least its longest record's
 * serial SHA-256 time); streams: 0 = 3 (max 16).  NULL on failure.  The defaults saturate
 * PCIe Gen5 on MI355X for uniform batches (~64 GB/s both directions together). */
ENET_API enet_pipeline* enet_pipeline_create(int device, uint64_t chunk_bytes, uint32_t streams);
ENET_API void enet_pipeline_destroy(enet_pipeline* pipe);
/* ChaCha20::apply per record (CryptoManager chunk mode with counters = LE32(chunk_id)) */
ENET_API int enet_pipeline_chacha20_xor(enet_pipeline* pipe, const enet_records* host_records,
                                        const uint32_t* counters);
/* RFC 8439 AEAD seal / open (no AAD): tags [n][16]; ok [n] (failed records come back zeroed) */
ENET_API int enet_pipeline_aead_seal(enet_pipeline* pipe, const enet_records* host_records,
                                     uint8_t* tags);
ENET_API int enet_pipeline_aead_open(enet_pipeline* pipe, const enet_records* host_records,
                                     const uint8_t* tags, uint8_t* ok);
/* AEAD + HMAC-SHA256(key, plaintext) (enet_aead_hmac_*_batch): macs [n][32] */
ENET_API int enet_pipeline_aead_hmac_seal(enet_pipeline* pipe, const enet_records* host_records,
                                          uint8_t* tags, uint8_t* macs);
ENET_API int enet_pipeline_aead_hmac_open(enet_pipeline* pipe, const enet_records* host_records,
                                          const uint8_t* tags, const uint8_t* macs, uint8_t* ok);
/* Whole wire frames (enet_wire_seal_batch / enet_wire_open_batch) from and to host memory:
 * seal out_offsets give |m_i| + 48, open out_offsets give max(0, |f_i| - 48); ok [n]. */
ENET_API int enet_pipeline_wire_seal(enet_pipeline* pipe, const enet_records* host_records);
ENET_API int enet_pipeline_wire_open(enet_pipeline* pipe, const enet_records* host_records, uint8_t* ok);
/* How host-resident batches reach the kernels (pipelines and crypto::batch::*), process-wide:
 * 0 = zero-copy -- the kernels read and write pinned host memory directly over PCIe;
 * 3 = SDMA with H2D on one stream, the kernels on their own stream(s) (two for hash-chain-bound
 * jobs) and D2H on another; 4 = SDMA for the H2D copies as 3, the kernels writing their outputs
 * straight into pinned host memory (no D2H copies).  Values 1 and 2 were retired (EINVAL).
 * Default: ENET_HOST_MODE=zc|splitk|zcout if set, else AUTO (-1): mode 3, except for jobs whose
 * output arena the device can write in place (caller-pinned: enet_host_alloc / registered) --
 * there the faster of 3 and 4 depends on the HIP runtime the process loaded (the system ROCm 7.2
 * runtime: 3, 39.7 vs 36.6 GiB/s per direction for C2; PyTorch's bundled runtime, loaded first in
 * a Python process: 4, 35.6 vs 29.5), so each device's first two such jobs of >= 64 MiB per mode
 * alternate 3 and 4 and the better rate is kept (mode 4 only when > 3 % faster).
 * enet_host_set_mode(-1) returns to auto and forgets the decisions; enet_host_mode() is the fixed
 * mode or -1.  Results are identical in every mode. */
#define ENET_HOST_MODE_AUTO (-1)
ENET_API int enet_host_set_mode(int mode);
ENET_API int enet_host_mode(void);
/* The auto state of a device: best job rate (GiB/s of input) seen in mode 3 and mode 4, jobs
 * sampled in each, and the decision (3 / 4, or -1 while sampling). */
typedef struct enet_host_probe {
    double splitk_gibs, zcout_gibs;
    int32_t samples_splitk, samples_zcout;
    int32_t mode;
} enet_host_probe;
/* Returns the device's decision (or -1) and fills *out (nullable). */
ENET_API int enet_host_mode_auto(int device, enet_host_probe* out);
/* Decides up front instead of from the first jobs: 256 MiB of 4 KiB AEAD seals from and to
 * pinned host memory (512 MiB pinned for the call, ~0.2 s), modes 3 and 4 alternating, best of
 * three each; the decision becomes the device's auto decision.  Returns 3 / 4 or ENET_EHIP /
 * ENET_ENOMEM. */
ENET_API int enet_host_mode_probe(int device, enet_host_probe* out);
/* The decision rule: 4 when zcout_gibs > 1.03 x splitk_gibs, else 3; -1 while either is 0. */
ENET_API int enet_host_mode_for(const enet_host_probe* rates);
/* Where a pipeline's host side runs (host_topo.hpp).  Pinned staging (and enet_host_alloc blocks)
 * go on the device's NUMA node: an anonymous mapping bound MPOL_PREFERRED to the node, faulted in
 * and hipHostRegister'ed (ENET_HOST_NUMA=auto (default) | hip (hipHostMalloc places it) | <node>).
 * Host worker threads run on that node's CPUs within the process's affinity mask; their number
 * comes from the CPU budget -- min(affinity mask, cgroup cpu.max quota), or ENET_HOST_CPUS --
 * shared by the engines alive in the process (at most 8 workers each), and they spin between task
 * sets only while every pool thread has a CPU of its own. */
typedef struct enet_host_stats {
    uint64_t jobs, chunks, records, in_bytes, out_bytes;
    uint64_t gathered_bytes, scattered_bytes;      /* copied by the host worker threads */
    uint64_t direct_in_chunks, direct_out_chunks;  /* chunks whose arena the device used in place */
    uint64_t pinned_bytes;                         /* staging the pipeline holds */
    int32_t device_node;   /* NUMA node of the device (-1 unknown) */
    int32_t target_node;   /* node the staging is placed on (-1: hipHostMalloc decides) */
    int32_t staging_node;  /* node its first staging page is on (-1 none yet / unknown) */
    uint32_t workers;      /* host worker threads (0 before the first gather / scatter) */
    uint32_t cpu_budget;   /* CPUs the plan had */
    int32_t spin;          /* workers spin between task sets */
    int32_t mode;          /* host mode of the last job */
} enet_host_stats;
ENET_API int enet_pipeline_stats(const enet_pipeline* pipe, enet_host_stats* out);
/* NUMA node of a device (from its PCI function; -1 unknown) */
ENET_API int enet_device_numa_node(int device);
/* the CPU budget of this process (affinity mask, cgroup quota, ENET_HOST_CPUS) */
ENET_API uint32_t enet_host_cpu_budget(void);
/* pinned host bytes held by the library (staging + enet_host_alloc) */
ENET_API uint64_t enet_host_pinned_bytes(void);
/* The thread plan for given facts (CPU-testable): node_cpulist / allowed_cpulist in sysfs list
 * form ("0-7,16"), cpu_max as cgroup v2 cpu.max ("1600000 100000", "max 100000"; NULL / "" =
 * unlimited), env_cpus as ENET_HOST_CPUS (0 = unset), engines sharing the budget. */
typedef struct enet_host_plan_t {
    uint32_t budget;    /* CPUs of the process */
    uint32_t workers;   /* worker threads per engine */
    int32_t spin;
    uint32_t ncpus;     /* CPUs the workers may run on */
    char cpus[256];     /* ... as a list (truncated if longer) */
} enet_host_plan_t;
ENET_API int enet_host_plan(const char* node_cpulist, const char* allowed_cpulist, const char* cpu_max,
                            uint32_t env_cpus, uint32_t engines, enet_host_plan_t* out);
/* ---- several devices of one node (no reference counterpart -- the reference
 *      runs src/crypto on one core per call): one pipeline, host thread and stream set per device,
 *      each call cuts the batch into contiguous record ranges balanced by input bytes and runs
 *      them concurrently, no collective.  devices == NULL or ndev == 0: every visible device (a
 *      device may be listed twice: two pipelines on it).  Same arguments and results as the
 *      single-device calls above; the first failing range's status is returned. */
typedef struct enet_pipeline_group enet_pipeline_group;
ENET_API enet_pipeline_group* enet_pipeline_group_create(const int* devices, uint32_t ndev,
                                                         uint64_t chunk_bytes, uint32_t streams);
ENET_API void enet_pipeline_group_destroy(enet_pipeline_group* group);
ENET_API uint32_t enet_pipeline_group_size(const enet_pipeline_group* group);
ENET_API int enet_pipeline_group_chacha20_xor(enet_pipeline_group* group,
                                              const enet_records* host_records,
                                              const uint32_t* counters);
ENET_API int enet_pipeline_group_aead_seal(enet_pipeline_group* group,
                                           const enet_records* host_records, uint8_t* tags);
ENET_API int enet_pipeline_group_aead_open(enet_pipeline_group* group,
                                           const enet_records* host_records, const uint8_t* tags,
                                           uint8_t* ok);
ENET_API int enet_pipeline_group_aead_hmac_seal(enet_pipeline_group* group,
                                                const enet_records* host_records, uint8_t* tags,
                                                uint8_t* macs);
ENET_API int enet_pipeline_group_aead_hmac_open(enet_pipeline_group* group,
                                                const enet_records* host_records,
                                                const uint8_t* tags, const uint8_t* macs,
                                                uint8_t* ok);
/* Pinned, device-mapped host memory for socket / relay buffer pools, on the NUMA node of the
 * calling thread's current device (see enet_pipeline_stats); NULL on failure. */
ENET_API void* enet_host_alloc(uint64_t bytes);
ENET_API void enet_host_free(void* p);
/* Register an existing host buffer pool (hipHostRegister, device-mapped) so pipelines work on it
 * in place; unregister before freeing it.  An arena is used in place only when it lies wholly in
 * ONE allocation or registered range -- otherwise it is gathered through the staging. */
ENET_API int enet_host_register(void* p, uint64_t bytes);
ENET_API int enet_host_unregister(void* p);

/* ---- helpers (host) */
/* LE32(chunk_id[0..3]) -- CryptoManager.cpp:8-13 derive_counter. */
ENET_API uint32_t enet_chunk_counter(const uint8_t chunk_id[32]);
/* Lanes the scheduler gives each record for a batch of this shape (for tests / tuning). */
ENET_API uint32_t enet_lanes_per_record(uint32_t count, uint64_t total_bytes, uint32_t max_len);
/* Force lanes per record (1, 2, 4, 8 or 16) for all later calls in this process; 0 restores the
 * scheduler.  Returns ENET_EINVAL for other values.  Tuning / test knob. */
ENET_API int enet_set_lanes_per_record(uint32_t lanes);
/* Sequence-parallel path (segments.hip) for enet_chacha20_xor_batch / enet_aead_seal_batch /
 * enet_aead_open_batch: a record of >= ENET_SEG_MIN bytes is cut into 64 KiB tiles spread over
 * every CU, the tiles' Poly1305 partials combined on the device (a lone 32 MiB record otherwise
 * gets 16 lanes).  Automatic (-1, default) when max_len_hint >= ENET_SEG_MIN, unless the batch is
 * uniform with count * 16 >= 131072 lanes (the record kernels fill the chip then); a value >= 0
 * sends every record of at least that many bytes to the tiles whatever the hints (0: every
 * record; INT64_MAX: never).  Results are identical; tuning / test knob. */
#define ENET_SEG_MIN (256u << 10)
ENET_API int enet_set_seg_min(int64_t bytes);
/* Chunk store / fetch: records of at least this many bytes (default ENET_HOST_HASH_MIN, and only
 * while the host threads' chains finish before one GPU lane's would: sum(long) < ~60 x CPU budget x
 * longest) have their SHA-256 computed on host threads (SHA-NI) while the device runs their
 * ChaCha20 on the tiles -- SHA-256 of one message is one serial chain (~34 MB/s on a GPU lane,
 * ~2.1 GB/s on a host core).  Taken only when the batch's max_len_hint is at least the threshold;
 * such a call synchronises the stream: it reads the offsets first and returns when the batch is
 * done.  -1 = auto; 0 .. INT64_MAX forces the threshold (INT64_MAX: never,
 * every chain on the GPU).  Results are identical; tuning / test knob. */
#define ENET_HOST_HASH_MIN (256u << 10)
ENET_API int enet_set_host_hash_min(int64_t bytes);
/* Chunk store / fetch batches that took the host-hash route in this process (tests / tuning). */
ENET_API uint64_t enet_host_hash_batches(void);
/* Batches that have taken the sequence-parallel path in this process (tests / tuning). */
ENET_API uint64_t enet_seg_batches(void);
/* Which record kernel the batches of this process ran on: out[k] = records handed so far to
 * launches of kind k -- 0 per-lane, 1 run-staged (256-thread workgroups), 2 line-staged, 3 lockstep
 * run-staged (512-thread workgroups), 4 streaming.  A uniform batch counts its whole workgroups
 * under the staged / streaming kind and its remaining records under 0.  Cumulative, relaxed
 * atomics (tests / tuning). */
ENET_API void enet_record_route_counts(uint64_t out[5]);
/* Staging of uniform-length batches (all records the same length): 1 = register prefetch + LDS
 * transposition (default; records that are not 128-byte aligned and get one lane each are staged
 * as whole aligned 128-byte lines; the rest in lockstep 512-thread workgroups), 4 = 1 without the
 * line staging, 5 = lockstep run staging only, 0 = per-lane path only, -1 restores the default.
 * (3, the LDS-DMA variant, was retired: it is refused.)
 * Results are identical; tuning / test knob. */
ENET_API int enet_set_staging(int variant);
/* ---- scalar C++ drop-in routing (include/ephemeralnet/crypto/{ChaCha20,Sha256,HmacSha256,
 *      CryptoManager}.hpp, security/StoreProof.hpp, network/KeyManager.hpp)
 * The reference signatures take ONE record per call from many session threads
 * (SessionManager.cpp:332,703) and never throw.  A GPU round trip costs >= ~18 us,
 * and SHA-256 of one message is one serial chain, so the drop-in routes each call by size:
 *   ENET_SCALAR_AUTO (default)  SHA-256 / HMAC / single PoW checks, and ChaCha20 records below
 *                               the crossover, run on the calling thread's host engine (SHA-NI,
 *                               AVX-512 / AVX2; csrc/host_engine.cpp); ChaCha20 records at or
 *                               above it go to the MI355X, concurrent callers coalesced into one
 *                               launch through a pinned arena; PoW searches and
 *                               KeyManager::rotate_all_due run on the MI355X.  The default
 *                               crossover is UINT64_MAX (never): measured on the box, the host
 *                               engine's keystream (~10 GB/s per thread) is as fast as the memcpy
 *                               a pageable caller buffer needs to reach the device at all.
 *   ENET_SCALAR_DEVICE          every call that has a device kernel runs on the MI355X (round-2
 *                               behaviour; the streaming Sha256 class stays on the host).
 *   ENET_SCALAR_HOST            everything on the host engine.
 * crossover_bytes = 0 keeps the current value.  A failed device call of the
 * scalar API is finished on the host engine (bit-exact), counted in device_failures and reported
 * once on stderr -- or, after enet_scalar_set_on_device_error(1), abort()s.  No exception ever
 * leaves a reference signature except std::bad_alloc.  The batch entry points (this header's
 * *_batch / pipeline calls and C++ crypto::batch::*) never use the host engine. */
#define ENET_SCALAR_AUTO 0
#define ENET_SCALAR_DEVICE 1
#define ENET_SCALAR_HOST 2
ENET_API int enet_scalar_set_policy(int policy, uint64_t crossover_bytes);
ENET_API int enet_scalar_policy(void);
/* 0 = finish a failed device call on the host engine (default), 1 = abort() */
ENET_API int enet_scalar_set_on_device_error(int mode);
typedef struct enet_scalar_stats {
    uint64_t host_calls;         /* scalar calls served by the host engine */
    uint64_t device_calls;       /* scalar calls served by the MI355X */
    uint64_t device_failures;    /* device calls that failed and were finished on the host */
    uint64_t coalesced_launches; /* device launches of the ChaCha20::apply coalescer */
    uint64_t coalesced_records;  /* records they carried (>= launches: calls merged across threads) */
} enet_scalar_stats;
ENET_API void enet_scalar_get_stats(enet_scalar_stats* out);
ENET_API void enet_scalar_reset_stats(void);
/* Test hook: the next n device calls of the scalar API fail as if the device had. */
ENET_API void enet_scalar_inject_device_failures(uint32_t n);
/* The host engine's instruction sets on this CPU ("sha-ni+avx2", ..., "portable"). */
ENET_API const char* enet_host_isa(void);
/* The host engine itself, one record (host pointers): ChaCha20::apply, Sha256::digest,
 * HmacSha256::compute semantics.  For callers that want the scalar path without the C++ API. */
ENET_API void enet_host_chacha20_xor(const uint8_t key[32], const uint8_t nonce[12], uint32_t counter,
                                     const uint8_t* in, uint8_t* out, uint64_t n);
ENET_API void enet_host_sha256(const uint8_t* in, uint64_t n, uint8_t digest[32]);
ENET_API void enet_host_hmac_sha256(const uint8_t* key, uint64_t key_len, const uint8_t* in, uint64_t n,
                                    uint8_t mac[32]);
/* One session frame's body on the host engine (SessionManager::send, SessionManager.cpp:374-385):
 * out[0..n+32) = ChaCha20(key, nonce, counter 0) XOR (m || HMAC-SHA256(key, m)); the wire frame is
 * nonce || BE32(n + 32) || out.  On AMD CPUs with SHA-NI + AVX-512 the HMAC is stitched into the
 * keystream's rounds in one pass over m.  out may overlap m. */
ENET_API void enet_host_seal_body(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* m, uint64_t n,
                                  uint8_t* out);
/* The receiving side (SessionManager::receive_loop, SessionManager.cpp:815-822, then
 * decode_signed's MAC check, Message.cpp:313-328): m[0..bl-32) = the decrypted body; returns 1 when
 * the decrypted MAC verifies, else 0 with m zeroed (0 for bl < 32).  Stitched like seal (the hash
 * one keystream step behind).  m may overlap body. */
ENET_API int enet_host_open_body(const uint8_t key[32], const uint8_t nonce[12], const uint8_t* body, uint64_t bl,
                                 uint8_t* m);
/* Tuning / test knob for the stitched pass of enet_host_seal_body / enet_host_open_body: -1 = on AMD
 * CPUs for bodies over 64 bytes (default), 0 = never, 1 = at every size whenever the CPU has
 * SHA-NI + AVX-512.  Results are identical.  Returns the previous mode. */
ENET_API int enet_host_set_seal_stitch(int mode);

/* Duplex paths with a hash beside the cipher (chunk store / fetch with ids, AEAD + HMAC): long
 * records run with each record's work split over a cipher, a SHA-256 schedule and a SHA-256
 * rounds wave (a ~1.4x shorter serial chain, duplex_split.hip).  -1 = automatic (when
 * max_len_hint >= 16 KiB and the batch is uniform or has an `order`, e.g. length-sorted; the
 * default), 0 = never, 1 = always.  Results are identical; tuning / test knob. */
ENET_API int enet_set_duplex_split(int mode);
/* Human-readable text of the last error on this host thread ("" if none). */
ENET_API const char* enet_last_error(void);
/* ABI version: (major << 16) | minor. */
ENET_API uint32_t enet_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ENET_CRYPTO_H */
