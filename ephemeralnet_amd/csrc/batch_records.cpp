// batch_records.cpp -- the crypto::batch calls (Batch.hpp) that run as one job of the host-memory
// batch runtime (host_batch.hpp): ChaCha20, AEAD, session frame bodies, wire frames and the chunk
// store / fetch steps.  Many records per call, always on the MI355X; they throw
// std::invalid_argument / std::runtime_error (not reference signatures).
//
// Every entry has the same shape: check_sizes, the early return of an empty batch, job_of, the
// op's own per-record arrays, then one of the two sinks, which runs the job.
#include "ephemeralnet/crypto/Batch.hpp"

#include <hip/hip_runtime.h>

#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "host_batch.hpp"
#include "staging.hpp"

namespace ephemeralnet::crypto::batch {

namespace {
using namespace enet::api;
using enet::hb::Job;
using enet::hb::Op;

// One batch call through the host-memory runtime of the calling thread's device (host_batch.hpp):
// pinned, device-mapped staging, host worker threads gathering / scattering, chunks overlapped.
void run_host_batch(const Job& j) {
    int dev = 0;
    enet::stage::hip_check(hipGetDevice(&dev), "hipGetDevice");
    enet::hb::run_shared(dev, j);
}

Job job_of(Op op, Records in, const std::uint8_t* keys, const std::uint8_t* nonces) {
    Job j;
    j.op = op;
    j.n = in.size();
    j.in_spans = in;
    j.keys = keys;
    j.nonces = nonces;
    return j;
}

// sink: one vector per record, resized by the runtime
void into_vectors(Job& j, std::vector<std::vector<std::uint8_t>>& out) {
    j.out_vecs = &out;
    run_host_batch(j);
}

// sink: one contiguous span, record i at the prefix sums of the op's output lengths
void into_span(Job& j, Records in, std::span<std::uint8_t> out, const char* what) {
    const auto off = enet::stage::offsets_of(in, enet::hb::out_delta(j.op));
    if (off.back() > out.size())
        throw std::invalid_argument(std::string("enet batch::") + what + ": output span too small");
    j.out_base = out.data();
    j.out_off = off.data();
    run_host_batch(j);
}
}  // namespace

std::vector<std::uint64_t> packed_offsets(Records records, std::int64_t delta) {
    return enet::stage::offsets_of(records, delta);
}

// ---- ChaCha20::apply
void chacha20_apply(std::span<const Key> keys, std::span<const Nonce> nonces, Records inputs,
                    std::span<const std::uint32_t> counters, std::vector<std::vector<std::uint8_t>>& out) {
    const size_t n = inputs.size();
    check_sizes("chacha20_apply", n, {keys.size(), nonces.size(), optional_size(counters, n)});
    out.resize(n);
    if (n == 0) return;
    auto j = job_of(Op::Xor, inputs, key_bytes(keys), nonce_bytes(nonces));
    j.counters = counters.empty() ? nullptr : counters.data();
    into_vectors(j, out);
}

std::vector<std::vector<std::uint8_t>> chacha20_apply(std::span<const Key> keys, std::span<const Nonce> nonces,
                                                      Records inputs, std::span<const std::uint32_t> counters) {
    std::vector<std::vector<std::uint8_t>> res;
    chacha20_apply(keys, nonces, inputs, counters, res);
    return res;
}

void chacha20_apply(std::span<const Key> keys, std::span<const Nonce> nonces, Records inputs,
                    std::span<const std::uint32_t> counters, std::span<std::uint8_t> out) {
    const size_t n = inputs.size();
    check_sizes("chacha20_apply", n, {keys.size(), nonces.size(), optional_size(counters, n)});
    if (n == 0) return;
    auto j = job_of(Op::Xor, inputs, key_bytes(keys), nonce_bytes(nonces));
    j.counters = counters.empty() ? nullptr : counters.data();
    into_span(j, inputs, out, "chacha20_apply");
}

// ---- RFC 8439 AEAD
void aead_seal(std::span<const Key> keys, std::span<const Nonce> nonces, Records plaintexts, std::vector<Sealed>& out) {
    const size_t n = plaintexts.size();
    check_sizes("aead_seal", n, {keys.size(), nonces.size()});
    out.resize(n);
    if (n == 0) return;
    std::vector<std::vector<std::uint8_t>*> each(n);
    for (size_t i = 0; i < n; ++i) each[i] = &out[i].data;
    std::vector<std::uint8_t> th(16 * n);
    auto j = job_of(Op::AeadSeal, plaintexts, key_bytes(keys), nonce_bytes(nonces));
    j.out_each = each;
    j.tags_out = th.data();
    run_host_batch(j);
    for (size_t i = 0; i < n; ++i) std::memcpy(out[i].tag.data(), th.data() + 16 * i, 16);
}

std::vector<Sealed> aead_seal(std::span<const Key> keys, std::span<const Nonce> nonces, Records plaintexts) {
    std::vector<Sealed> res;
    aead_seal(keys, nonces, plaintexts, res);
    return res;
}

void aead_seal(std::span<const Key> keys, std::span<const Nonce> nonces, Records plaintexts,
               std::span<std::uint8_t> out, std::span<std::array<std::uint8_t, 16>> tags) {
    const size_t n = plaintexts.size();
    check_sizes("aead_seal", n, {keys.size(), nonces.size(), tags.size()});
    if (n == 0) return;
    auto j = job_of(Op::AeadSeal, plaintexts, key_bytes(keys), nonce_bytes(nonces));
    j.tags_out = tags.data()->data();
    into_span(j, plaintexts, out, "aead_seal");
}

void aead_open(std::span<const Key> keys, std::span<const Nonce> nonces, Records ciphertexts,
               std::span<const std::array<std::uint8_t, 16>> tags, std::vector<std::vector<std::uint8_t>>& out,
               std::vector<std::uint8_t>& ok) {
    const size_t n = ciphertexts.size();
    check_sizes("aead_open", n, {keys.size(), nonces.size(), tags.size()});
    ok.assign(n, 0);
    out.resize(n);
    if (n == 0) return;
    auto j = job_of(Op::AeadOpen, ciphertexts, key_bytes(keys), nonce_bytes(nonces));
    j.tags_in = tags.data()->data();
    j.ok_out = ok.data();
    into_vectors(j, out);
}

std::vector<std::vector<std::uint8_t>> aead_open(std::span<const Key> keys, std::span<const Nonce> nonces,
                                                 Records ciphertexts,
                                                 std::span<const std::array<std::uint8_t, 16>> tags,
                                                 std::vector<std::uint8_t>& ok) {
    std::vector<std::vector<std::uint8_t>> res;
    aead_open(keys, nonces, ciphertexts, tags, res, ok);
    return res;
}

void aead_open(std::span<const Key> keys, std::span<const Nonce> nonces, Records ciphertexts,
               std::span<const std::array<std::uint8_t, 16>> tags, std::span<std::uint8_t> out,
               std::span<std::uint8_t> ok) {
    const size_t n = ciphertexts.size();
    check_sizes("aead_open", n, {keys.size(), nonces.size(), tags.size(), ok.size()});
    if (n == 0) return;
    auto j = job_of(Op::AeadOpen, ciphertexts, key_bytes(keys), nonce_bytes(nonces));
    j.tags_in = tags.data()->data();
    j.ok_out = ok.data();
    into_span(j, ciphertexts, out, "aead_open");
}

// ---- session frame bodies
std::vector<std::vector<std::uint8_t>> frame_seal(Keys32 session_keys, std::span<const Nonce> nonces, Records messages) {
    const size_t n = messages.size();
    check_sizes("frame_seal", n, {session_keys.size(), nonces.size()});
    std::vector<std::vector<std::uint8_t>> res;
    if (n == 0) return res;
    auto j = job_of(Op::FrameSeal, messages, session_keys.data()->data(), nonce_bytes(nonces));
    into_vectors(j, res);
    return res;
}

std::vector<std::vector<std::uint8_t>> frame_open(Keys32 session_keys, std::span<const Nonce> nonces, Records bodies,
                                                  std::vector<std::uint8_t>& ok) {
    const size_t n = bodies.size();
    check_sizes("frame_open", n, {session_keys.size(), nonces.size()});
    ok.assign(n, 0);
    std::vector<std::vector<std::uint8_t>> res;
    if (n == 0) return res;
    auto j = job_of(Op::FrameOpen, bodies, session_keys.data()->data(), nonce_bytes(nonces));
    j.ok_out = ok.data();
    into_vectors(j, res);
    return res;
}

// ---- chunk store / fetch
std::vector<StoredChunk> chunk_store(std::span<const Key> keys, std::span<const Nonce> nonces, Records chunks,
                                     std::span<const ChunkId> chunk_ids) {
    const size_t n = chunks.size();
    check_sizes("chunk_store", n, {keys.size(), nonces.size(), optional_size(chunk_ids, n)});
    if (n == 0) return {};
    std::vector<std::vector<std::uint8_t>> data;
    std::vector<std::uint8_t> hh(32 * n);
    auto j = job_of(Op::ChunkStore, chunks, key_bytes(keys), nonce_bytes(nonces));
    j.ids = chunk_ids.empty() ? nullptr : chunk_ids.data()->data();
    j.macs_out = hh.data();
    into_vectors(j, data);
    std::vector<StoredChunk> res(n);
    for (size_t i = 0; i < n; ++i) {
        res[i].data = std::move(data[i]);
        std::memcpy(res[i].chunk_hash.data(), hh.data() + 32 * i, 32);
    }
    return res;
}

std::vector<std::vector<std::uint8_t>> chunk_fetch(std::span<const Key> keys, std::span<const Nonce> nonces,
                                                   std::span<const ChunkId> chunk_ids, Records ciphertexts,
                                                   Keys32 chunk_hashes, std::vector<std::uint8_t>& ok) {
    const size_t n = ciphertexts.size();
    check_sizes("chunk_fetch", n, {keys.size(), nonces.size(), chunk_ids.size(), chunk_hashes.size()});
    ok.assign(n, 0);
    std::vector<std::vector<std::uint8_t>> res;
    if (n == 0) return res;
    auto j = job_of(Op::ChunkFetch, ciphertexts, key_bytes(keys), nonce_bytes(nonces));
    j.ids = chunk_ids.data()->data();
    j.macs_in = chunk_hashes.data()->data();
    j.ok_out = ok.data();
    into_vectors(j, res);
    return res;
}

// ---- wire frames
void wire_seal(Keys32 session_keys, std::span<const Nonce> nonces, Records messages,
               std::vector<std::vector<std::uint8_t>>& frames) {
    const size_t n = messages.size();
    check_sizes("wire_seal", n, {session_keys.size(), nonces.size()});
    frames.resize(n);
    if (n == 0) return;
    auto j = job_of(Op::WireSeal, messages, session_keys.data()->data(), nonce_bytes(nonces));
    into_vectors(j, frames);
}

std::vector<std::vector<std::uint8_t>> wire_seal(Keys32 session_keys, std::span<const Nonce> nonces, Records messages) {
    std::vector<std::vector<std::uint8_t>> res;
    wire_seal(session_keys, nonces, messages, res);
    return res;
}

void wire_seal(Keys32 session_keys, std::span<const Nonce> nonces, Records messages, std::span<std::uint8_t> frames) {
    const size_t n = messages.size();
    check_sizes("wire_seal", n, {session_keys.size(), nonces.size()});
    if (n == 0) return;
    auto j = job_of(Op::WireSeal, messages, session_keys.data()->data(), nonce_bytes(nonces));
    into_span(j, messages, frames, "wire_seal");
}

void wire_open(Keys32 session_keys, Records frames, std::vector<std::vector<std::uint8_t>>& messages,
               std::vector<std::uint8_t>& ok) {
    const size_t n = frames.size();
    check_sizes("wire_open", n, {session_keys.size()});
    ok.assign(n, 0);
    messages.resize(n);
    if (n == 0) return;
    auto j = job_of(Op::WireOpen, frames, session_keys.data()->data(), nullptr);
    j.ok_out = ok.data();
    into_vectors(j, messages);
}

std::vector<std::vector<std::uint8_t>> wire_open(Keys32 session_keys, Records frames, std::vector<std::uint8_t>& ok) {
    std::vector<std::vector<std::uint8_t>> res;
    wire_open(session_keys, frames, res, ok);
    return res;
}

void wire_open(Keys32 session_keys, Records frames, std::span<std::uint8_t> messages, std::span<std::uint8_t> ok) {
    const size_t n = frames.size();
    check_sizes("wire_open", n, {session_keys.size(), ok.size()});
    if (n == 0) return;
    auto j = job_of(Op::WireOpen, frames, session_keys.data()->data(), nullptr);
    j.ok_out = ok.data();
    into_span(j, frames, messages, "wire_open");
}

std::vector<std::vector<std::uint8_t>> wire_seal_sessions(Keys32 session_table, std::span<const std::uint32_t> session,
                                                          std::span<const Nonce> nonces, Records messages) {
    const size_t n = messages.size(), K = session_table.size();
    check_sizes("wire_seal_sessions", n, {session.size(), nonces.size()}, K <= 0xffffffffu);
    std::vector<std::vector<std::uint8_t>> res;
    if (n == 0) return res;
    check_sessions(session, K, "wire_seal_sessions");
    auto j = job_of(Op::WireSeal, messages, session_table.data()->data(), nonce_bytes(nonces));
    j.session = session.data();
    j.n_sessions = (std::uint32_t)K;
    into_vectors(j, res);
    return res;
}

std::vector<std::vector<std::uint8_t>> wire_open_sessions(Keys32 session_table, std::span<const std::uint32_t> session,
                                                          Records frames, std::vector<std::uint8_t>& ok) {
    const size_t n = frames.size(), K = session_table.size();
    check_sizes("wire_open_sessions", n, {session.size()}, K <= 0xffffffffu);
    ok.assign(n, 0);
    std::vector<std::vector<std::uint8_t>> res;
    if (n == 0) return res;
    check_sessions(session, K, "wire_open_sessions");
    auto j = job_of(Op::WireOpen, frames, session_table.data()->data(), nullptr);
    j.session = session.data();
    j.n_sessions = (std::uint32_t)K;
    j.ok_out = ok.data();
    into_vectors(j, res);
    return res;
}

}  // namespace ephemeralnet::crypto::batch
