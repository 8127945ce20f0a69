// batch_staged.cpp -- the crypto::batch and security::batch calls (Batch.hpp, StoreProof.hpp) that
// drive the C ABI themselves over the calling thread's staging (staging.hpp): SHA-256, Shamir key
// shares and the chunk steps that carry them, chunk transfer, announce and Request / Acknowledge frames,
// frame triage, proof of work, session keys,
// key exchange and handshake admission.  Many records per call, always on the MI355X; they throw
// std::invalid_argument / std::runtime_error (not reference signatures).
//
// Every device sequence runs inside staged(): st.up() for each input, st.room() for each output,
// the C ABI call(s), st.d2h() for each result, st.sync().
#include "ephemeralnet/crypto/Batch.hpp"
#include "ephemeralnet/security/StoreProof.hpp"

#include <algorithm>
#include <cstring>
#include <iterator>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "api_common.hpp"
#include "enet_crypto.h"
#include "staging.hpp"

namespace ephemeralnet::crypto::batch {

using namespace enet::api;
using namespace enet::stage;

std::vector<std::array<std::uint8_t, 32>> sha256(Records messages) {
    const size_t n = messages.size();
    if (n == 0) return {};
    return staged([&](Staging& st) {
        const Packed in = pack(messages);
        auto* din = st.up(S_IN, in.arena.data(), in.arena.size());
        auto* doff = st.up<uint64_t>(S_INOFF, in.off.data(), 8 * (n + 1));
        auto* dout = st.room(S_OUT, 32 * n);
        enet_check(enet_sha256_batch((uint32_t)n, din, doff, dout, st.s()), "sha256");
        std::vector<std::array<std::uint8_t, 32>> res(n);
        st.d2h(res.data(), dout, 32 * n);
        st.sync();
        return res;
    });
}

// ---- Shamir key shares (enet_shamir_*_batch) and the store / fetch steps that carry them
namespace {
// n random bytes: a ChaCha20 keystream under a key from std::random_device (fill_random_bytes),
// one key per call -- std::random_device itself costs a system call or an RDRAND per 4 bytes
std::vector<std::uint8_t> random_stream(std::size_t n) {
    std::vector<std::uint8_t> out(n, 0);
    std::uint8_t key[32];
    const std::uint8_t nonce[12] = {};
    fill_random_bytes(key);
    enet_host_chacha20_xor(key, nonce, 0, out.data(), out.data(), n);
    return out;
}

void check_split_args(std::uint8_t threshold, std::uint8_t share_count, const char* what) {
    if (threshold == 0 || share_count == 0 || threshold > share_count)
        throw std::invalid_argument(std::string("enet batch::") + what + ": need 1 <= threshold <= share_count");
}

// indices [n][t] behind values [n][t][32] in one buffer (values first: they need the alignment)
std::vector<std::uint8_t> pack_shares(std::span<const std::vector<ShamirShare>> shares, std::uint8_t threshold,
                                      const char* what) {
    const std::size_t n = shares.size(), t = threshold;
    if (t == 0) throw std::invalid_argument(std::string("enet batch::") + what + ": threshold is 0");
    std::vector<std::uint8_t> buf(33 * n * t);
    for (std::size_t i = 0; i < n; ++i) {
        if (shares[i].size() < t)
            throw std::invalid_argument(std::string("enet batch::") + what + ": a record has fewer shares than threshold");
        for (std::size_t k = 0; k < t; ++k) {
            std::memcpy(buf.data() + 32 * (i * t + k), shares[i][k].value.data(), 32);
            buf[32 * n * t + i * t + k] = shares[i][k].index;
        }
    }
    return buf;
}

std::vector<std::vector<ShamirShare>> unpack_shares(const std::vector<std::uint8_t>& flat, std::size_t n,
                                                    std::size_t share_count) {
    std::vector<std::vector<ShamirShare>> res(n, std::vector<ShamirShare>(share_count));
    for (std::size_t i = 0; i < n; ++i)
        for (std::size_t j = 0; j < share_count; ++j) {
            res[i][j].index = static_cast<std::uint8_t>(j + 1);
            std::memcpy(res[i][j].value.data(), flat.data() + 32 * (i * share_count + j), 32);
        }
    return res;
}
}  // namespace

std::vector<std::vector<ShamirShare>> shamir_split(Keys32 secrets, std::uint8_t threshold, std::uint8_t share_count) {
    check_split_args(threshold, share_count, "shamir_split");
    const std::size_t n = secrets.size(), t = threshold, sc = share_count;
    check_count(n, "shamir_split");
    if (n == 0) return {};
    const std::vector<std::uint8_t> coeffs = random_stream(32 * n * (t - 1));
    return staged([&](Staging& st) {
        auto* dsec = st.up(S_KEYS, secrets.data(), 32 * n);
        auto* dco = t > 1 ? st.up(S_AUX, coeffs.data(), coeffs.size()) : nullptr;
        auto* dsh = st.room(S_OUT, 32 * n * sc);
        enet_check(enet_shamir_split_batch((uint32_t)n, dsec, dco, threshold, share_count, dsh, st.s()), "shamir_split");
        std::vector<std::uint8_t> flat(32 * n * sc);
        st.d2h(flat.data(), dsh, flat.size());
        st.sync();
        return unpack_shares(flat, n, sc);
    });
}

std::vector<std::array<std::uint8_t, 32>> shamir_combine(std::span<const std::vector<ShamirShare>> shares,
                                                         std::uint8_t threshold, std::vector<std::uint8_t>& ok) {
    const std::size_t n = shares.size(), t = threshold;
    check_count(n, "shamir_combine");
    const std::vector<std::uint8_t> packed = pack_shares(shares, threshold, "shamir_combine");
    ok.assign(n, 0);
    if (n == 0) return {};
    return staged([&](Staging& st) {
        auto* dsh = st.up(S_AUX, packed.data(), packed.size());
        auto* dsec = st.room(S_KEYS, 32 * n);
        auto* dok = st.room(S_OK, n);
        enet_check(enet_shamir_combine_batch((uint32_t)n, threshold, dsh + 32 * n * t, dsh, dsec, dok, st.s()),
                   "shamir_combine");
        std::vector<std::array<std::uint8_t, 32>> res(n);
        st.d2h(res.data(), dsec, 32 * n);
        st.d2h(ok.data(), dok, n);
        st.sync();
        return res;
    });
}

namespace {
// the records descriptor of a chunk batch whose arenas share one offsets array
enet_records chunk_records(std::size_t n, const Packed& p, const uint64_t* doff, const uint8_t* din, uint8_t* dout,
                           const uint8_t* dkeys, const uint8_t* dnonces, const char* what) {
    uint64_t longest = 0;
    for (std::size_t i = 0; i < n; ++i) longest = std::max(longest, p.off[i + 1] - p.off[i]);
    if (longest > 0xFFFFFFFFull) throw std::invalid_argument(std::string("enet batch::") + what + ": chunk too long");
    return records_of(n, doff, doff, din, dout, dkeys, dnonces, p.off[n], (uint32_t)longest);
}
}  // namespace

std::vector<SharedChunk> chunk_store_shared(std::span<const Nonce> nonces, Records chunks,
                                            std::span<const ChunkId> chunk_ids, std::uint8_t threshold,
                                            std::uint8_t share_count) {
    check_split_args(threshold, share_count, "chunk_store_shared");
    const std::size_t n = chunks.size(), t = threshold, sc = share_count;
    check_sizes("chunk_store_shared", n, {nonces.size(), optional_size(chunk_ids, n)});
    check_count(n, "chunk_store_shared");
    if (n == 0) return {};
    // keys [n][32], then the coefficient rows [n][t-1][32]
    const std::vector<std::uint8_t> rnd = random_stream(32 * n * t);
    const Packed in = pack(chunks);
    return staged([&](Staging& st) {
        const std::size_t bytes = in.arena.size();
        auto* din = st.up(S_IN, in.arena.data(), bytes);
        auto* dout = st.room(S_OUT, bytes);
        auto* doff = st.up<uint64_t>(S_INOFF, in.off.data(), 8 * (n + 1));
        auto* dkeys = st.up(S_KEYS, rnd.data(), 32 * n);
        auto* dco = t > 1 ? st.up(S_AUX, rnd.data() + 32 * n, 32 * n * (t - 1)) : nullptr;
        auto* dnon = st.up(S_NONCES, nonce_bytes(nonces), 12 * n);
        auto* dids = chunk_ids.empty() ? nullptr : st.up(S_CTR, chunk_ids.data()->data(), 32 * n);
        auto* dhash = st.room(S_TAGS, 32 * n);
        auto* dsh = st.room(S_OK, 32 * n * sc);
        const enet_records r = chunk_records(n, in, doff, din, dout, dkeys, dnon, "chunk_store_shared");
        enet_check(enet_chunk_store_batch(&r, dids, dhash, st.s()), "chunk_store");
        enet_check(enet_shamir_split_batch((uint32_t)n, dkeys, dco, threshold, share_count, dsh, st.s()),
                   "shamir_split");
        std::vector<std::uint8_t> data(bytes), hh(32 * n), flat(32 * n * sc);
        st.d2h(data.data(), dout, bytes);
        st.d2h(hh.data(), dhash, 32 * n);
        st.d2h(flat.data(), dsh, flat.size());
        st.sync();
        auto shares = unpack_shares(flat, n, sc);
        std::vector<SharedChunk> res(n);
        for (std::size_t i = 0; i < n; ++i) {
            res[i].chunk.data.assign(data.begin() + in.off[i], data.begin() + in.off[i + 1]);
            std::memcpy(res[i].chunk.chunk_hash.data(), hh.data() + 32 * i, 32);
            res[i].shares = std::move(shares[i]);
        }
        return res;
    });
}

std::vector<std::vector<std::uint8_t>> chunk_fetch_shared(std::span<const std::vector<ShamirShare>> shares,
                                                          std::uint8_t threshold, std::span<const Nonce> nonces,
                                                          std::span<const ChunkId> chunk_ids, Records ciphertexts,
                                                          Keys32 chunk_hashes, std::vector<std::uint8_t>& ok) {
    const std::size_t n = ciphertexts.size(), t = threshold;
    check_sizes("chunk_fetch_shared", n, {shares.size(), nonces.size(), chunk_ids.size(), chunk_hashes.size()});
    check_count(n, "chunk_fetch_shared");
    const std::vector<std::uint8_t> packed = pack_shares(shares, threshold, "chunk_fetch_shared");
    ok.assign(n, 0);
    if (n == 0) return {};
    const Packed in = pack(ciphertexts);
    return staged([&](Staging& st) {
        const std::size_t bytes = in.arena.size(), okpad = (n + 3) & ~std::size_t(3);
        auto* din = st.up(S_IN, in.arena.data(), bytes);
        auto* dout = st.room(S_OUT, bytes);
        auto* doff = st.up<uint64_t>(S_INOFF, in.off.data(), 8 * (n + 1));
        auto* dsh = st.up(S_AUX, packed.data(), packed.size());
        auto* dkeys = st.room(S_KEYS, std::max(32 * n, kDeviceOnly));
        auto* dnon = st.up(S_NONCES, nonce_bytes(nonces), 12 * n);
        auto* dids = st.up(S_CTR, chunk_ids.data()->data(), 32 * n);
        auto* dhash = st.up(S_TAGS, chunk_hashes.data()->data(), 32 * n);
        auto* dok = st.room(S_OK, 2 * okpad);  // the combine's verdicts, then the fetch's
        enet_check(enet_shamir_combine_batch((uint32_t)n, threshold, dsh + 32 * n * t, dsh, dkeys, dok, st.s()),
                   "shamir_combine");
        const enet_records r = chunk_records(n, in, doff, din, dout, dkeys, dnon, "chunk_fetch_shared");
        enet_check(enet_chunk_fetch_batch(&r, dids, dhash, dok + okpad, st.s()), "chunk_fetch");
        std::vector<std::uint8_t> data(bytes), oks(2 * okpad);
        st.d2h(data.data(), dout, bytes);
        st.d2h(oks.data(), dok, oks.size());
        st.sync();
        std::vector<std::vector<std::uint8_t>> res(n);
        for (std::size_t i = 0; i < n; ++i) {
            ok[i] = oks[i] & oks[okpad + i];
            res[i].assign(data.begin() + in.off[i], data.begin() + in.off[i + 1]);
            // a failed combine leaves the all-zero key, whose plaintext can only pass the hash check
            // by being the real one; it is withheld all the same
            if (!ok[i]) std::fill(res[i].begin(), res[i].end(), std::uint8_t{0});
        }
        return res;
    });
}

// ---- chunk transfer frames (enet_chunk_frame_*_batch): every per-record array travels in one
// buffer, each part at a 4-byte aligned offset
namespace {
// the head of that buffer: record i's session key
void gather_session_keys(std::vector<std::uint8_t>& meta, Keys32 table, std::span<const std::uint32_t> session) {
    for (std::size_t i = 0; i < session.size(); ++i) std::memcpy(meta.data() + 32 * i, table[session[i]].data(), 32);
}
}  // namespace

std::vector<std::vector<std::uint8_t>> chunk_frames_seal(Keys32 session_table, std::span<const std::uint32_t> session,
                                                         std::span<const Nonce> nonces, std::span<const ChunkId> chunk_ids,
                                                         std::span<const std::uint32_t> ttl_seconds, Records stored,
                                                         std::span<const std::uint8_t> versions) {
    const std::size_t n = stored.size(), K = session_table.size();
    check_sizes("chunk_frames_seal", n,
                {session.size(), nonces.size(), chunk_ids.size(), ttl_seconds.size(), optional_size(versions, n)});
    check_count(n, "chunk_frames_seal");
    if (n == 0) return {};
    check_sessions(session, K, "chunk_frames_seal");
    const Packed in = pack(stored);
    const std::vector<std::uint64_t> ooff = offsets_of(stored, 90);
    // keys | chunk ids | ttl | nonces | versions
    const std::size_t o_id = 32 * n, o_ttl = 64 * n, o_non = 68 * n, o_ver = 80 * n;
    std::vector<std::uint8_t> meta(81 * n);
    gather_session_keys(meta, session_table, session);
    std::memcpy(meta.data() + o_id, chunk_ids.data()->data(), 32 * n);
    std::memcpy(meta.data() + o_ttl, ttl_seconds.data(), 4 * n);
    std::memcpy(meta.data() + o_non, nonce_bytes(nonces), 12 * n);
    if (!versions.empty()) std::memcpy(meta.data() + o_ver, versions.data(), n);
    return staged([&](Staging& st) {
        const std::size_t obytes = ooff[n];
        auto* din = st.up(S_IN, in.arena.data(), in.arena.size());
        auto* dout = st.room(S_OUT, obytes);
        auto* dioff = st.up<uint64_t>(S_INOFF, in.off.data(), 8 * (n + 1));
        auto* dooff = st.up<uint64_t>(S_OUTOFF, ooff.data(), 8 * (n + 1));
        auto* dm = st.up(S_KEYS, meta.data(), meta.size());
        const enet_records r = records_of(n, dioff, dooff, din, dout, dm, dm + o_non);
        enet_check(enet_chunk_frame_seal_batch(&r, nullptr, 0, nullptr, dm + o_id, reinterpret_cast<const uint32_t*>(dm + o_ttl),
                                               versions.empty() ? nullptr : dm + o_ver, st.s()),
                   "chunk_frame_seal");
        std::vector<std::uint8_t> flat(obytes);
        st.d2h(flat.data(), dout, obytes);
        st.sync();
        std::vector<std::vector<std::uint8_t>> res(n);
        for (std::size_t i = 0; i < n; ++i) res[i].assign(flat.begin() + ooff[i], flat.begin() + ooff[i + 1]);
        return res;
    });
}

std::vector<OpenedChunk> chunk_frames_open(Keys32 session_table, std::span<const std::uint32_t> session, Records frames,
                                           std::span<const ChunkId> chunk_ids, std::span<const Key> chunk_keys,
                                           std::span<const Nonce> chunk_nonces, Keys32 chunk_hashes) {
    const std::size_t n = frames.size(), K = session_table.size();
    check_sizes("chunk_frames_open", n,
                {session.size(), chunk_ids.size(), chunk_keys.size(), chunk_nonces.size(), chunk_hashes.size()});
    check_count(n, "chunk_frames_open");
    if (n == 0) return {};
    check_sessions(session, K, "chunk_frames_open");
    const Packed in = pack(frames);
    const std::vector<std::uint64_t> ooff = offsets_of(frames, -90);
    // session keys | chunk ids | chunk keys | chunk hashes | chunk nonces
    const std::size_t o_id = 32 * n, o_ck = 64 * n, o_h = 96 * n, o_cn = 128 * n;
    std::vector<std::uint8_t> meta(140 * n);
    gather_session_keys(meta, session_table, session);
    std::memcpy(meta.data() + o_id, chunk_ids.data()->data(), 32 * n);
    std::memcpy(meta.data() + o_ck, key_bytes(chunk_keys), 32 * n);
    std::memcpy(meta.data() + o_h, chunk_hashes.data()->data(), 32 * n);
    std::memcpy(meta.data() + o_cn, nonce_bytes(chunk_nonces), 12 * n);
    return staged([&](Staging& st) {
        const std::size_t obytes = ooff[n];
        auto* din = st.up(S_IN, in.arena.data(), in.arena.size());
        auto* dpt = st.room(S_OUT, obytes);
        auto* dct = st.room(S_AUX, obytes);
        auto* dioff = st.up<uint64_t>(S_INOFF, in.off.data(), 8 * (n + 1));
        auto* dooff = st.up<uint64_t>(S_OUTOFF, ooff.data(), 8 * (n + 1));
        auto* dm = st.up(S_KEYS, meta.data(), meta.size());
        auto* dres = st.room(S_OK, 5 * n);  // ttl [n] uint32, then status [n]
        const enet_records r = records_of(n, dioff, dooff, din, dpt, dm, nullptr);
        enet_check(enet_chunk_frame_open_batch(&r, nullptr, 0, nullptr, dm + o_id, dm + o_ck, dm + o_cn, dm + o_h, dct,
                                               reinterpret_cast<uint32_t*>(dres), dres + 4 * n, st.s()),
                   "chunk_frame_open");
        std::vector<std::uint8_t> pt(obytes), ct(obytes), resv(5 * n);
        st.d2h(pt.data(), dpt, obytes);
        st.d2h(ct.data(), dct, obytes);
        st.d2h(resv.data(), dres, resv.size());
        st.sync();
        std::vector<OpenedChunk> res(n);
        for (std::size_t i = 0; i < n; ++i) {
            res[i].status = static_cast<ChunkFrameStatus>(resv[4 * n + i]);
            if (res[i].status != ChunkFrameStatus::Ok) continue;  // no plaintext, ciphertext or ttl of a failed frame
            std::memcpy(&res[i].ttl_seconds, resv.data() + 4 * i, 4);
            res[i].plaintext.assign(pt.begin() + ooff[i], pt.begin() + ooff[i + 1]);
            res[i].stored.assign(ct.begin() + ooff[i], ct.begin() + ooff[i + 1]);
        }
        return res;
    });
}

// ---- announce frames (enet_announce_frame_*_batch): every record brings its own manifest and
// endpoint (the NULL-index form of the C ABI); the three field arenas share one offsets buffer
SealedAnnounces announce_frames_seal(Keys32 session_table, std::span<const std::uint32_t> session,
                                     std::span<const Nonce> nonces, std::span<const AnnounceFields> announces,
                                     std::uint8_t difficulty, std::uint64_t max_attempts) {
    const std::size_t n = announces.size(), K = session_table.size();
    check_sizes("announce_frames_seal", n, {session.size(), nonces.size()});
    check_count(n, "announce_frames_seal");
    if (n == 0) return {};
    check_sessions(session, K, "announce_frames_seal");
    for (const AnnounceFields& a : announces)
        if (a.peer_id != announces[0].peer_id)
            throw std::invalid_argument("enet batch::announce_frames_seal: the announces of one call carry one peer_id");
    // uri | endpoint | shard arenas and their offsets [3][n + 1]; the frame offsets
    std::vector<std::uint8_t> uris, eps, shards;
    std::vector<std::uint64_t> off(3 * (n + 1), 0), ooff(n + 1, 0);
    for (std::size_t i = 0; i < n; ++i) {
        const AnnounceFields& a = announces[i];
        uris.insert(uris.end(), a.manifest_uri.begin(), a.manifest_uri.end());
        eps.insert(eps.end(), a.endpoint.begin(), a.endpoint.end());
        shards.insert(shards.end(), a.assigned_shards.begin(), a.assigned_shards.end());
        off[i + 1] = uris.size();
        off[n + 1 + i + 1] = eps.size();
        off[2 * (n + 1) + i + 1] = shards.size();
        const std::uint8_t v = a.version < 1 ? 1 : (a.version > 4 ? 4 : a.version);  // clamp_version
        ooff[i + 1] = ooff[i] + 130 + a.manifest_uri.size() + a.endpoint.size() + a.assigned_shards.size() + (v == 4 ? 8 : 0);
    }
    // keys | chunk ids | work nonces | ttl | frame nonces | local id | versions
    const std::size_t o_id = 32 * n, o_wn = 64 * n, o_ttl = 72 * n, o_non = 76 * n, o_pid = 88 * n, o_ver = 88 * n + 32;
    std::vector<std::uint8_t> meta(89 * n + 32);
    gather_session_keys(meta, session_table, session);
    for (std::size_t i = 0; i < n; ++i) {
        std::memcpy(meta.data() + o_id + 32 * i, announces[i].chunk_id.data(), 32);
        std::memcpy(meta.data() + o_wn + 8 * i, &announces[i].work_nonce, 8);
        std::memcpy(meta.data() + o_ttl + 4 * i, &announces[i].ttl_seconds, 4);
        meta[o_ver + i] = announces[i].version;
    }
    std::memcpy(meta.data() + o_non, nonce_bytes(nonces), 12 * n);
    std::memcpy(meta.data() + o_pid, announces[0].peer_id.data(), 32);
    return staged([&](Staging& st) {
        const std::size_t obytes = ooff[n];
        auto* dout = st.room(S_OUT, obytes);
        auto* dooff = st.up<uint64_t>(S_OUTOFF, ooff.data(), 8 * (n + 1));
        auto* doff = st.up<uint64_t>(S_INOFF, off.data(), 8 * off.size());
        // an arena may be empty (its vector then has no storage to copy from): room for one unread byte
        auto arena = [&](Slot slot, const std::vector<std::uint8_t>& v) {
            return v.empty() ? st.room(slot, 1) : st.up(slot, v.data(), v.size());
        };
        auto* duri = arena(S_IN, uris);
        auto* dep = arena(S_AUX, eps);
        auto* dsh = arena(S_TAGS, shards);
        auto* dm = st.up(S_KEYS, meta.data(), meta.size());
        auto* dst = st.room(S_OK, n);
        enet_records r = records_of(n, nullptr, dooff, nullptr, dout, dm, dm + o_non);
        enet_announce_fields f{};
        f.manifests = f.endpoints = static_cast<std::uint32_t>(n);
        f.chunk_ids = dm + o_id;
        f.uris = duri;
        f.uri_offsets = doff;
        f.endpoint_bytes = dep;
        f.endpoint_offsets = doff + (n + 1);
        f.shards = dsh;
        f.shard_offsets = doff + 2 * (n + 1);
        f.peer_id = dm + o_pid;
        f.ttl = reinterpret_cast<const uint32_t*>(dm + o_ttl);
        f.versions = dm + o_ver;
        auto* dwn = reinterpret_cast<uint64_t*>(dm + o_wn);
        enet_check(enet_announce_frame_seal_batch(&r, nullptr, 0, nullptr, &f, difficulty, max_attempts, dwn, dst, st.s()),
                   "announce_frame_seal");
        std::vector<std::uint8_t> flat(obytes), status(n);
        SealedAnnounces res;
        res.work_nonce.resize(n);
        st.d2h(flat.data(), dout, obytes);
        st.d2h(res.work_nonce.data(), dwn, 8 * n);
        st.d2h(status.data(), dst, n);
        st.sync();
        res.frames.resize(n);
        res.status.resize(n);
        for (std::size_t i = 0; i < n; ++i) {
            res.status[i] = static_cast<AnnounceStatus>(status[i]);
            if (res.status[i] == AnnounceStatus::Ok) res.frames[i].assign(flat.begin() + ooff[i], flat.begin() + ooff[i + 1]);
        }
        return res;
    });
}

std::vector<OpenedAnnounce> announce_frames_open(Keys32 session_table, std::span<const std::uint32_t> session,
                                                 Records frames, std::span<const PeerId> peers, std::uint8_t difficulty) {
    const std::size_t n = frames.size(), K = session_table.size();
    check_sizes("announce_frames_open", n, {session.size(), peers.size()});
    check_count(n, "announce_frames_open");
    if (n == 0) return {};
    check_sessions(session, K, "announce_frames_open");
    const Packed in = pack(frames);
    const std::vector<std::uint64_t> ooff = offsets_of(frames, -48);
    // session keys | peers
    std::vector<std::uint8_t> meta(64 * n);
    gather_session_keys(meta, session_table, session);
    std::memcpy(meta.data() + 32 * n, peers.data()->data(), 32 * n);
    return staged([&](Staging& st) {
        const std::size_t obytes = ooff[n];
        auto* din = st.up(S_IN, in.arena.data(), in.arena.size());
        auto* dmsg = st.room(S_OUT, std::max<std::size_t>(obytes, 1));
        auto* dioff = st.up<uint64_t>(S_INOFF, in.off.data(), 8 * (n + 1));
        auto* dooff = st.up<uint64_t>(S_OUTOFF, ooff.data(), 8 * (n + 1));
        auto* dm = st.up(S_KEYS, meta.data(), meta.size());
        auto* dres = st.room(S_OK, 33 * n);  // info [n][8] uint32, then status [n]
        const enet_records r = records_of(n, dioff, dooff, din, dmsg, dm, nullptr);
        enet_check(enet_announce_frame_open_batch(&r, nullptr, 0, nullptr, dm + 32 * n, difficulty,
                                                  reinterpret_cast<uint32_t*>(dres), dres + 32 * n, st.s()),
                   "announce_frame_open");
        std::vector<std::uint8_t> msg(obytes), resv(33 * n);
        if (obytes) st.d2h(msg.data(), dmsg, obytes);
        st.d2h(resv.data(), dres, resv.size());
        st.sync();
        std::vector<OpenedAnnounce> res(n);
        for (std::size_t i = 0; i < n; ++i) {
            res[i].status = static_cast<AnnounceStatus>(resv[32 * n + i]);
            if (res[i].status != AnnounceStatus::Ok) {  // no field of a failed frame
                res[i].fields.version = 0;
                continue;
            }
            std::uint32_t info[8];
            std::memcpy(info, resv.data() + 32 * i, 32);
            const std::uint8_t* m = msg.data() + ooff[i];
            AnnounceFields& a = res[i].fields;
            a.version = static_cast<std::uint8_t>(info[0]);
            a.ttl_seconds = info[1];
            std::memcpy(a.chunk_id.data(), m + 18, 32);
            std::memcpy(a.peer_id.data(), m + 50, 32);
            const std::uint8_t* p = m + 82;
            a.endpoint.assign(p, p + info[2]);
            a.manifest_uri.assign(p + info[2], p + info[2] + info[3]);
            a.assigned_shards.assign(p + info[2] + info[3], p + info[2] + info[3] + info[4]);
            a.work_nonce = (static_cast<std::uint64_t>(info[6]) << 32) | info[5];
        }
        return res;
    });
}

// ---- Request / Acknowledge frames and triage (enet_control_frame_*_batch, enet_frame_classify_batch)
SealedControls control_frames_seal(Keys32 session_table, std::span<const std::uint32_t> session,
                                   std::span<const Nonce> nonces, std::span<const ControlFields> controls,
                                   const PeerId& local_id) {
    const std::size_t n = controls.size(), K = session_table.size();
    check_sizes("control_frames_seal", n, {session.size(), nonces.size()});
    check_count(n, "control_frames_seal");
    if (n == 0) return {};
    check_sessions(session, K, "control_frames_seal");
    std::vector<std::uint64_t> ooff(n + 1, 0);
    for (std::size_t i = 0; i < n; ++i) ooff[i + 1] = ooff[i] + (controls[i].kind == ControlKind::Request ? 114 : 115);
    // keys | chunk ids | frame nonces | local id | kinds | accepted | versions
    const std::size_t o_id = 32 * n, o_non = 64 * n, o_pid = 76 * n, o_kind = 76 * n + 32, o_acc = o_kind + n, o_ver = o_acc + n;
    std::vector<std::uint8_t> meta(79 * n + 32);
    gather_session_keys(meta, session_table, session);
    for (std::size_t i = 0; i < n; ++i) {
        std::memcpy(meta.data() + o_id + 32 * i, controls[i].chunk_id.data(), 32);
        meta[o_kind + i] = static_cast<std::uint8_t>(controls[i].kind);
        meta[o_acc + i] = controls[i].accepted ? 1 : 0;
        meta[o_ver + i] = controls[i].version;
    }
    std::memcpy(meta.data() + o_non, nonce_bytes(nonces), 12 * n);
    std::memcpy(meta.data() + o_pid, local_id.data(), 32);
    return staged([&](Staging& st) {
        const std::size_t obytes = ooff[n];
        auto* dout = st.room(S_OUT, obytes);
        auto* dooff = st.up<uint64_t>(S_OUTOFF, ooff.data(), 8 * (n + 1));
        auto* dm = st.up(S_KEYS, meta.data(), meta.size());
        auto* dst = st.room(S_OK, n);
        const enet_records r = records_of(n, nullptr, dooff, nullptr, dout, dm, dm + o_non);
        enet_check(enet_control_frame_seal_batch(&r, nullptr, 0, nullptr, dm + o_kind, dm + o_id, dm + o_pid, dm + o_acc, 0,
                                                 dm + o_ver, dst, st.s()),
                   "control_frame_seal");
        std::vector<std::uint8_t> flat(obytes), status(n);
        st.d2h(flat.data(), dout, obytes);
        st.d2h(status.data(), dst, n);
        st.sync();
        SealedControls res;
        res.frames.resize(n);
        res.status.resize(n);
        for (std::size_t i = 0; i < n; ++i) {
            res.status[i] = static_cast<ControlStatus>(status[i]);
            if (res.status[i] == ControlStatus::Ok) res.frames[i].assign(flat.begin() + ooff[i], flat.begin() + ooff[i + 1]);
        }
        return res;
    });
}

std::vector<OpenedControl> control_frames_open(Keys32 session_table, std::span<const std::uint32_t> session,
                                               Records frames, std::span<const PeerId> senders) {
    const std::size_t n = frames.size(), K = session_table.size();
    check_sizes("control_frames_open", n, {session.size(), optional_size(senders, n)});
    check_count(n, "control_frames_open");
    if (n == 0) return {};
    check_sessions(session, K, "control_frames_open");
    const Packed in = pack(frames);
    // session keys | senders
    std::vector<std::uint8_t> meta(64 * n);
    gather_session_keys(meta, session_table, session);
    if (!senders.empty()) std::memcpy(meta.data() + 32 * n, senders.data()->data(), 32 * n);
    return staged([&](Staging& st) {
        auto* din = st.up(S_IN, in.arena.data(), in.arena.size());
        auto* dioff = st.up<uint64_t>(S_INOFF, in.off.data(), 8 * (n + 1));
        auto* dm = st.up(S_KEYS, meta.data(), meta.size());
        auto* dres = st.room(S_OK, 69 * n);  // chunk ids [n][32], peer ids [n][32], info [n][4], status [n]
        const enet_records r = records_of(n, dioff, nullptr, din, nullptr, dm, nullptr);
        enet_check(enet_control_frame_open_batch(&r, nullptr, 0, nullptr, senders.empty() ? nullptr : dm + 32 * n, dres,
                                                 dres + 32 * n, dres + 64 * n, dres + 68 * n, st.s()),
                   "control_frame_open");
        std::vector<std::uint8_t> resv(69 * n);
        st.d2h(resv.data(), dres, resv.size());
        st.sync();
        std::vector<OpenedControl> res(n);
        for (std::size_t i = 0; i < n; ++i) {
            OpenedControl& c = res[i];
            const std::uint8_t* info = resv.data() + 64 * n + 4 * i;
            c.status = static_cast<ControlStatus>(resv[68 * n + i]);
            c.version = info[0];
            c.type = info[1];
            c.accepted = info[2] != 0;
            c.sender_match = info[3] != 0;
            std::memcpy(c.chunk_id.data(), resv.data() + 32 * i, 32);
            std::memcpy(c.peer_id.data(), resv.data() + 32 * n + 32 * i, 32);
        }
        return res;
    });
}

std::vector<FrameKind> classify_frames(Keys32 session_table, std::span<const std::uint32_t> session, Records frames) {
    const std::size_t n = frames.size(), K = session_table.size();
    check_sizes("classify_frames", n, {session.size()});
    check_count(n, "classify_frames");
    if (n == 0) return {};
    check_sessions(session, K, "classify_frames");
    const Packed in = pack(frames);
    std::vector<std::uint8_t> keys(32 * n);
    gather_session_keys(keys, session_table, session);
    return staged([&](Staging& st) {
        auto* din = st.up(S_IN, in.arena.data(), in.arena.size());
        auto* dioff = st.up<uint64_t>(S_INOFF, in.off.data(), 8 * (n + 1));
        auto* dk = st.up(S_KEYS, keys.data(), keys.size());
        auto* dlists = reinterpret_cast<uint32_t*>(st.room(S_OUT, 20 * n + 20));  // lists [5][n], counts [5]
        auto* dkind = st.room(S_OK, n);
        const enet_records r = records_of(n, dioff, nullptr, din, nullptr, dk, nullptr);
        enet_check(enet_frame_classify_batch(&r, nullptr, 0, dkind, dlists, dlists + 5 * n, st.s()), "frame_classify");
        std::vector<FrameKind> res(n);
        static_assert(sizeof(FrameKind) == 1);
        st.d2h(res.data(), dkind, n);
        st.sync();
        return res;
    });
}

// ------------------------------------------------------------------------------ proof of work
std::vector<PowResult> pow_search(Records prefixes, std::span<const std::uint8_t> difficulty, PowSchedule schedule,
                                  std::uint64_t max_attempts) {
    const size_t n = prefixes.size();
    check_sizes("pow_search", n, {difficulty.size()});
    if (n == 0) return {};
    return staged([&](Staging& st) {
        const Packed in = pack(prefixes);
        auto* din = st.up(S_IN, in.arena.data(), in.arena.size());
        auto* doff = st.up<uint64_t>(S_INOFF, in.off.data(), 8 * (n + 1));
        auto* dd = st.up(S_AUX, difficulty.data(), n);
        auto* dnonce = st.room<uint64_t>(S_OUT, 8 * n);
        auto* datt = st.room<uint64_t>(S_TAGS, 8 * n);
        auto* dfound = st.room(S_OK, n);
        enet_check(enet_pow_search_batch((uint32_t)n, din, doff, dd, static_cast<int>(schedule), max_attempts,
                                         dnonce, datt, dfound, st.s()),
                   "pow_search");
        std::vector<std::uint64_t> nonce(n), att(n);
        std::vector<std::uint8_t> found(n);
        st.d2h(nonce.data(), dnonce, 8 * n);
        st.d2h(att.data(), datt, 8 * n);
        st.d2h(found.data(), dfound, n);
        st.sync();
        std::vector<PowResult> res(n);
        for (size_t i = 0; i < n; ++i) res[i] = PowResult{found[i] != 0, nonce[i], att[i]};
        return res;
    });
}

std::vector<std::uint8_t> pow_check(Records prefixes, std::span<const std::uint64_t> nonces,
                                    std::span<const std::uint8_t> difficulty) {
    const size_t n = prefixes.size();
    check_sizes("pow_check", n, {difficulty.size(), nonces.size()});
    if (n == 0) return {};
    return staged([&](Staging& st) {
        const Packed in = pack(prefixes);
        auto* din = st.up(S_IN, in.arena.data(), in.arena.size());
        auto* doff = st.up<uint64_t>(S_INOFF, in.off.data(), 8 * (n + 1));
        auto* dd = st.up(S_AUX, difficulty.data(), n);
        auto* dnonce = st.up<uint64_t>(S_CTR, nonces.data(), 8 * n);
        auto* dok = st.room(S_OK, n);
        enet_check(enet_pow_check_batch((uint32_t)n, din, doff, dnonce, dd, dok, st.s()), "pow_check");
        std::vector<std::uint8_t> ok(n);
        st.d2h(ok.data(), dok, n);
        st.sync();
        return ok;
    });
}

namespace {
void put_lp64(std::vector<std::uint8_t>& v, const std::uint8_t* p, std::size_t n) {  // Node.cpp:149-153
    put_be64(std::back_inserter(v), n);
    v.insert(v.end(), p, p + n);
}
}  // namespace

std::vector<std::uint8_t> announce_pow_prefix(const ChunkId& chunk_id, const PeerId& peer_id,
                                              std::string_view endpoint, std::string_view manifest_uri,
                                              std::span<const std::uint8_t> assigned_shards,
                                              std::int64_t ttl_seconds) {
    std::vector<std::uint8_t> v;
    v.reserve(120 + endpoint.size() + manifest_uri.size() + assigned_shards.size());
    put_lp64(v, chunk_id.data(), chunk_id.size());
    put_lp64(v, peer_id.data(), peer_id.size());
    put_lp64(v, reinterpret_cast<const std::uint8_t*>(endpoint.data()), endpoint.size());
    put_lp64(v, reinterpret_cast<const std::uint8_t*>(manifest_uri.data()), manifest_uri.size());
    put_lp64(v, assigned_shards.data(), assigned_shards.size());
    put_be64(std::back_inserter(v), static_cast<std::uint64_t>(ttl_seconds));  // Node.cpp:165-166
    return v;
}

std::vector<std::uint8_t> handshake_pow_prefix(const PeerId& initiator, const PeerId& responder,
                                               std::uint32_t initiator_public) {
    std::vector<std::uint8_t> v;
    v.reserve(88);
    put_lp64(v, initiator.data(), initiator.size());
    put_lp64(v, responder.data(), responder.size());
    put_be64(std::back_inserter(v), static_cast<std::uint64_t>(initiator_public));  // Node.cpp:241-242
    return v;
}

// ------------------------------------------------------------------------------ sessions
std::vector<std::array<std::uint8_t, 32>> session_keys(std::span<const Key> secrets,
                                                       std::span<const std::uint64_t> counters,
                                                       std::span<const std::int64_t> ticks) {
    const size_t n = secrets.size();
    check_sizes("session_keys", n, {counters.size(), ticks.size()});
    if (n == 0) return {};
    return staged([&](Staging& st) {
        auto* dk = st.up(S_KEYS, key_bytes(secrets), 32 * n);
        auto* dc = st.up<uint64_t>(S_CTR, counters.data(), 8 * n);
        auto* dt = st.up<int64_t>(S_NONCES, ticks.data(), 8 * n);
        auto* dout = st.room(S_OUT, 32 * n);
        enet_check(enet_session_key_batch((uint32_t)n, dk, dc, dt, dout, st.s()), "session_keys");
        std::vector<std::array<std::uint8_t, 32>> res(n);
        st.d2h(res.data(), dout, 32 * n);
        st.sync();
        return res;
    });
}

KeyExchangeResult key_exchange(std::span<const std::uint32_t> privates, std::span<const std::uint32_t> remotes) {
    const size_t n = privates.size();
    check_sizes("key_exchange", n, {optional_size(remotes, n)});
    KeyExchangeResult res;
    if (n == 0) return res;
    return staged([&](Staging& st) {
        const bool secrets = !remotes.empty();
        auto* dp = st.up<uint32_t>(S_IN, privates.data(), 4 * n);
        auto* dr = secrets ? st.up<uint32_t>(S_KEYS, remotes.data(), 4 * n) : nullptr;
        auto* dpub = st.room<uint32_t>(S_OUT, 4 * n);
        auto* dsec = secrets ? st.room(S_AUX, 32 * n) : nullptr;
        enet_check(enet_key_exchange_batch((uint32_t)n, dp, dr, dpub, dsec, st.s()), "key_exchange");
        res.publics.resize(n);
        st.d2h(res.publics.data(), dpub, 4 * n);
        if (secrets) {
            res.secrets.resize(n);
            st.d2h(res.secrets.data(), dsec, 32 * n);
        }
        st.sync();
        return res;
    });
}

std::vector<HandshakeResult> handshake_accept(const PeerId& local_id, std::uint32_t local_private,
                                              std::uint8_t difficulty, std::chrono::steady_clock::time_point now,
                                              std::span<const HandshakeRequest> requests) {
    const size_t n = requests.size();
    std::vector<HandshakeResult> res(n);
    if (n == 0) return res;
    // 5^local_private mod 2^31-1 (KeyExchange::compute_public), one scalar on the host
    std::uint64_t local_public = 1, base = 5;
    for (std::uint32_t e = local_private; e != 0; e >>= 1) {
        if (e & 1u) local_public = local_public * base % 2147483647ull;
        base = base * base % 2147483647ull;
    }
    return staged([&](Staging& st) {
        // inputs: peer ids [n][32] | nonces [n] u64 | publics [n] u32 | local id [32]
        std::vector<uint8_t> in(44 * n + 32);
        for (size_t i = 0; i < n; ++i) {
            std::memcpy(in.data() + 32 * i, requests[i].peer_id.data(), 32);
            std::memcpy(in.data() + 32 * n + 8 * i, &requests[i].work_nonce, 8);
            std::memcpy(in.data() + 40 * n + 4 * i, &requests[i].remote_public, 4);
        }
        std::memcpy(in.data() + 44 * n, local_id.data(), 32);
        auto* din = st.up(S_IN, in.data(), in.size());
        // the call's table, slot i for request i: secrets | keys | mid | counters | last_rotation | live
        auto* dt = st.room(S_OUT, 145 * n);
        auto* dv = st.room(S_OK, n);
        enet_session_table t{};
        t.sessions = (uint32_t)n;
        t.secrets = dt;
        t.keys = dt + 32 * n;
        t.mid = (uint32_t*)(dt + 64 * n);
        t.counters = (uint64_t*)(dt + 128 * n);
        t.last_rotation = (int64_t*)(dt + 136 * n);
        t.live = dt + 144 * n;
        const auto ticks = std::chrono::duration_cast<std::chrono::nanoseconds>(now.time_since_epoch()).count();
        enet_check(enet_handshake_accept_batch(&t, (uint32_t)n, din, (const uint32_t*)(din + 40 * n),
                                               (const uint64_t*)(din + 32 * n), nullptr, din + 44 * n, local_private,
                                               (uint32_t)local_public, difficulty, ticks, dv, st.s()),
                   "handshake_accept");
        std::vector<uint8_t> verdict(n), rows(64 * n);
        st.d2h(verdict.data(), dv, n);
        st.d2h(rows.data(), dt, 64 * n);
        st.sync();
        for (size_t i = 0; i < n; ++i) {
            res[i].verdict = (HandshakeVerdict)verdict[i];
            if (verdict[i] != ENET_HS_OK) continue;  // rejected slots were never written
            std::memcpy(res[i].shared_secret.bytes.data(), rows.data() + 32 * i, 32);
            std::memcpy(res[i].session_key.data(), rows.data() + 32 * n + 32 * i, 32);
        }
        return res;
    });
}

}  // namespace ephemeralnet::crypto::batch

// ------------------------------------------------------------------------------ security::StoreProof batches
namespace ephemeralnet::security {

std::vector<std::uint8_t> store_pow_prefix(const StoreWorkInput& input) {
    std::vector<std::uint8_t> v(input.chunk_id.begin(), input.chunk_id.end());
    enet::api::put_be64(std::back_inserter(v), input.payload_size);
    enet::api::put_be32(std::back_inserter(v),
                        static_cast<std::uint32_t>(std::min<std::size_t>(input.filename_hint.size(),
                                                                         std::numeric_limits<std::uint32_t>::max())));
    v.insert(v.end(), input.filename_hint.begin(), input.filename_hint.end());
    return v;
}

namespace batch {
namespace {
// every input's PoW prefix and the views the crypto::batch PoW calls take
struct Prefixes {
    std::vector<std::vector<std::uint8_t>> bytes;
    std::vector<std::span<const std::uint8_t>> views;
    explicit Prefixes(std::span<const StoreWorkInput> inputs) : bytes(all(inputs)), views(bytes.begin(), bytes.end()) {}
    static std::vector<std::vector<std::uint8_t>> all(std::span<const StoreWorkInput> inputs) {
        std::vector<std::vector<std::uint8_t>> pre;
        pre.reserve(inputs.size());
        for (const auto& in : inputs) pre.push_back(store_pow_prefix(in));
        return pre;
    }
};
}  // namespace

std::vector<std::optional<std::uint64_t>> compute_store_pow(std::span<const StoreWorkInput> inputs,
                                                            std::uint8_t difficulty_bits,
                                                            std::uint64_t max_attempts) {
    std::vector<std::optional<std::uint64_t>> res(inputs.size());
    if (inputs.empty()) return res;
    if (difficulty_bits == 0) {  // StoreProof.cpp:125-127
        for (auto& r : res) r = std::uint64_t{0};
        return res;
    }
    if (max_attempts == 0) max_attempts = kDefaultStorePowMaxAttempts;  // :131-133
    const Prefixes pre(inputs);
    const std::vector<std::uint8_t> diffs(inputs.size(), enet::api::clamp_store_difficulty(difficulty_bits));
    auto r = crypto::batch::pow_search(pre.views, diffs, crypto::batch::PowSchedule::Store, max_attempts);
    for (size_t i = 0; i < r.size(); ++i)
        if (r[i].found) res[i] = r[i].nonce;
    return res;
}

std::vector<std::uint8_t> store_pow_valid(std::span<const StoreWorkInput> inputs,
                                          std::span<const std::uint64_t> nonces,
                                          std::uint8_t difficulty_bits) {
    if (nonces.size() != inputs.size()) throw std::invalid_argument("enet store_pow_valid: size mismatch");
    if (difficulty_bits == 0) return std::vector<std::uint8_t>(inputs.size(), 1);  // :112-113
    const Prefixes pre(inputs);
    const std::vector<std::uint8_t> diffs(inputs.size(), enet::api::clamp_store_difficulty(difficulty_bits));
    return crypto::batch::pow_check(pre.views, nonces, diffs);
}
}  // namespace batch

}  // namespace ephemeralnet::security
