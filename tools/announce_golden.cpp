// announce_golden.cpp -- driver of tools/gen_announce_golden.py: runs the REFERENCE's
// protocol::encode_signed / decode_signed, HmacSha256, ChaCha20, Sha256 and encode_manifest
// (compiled from the reference checkout where it lies, never copied here) on the operations it
// reads from stdin, one per line, and prints one result line each ("-" stands for an empty hex
// string in both directions):
//   encode <version> <ttl> <chunk_id> <peer_id> <endpoint> <uri> <shards> <nonce> <key>
//                                         -> encode_signed of that Announce, hex
//   decode <signed> <key>                 -> decode_signed: "none", "other <type>", or
//                                            "announce <version> <ttl> <chunk_id> <peer_id> <endpoint>
//                                            <uri> <shards> <nonce>"
//   sign <message> <key>                  -> message || HmacSha256::compute(key, message), hex
//   chacha <key> <nonce> <data>           -> ChaCha20::apply from counter 0, hex
//   sha <message>                         -> Sha256::digest, hex
//   manifest <chunk_id> <chunk_hash> <nonce> <threshold> <total> <expires s> <shard values>
//                                         -> encode_manifest of a manifest with shards 1..total
//                                            (32-byte values cut from <shard values>), no metadata,
//                                            no hints; the URI as hex
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <span>
#include <sstream>
#include <string>
#include <variant>
#include <vector>

#include "ephemeralnet/crypto/ChaCha20.hpp"
#include "ephemeralnet/crypto/HmacSha256.hpp"
#include "ephemeralnet/crypto/Sha256.hpp"
#include "ephemeralnet/protocol/Manifest.hpp"
#include "ephemeralnet/protocol/Message.hpp"

using namespace ephemeralnet;

static std::vector<std::uint8_t> unhex(const std::string& s) {
    std::vector<std::uint8_t> v;
    if (s == "-") return v;
    for (std::size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((std::uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return v;
}

template <class A>
static std::string hex(const A& a) {
    std::string out;
    char buf[3];
    for (auto b : a) {
        std::snprintf(buf, sizeof buf, "%02x", (unsigned)(std::uint8_t)b);
        out += buf;
    }
    return out.empty() ? "-" : out;
}

template <class A>
static A array_of(const std::string& h) {
    A a{};
    const auto v = unhex(h);
    for (std::size_t i = 0; i < a.size() && i < v.size(); ++i) a[i] = v[i];
    return a;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        if (op == "encode") {
            unsigned version = 0;
            std::uint64_t ttl = 0, nonce = 0;
            std::string cid, pid, ep, uri, sh, key;
            in >> version >> ttl >> cid >> pid >> ep >> uri >> sh >> nonce >> key;
            protocol::AnnouncePayload p{};
            p.chunk_id = array_of<ChunkId>(cid);
            p.peer_id = array_of<PeerId>(pid);
            const auto e = unhex(ep), u = unhex(uri);
            p.endpoint.assign(e.begin(), e.end());
            p.manifest_uri.assign(u.begin(), u.end());
            p.assigned_shards = unhex(sh);
            p.ttl = std::chrono::seconds(ttl);
            p.work_nonce = nonce;
            protocol::Message m{};
            m.version = (std::uint8_t)version;
            m.type = protocol::MessageType::Announce;
            m.payload = p;
            const auto k = unhex(key);
            std::cout << hex(protocol::encode_signed(m, std::span<const std::uint8_t>(k))) << "\n";
        } else if (op == "decode") {
            std::string sg, key;
            in >> sg >> key;
            const auto s = unhex(sg), k = unhex(key);
            const auto m = protocol::decode_signed(std::span<const std::uint8_t>(s), std::span<const std::uint8_t>(k));
            if (!m) {
                std::cout << "none\n";
            } else if (const auto* p = std::get_if<protocol::AnnouncePayload>(&m->payload)) {
                std::cout << "announce " << (unsigned)m->version << " " << p->ttl.count() << " " << hex(p->chunk_id) << " "
                          << hex(p->peer_id) << " " << hex(p->endpoint) << " " << hex(p->manifest_uri) << " "
                          << hex(p->assigned_shards) << " " << p->work_nonce << "\n";
            } else {
                std::cout << "other " << (unsigned)m->type << "\n";
            }
        } else if (op == "sign") {
            std::string msg, key;
            in >> msg >> key;
            auto m = unhex(msg);
            const auto k = unhex(key);
            const auto mac = crypto::HmacSha256::compute(std::span<const std::uint8_t>(k), std::span<const std::uint8_t>(m));
            m.insert(m.end(), mac.begin(), mac.end());
            std::cout << hex(m) << "\n";
        } else if (op == "chacha") {
            std::string key, nonce, data;
            in >> key >> nonce >> data;
            crypto::Key k{};
            k.bytes = array_of<std::array<std::uint8_t, 32>>(key);
            crypto::Nonce n{};
            n.bytes = array_of<std::array<std::uint8_t, 12>>(nonce);
            const auto d = unhex(data);
            std::vector<std::uint8_t> out;
            crypto::ChaCha20::apply(k, n, std::span<const std::uint8_t>(d), out, 0);
            std::cout << hex(out) << "\n";
        } else if (op == "sha") {
            std::string msg;
            in >> msg;
            const auto m = unhex(msg);
            std::cout << hex(crypto::Sha256::digest(std::span<const std::uint8_t>(m))) << "\n";
        } else if (op == "manifest") {
            std::string cid, hash, nonce, values;
            unsigned threshold = 0, total = 0;
            std::int64_t expires = 0;
            in >> cid >> hash >> nonce >> threshold >> total >> expires >> values;
            protocol::Manifest mf{};
            mf.chunk_id = array_of<ChunkId>(cid);
            mf.chunk_hash = array_of<std::array<std::uint8_t, 32>>(hash);
            mf.nonce.bytes = array_of<std::array<std::uint8_t, 12>>(nonce);
            mf.threshold = (std::uint8_t)threshold;
            mf.total_shares = (std::uint8_t)total;
            mf.expires_at = std::chrono::system_clock::time_point{} + std::chrono::seconds(expires);
            const auto v = unhex(values);
            for (unsigned i = 0; i < total; ++i) {
                protocol::KeyShard s{};
                s.index = (std::uint8_t)(i + 1);
                for (std::size_t b = 0; b < 32 && 32 * i + b < v.size(); ++b) s.value[b] = v[32 * i + b];
                mf.shards.push_back(s);
            }
            std::cout << hex(protocol::encode_manifest(mf)) << "\n";
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}
