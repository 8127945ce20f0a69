// announce_frames_test.cpp -- crypto::batch::announce_frames_seal / announce_frames_open over host
// vectors, as a node's gossip paths would call them (Node::deliver_manifest, Node::handle_announce).
// Reads one operation per line from stdin ("-" = an empty hex string):
//   seal <difficulty> <max_attempts> <key> <frame nonce> <version> <ttl> <chunk_id> <peer_id>
//        <endpoint> <uri> <shards> <work_nonce>      -> one call; "<status> <work_nonce> <frame hex>"
//   open <difficulty> <key> <peer> <frame>           -> all open lines of one difficulty go into ONE
//        call after the input ends; per line, in input order, "<status> <version> <ttl> <chunk_id>
//        <peer_id> <endpoint> <uri> <shards> <work_nonce>"
//   args                                             -> the argument checks, which run before any
//        device call: one "<label> | <what() or result>" line each
#include <iostream>
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "ephemeralnet/crypto/Batch.hpp"

using namespace ephemeralnet;
namespace B = crypto::batch;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    if (s == "-") return v;
    for (size_t i = 0; i + 1 < s.size(); i += 2) v.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return v;
}

template <class A>
static std::string hex(const A& a) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (auto c : a) { s += d[(uint8_t)c >> 4]; s += d[(uint8_t)c & 15]; }
    return s.empty() ? "-" : s;
}

template <class A>
static A array_of(const std::string& h) {
    A a{};
    const auto v = unhex(h);
    for (size_t i = 0; i < a.size() && i < v.size(); ++i) a[i] = v[i];
    return a;
}

struct OpenLine {
    size_t at;
    std::array<uint8_t, 32> key;
    PeerId peer;
    std::vector<uint8_t> frame;
};

int main() {
    std::vector<std::string> out;
    std::map<unsigned, std::vector<OpenLine>> opens;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        if (op == "seal") {
            unsigned difficulty = 0, version = 0;
            uint64_t max_attempts = 0, nonce = 0;
            uint32_t ttl = 0;
            std::string key, fn, cid, pid, ep, uri, sh;
            in >> difficulty >> max_attempts >> key >> fn >> version >> ttl >> cid >> pid >> ep >> uri >> sh >> nonce;
            B::AnnounceFields a;
            a.chunk_id = array_of<ChunkId>(cid);
            a.peer_id = array_of<PeerId>(pid);
            const auto e = unhex(ep), u = unhex(uri);
            a.endpoint.assign(e.begin(), e.end());
            a.manifest_uri.assign(u.begin(), u.end());
            a.assigned_shards = unhex(sh);
            a.ttl_seconds = ttl;
            a.version = (uint8_t)version;
            a.work_nonce = nonce;
            const std::vector<std::array<uint8_t, 32>> table = {array_of<std::array<uint8_t, 32>>(key)};
            const std::vector<uint32_t> session = {0};
            crypto::Nonce n{};
            n.bytes = array_of<std::array<uint8_t, 12>>(fn);
            const std::vector<crypto::Nonce> nonces = {n};
            const std::vector<B::AnnounceFields> as = {a};
            const auto r = B::announce_frames_seal(table, session, nonces, as, (uint8_t)difficulty, max_attempts);
            out.push_back(std::to_string((int)r.status[0]) + " " + std::to_string(r.work_nonce[0]) + " " + hex(r.frames[0]));
        } else if (op == "args") {
            const std::vector<std::array<uint8_t, 32>> table(2);
            const std::vector<uint32_t> s1 = {0}, s2 = {0, 1}, far = {0, 2}, none;
            const std::vector<crypto::Nonce> n2(2), n0;
            std::vector<B::AnnounceFields> a2(2), a0;
            const std::vector<PeerId> p1(1), p0;
            const std::vector<uint8_t> fr(48);
            const std::vector<std::span<const uint8_t>> f2 = {fr, fr}, f0;
            auto thrown = [&](const char* label, auto&& call) {
                try {
                    call();
                    out.push_back(std::string(label) + " | no exception");
                } catch (const std::invalid_argument& e) {
                    out.push_back(std::string(label) + " | " + e.what());
                }
            };
            thrown("mismatch seal", [&] { (void)B::announce_frames_seal(table, s1, n2, a2, 6); });
            thrown("mismatch open", [&] { (void)B::announce_frames_open(table, s2, f2, p1, 6); });
            thrown("session seal", [&] { (void)B::announce_frames_seal(table, far, n2, a2, 6); });
            thrown("session open", [&] { (void)B::announce_frames_open(table, far, f2, std::vector<PeerId>(2), 6); });
            a2[1].peer_id[0] = 1;
            thrown("peers seal", [&] { (void)B::announce_frames_seal(table, s2, n2, a2, 6); });
            out.push_back(std::string("empty seal | ") + (B::announce_frames_seal(table, none, n0, a0, 6).frames.empty() ? "empty" : "?"));
            out.push_back(std::string("empty open | ") + (B::announce_frames_open(table, none, f0, p0, 6).empty() ? "empty" : "?"));
        } else if (op == "open") {
            unsigned difficulty = 0;
            std::string key, peer, frame;
            in >> difficulty >> key >> peer >> frame;
            opens[difficulty].push_back({out.size(), array_of<std::array<uint8_t, 32>>(key), array_of<PeerId>(peer), unhex(frame)});
            out.emplace_back();
        }
    }
    for (const auto& [difficulty, ls] : opens) {
        // one session per frame, named in reverse so the table lookup is exercised
        std::vector<std::array<uint8_t, 32>> table(ls.size());
        std::vector<uint32_t> session(ls.size());
        std::vector<PeerId> peers;
        std::vector<std::span<const uint8_t>> frames;
        for (size_t i = 0; i < ls.size(); ++i) {
            session[i] = (uint32_t)(ls.size() - 1 - i);
            table[session[i]] = ls[i].key;
            peers.push_back(ls[i].peer);
            frames.emplace_back(ls[i].frame);
        }
        const auto r = B::announce_frames_open(table, session, frames, peers, (uint8_t)difficulty);
        for (size_t i = 0; i < ls.size(); ++i) {
            const auto& a = r[i].fields;
            out[ls[i].at] = std::to_string((int)r[i].status) + " " + std::to_string((int)a.version) + " " +
                            std::to_string(a.ttl_seconds) + " " + hex(a.chunk_id) + " " + hex(a.peer_id) + " " +
                            hex(a.endpoint) + " " + hex(a.manifest_uri) + " " + hex(a.assigned_shards) + " " +
                            std::to_string(a.work_nonce);
        }
    }
    for (const auto& l : out) std::cout << l << "\n";
    return 0;
}
