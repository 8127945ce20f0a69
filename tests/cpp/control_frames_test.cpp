// control_frames_test.cpp -- crypto::batch::control_frames_seal / control_frames_open /
// classify_frames over host vectors, as a node's transfer paths would call them
// (Node::request_chunk, Node::handle_chunk, the receive loop).  Reads one operation per line from
// stdin ("-" = an empty hex string):
//   seal <key> <frame nonce> <kind> <version> <accepted> <chunk_id> <local id>
//        -> all seal lines of one local id go into ONE call after the input ends; per line, in
//           input order, "<status> <frame hex>"
//   open <key> <sender> <frame>   -> all open lines go into ONE open call and ONE classify call;
//        per line "<status> <version> <type> <accepted> <chunk_id> <peer_id> <sender_match> <kind>"
//   args                          -> the argument checks, which run before any device call: one
//        "<label> | <what() or result>" line each
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

struct SealLine {
    size_t at;
    std::array<uint8_t, 32> key;
    crypto::Nonce nonce;
    B::ControlFields fields;
};
struct OpenLine {
    size_t at;
    std::array<uint8_t, 32> key;
    PeerId sender;
    std::vector<uint8_t> frame;
};

int main() {
    std::vector<std::string> out;
    std::map<std::string, std::vector<SealLine>> seals;
    std::vector<OpenLine> opens;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        if (op == "seal") {
            unsigned kind = 0, version = 0, accepted = 0;
            std::string key, fn, cid, local;
            in >> key >> fn >> kind >> version >> accepted >> cid >> local;
            SealLine s{out.size(), array_of<std::array<uint8_t, 32>>(key), {}, {}};
            s.nonce.bytes = array_of<std::array<uint8_t, 12>>(fn);
            s.fields.kind = static_cast<B::ControlKind>(kind);
            s.fields.version = (uint8_t)version;
            s.fields.accepted = accepted != 0;
            s.fields.chunk_id = array_of<ChunkId>(cid);
            seals[local].push_back(s);
            out.emplace_back();
        } else if (op == "open") {
            std::string key, sender, frame;
            in >> key >> sender >> frame;
            opens.push_back({out.size(), array_of<std::array<uint8_t, 32>>(key), array_of<PeerId>(sender), unhex(frame)});
            out.emplace_back();
        } else if (op == "args") {
            const std::vector<std::array<uint8_t, 32>> table(2);
            const std::vector<uint32_t> s1 = {0}, s2 = {0, 1}, far = {0, 2}, none;
            const std::vector<crypto::Nonce> n2(2), n0;
            const std::vector<B::ControlFields> c2(2), c0;
            const std::vector<PeerId> p1(1), p0;
            const PeerId local{};
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
            thrown("mismatch seal", [&] { (void)B::control_frames_seal(table, s1, n2, c2, local); });
            thrown("mismatch seal nonces", [&] { (void)B::control_frames_seal(table, s2, n0, c2, local); });
            thrown("mismatch open", [&] { (void)B::control_frames_open(table, s1, f2); });
            thrown("mismatch open senders", [&] { (void)B::control_frames_open(table, s2, f2, p1); });
            thrown("mismatch classify", [&] { (void)B::classify_frames(table, s1, f2); });
            thrown("session seal", [&] { (void)B::control_frames_seal(table, far, n2, c2, local); });
            thrown("session open", [&] { (void)B::control_frames_open(table, far, f2); });
            thrown("session classify", [&] { (void)B::classify_frames(table, far, f2); });
            out.push_back(std::string("empty seal | ") + (B::control_frames_seal(table, none, n0, c0, local).frames.empty() ? "empty" : "?"));
            out.push_back(std::string("empty open | ") + (B::control_frames_open(table, none, f0, p0).empty() ? "empty" : "?"));
            out.push_back(std::string("empty classify | ") + (B::classify_frames(table, none, f0).empty() ? "empty" : "?"));
        }
    }
    for (const auto& [local, ls] : seals) {
        // one session per frame, named in reverse so the table lookup is exercised
        std::vector<std::array<uint8_t, 32>> table(ls.size());
        std::vector<uint32_t> session(ls.size());
        std::vector<crypto::Nonce> nonces;
        std::vector<B::ControlFields> fields;
        for (size_t i = 0; i < ls.size(); ++i) {
            session[i] = (uint32_t)(ls.size() - 1 - i);
            table[session[i]] = ls[i].key;
            nonces.push_back(ls[i].nonce);
            fields.push_back(ls[i].fields);
        }
        const auto r = B::control_frames_seal(table, session, nonces, fields, array_of<PeerId>(local));
        for (size_t i = 0; i < ls.size(); ++i) out[ls[i].at] = std::to_string((int)r.status[i]) + " " + hex(r.frames[i]);
    }
    if (!opens.empty()) {
        std::vector<std::array<uint8_t, 32>> table(opens.size());
        std::vector<uint32_t> session(opens.size());
        std::vector<PeerId> senders;
        std::vector<std::span<const uint8_t>> frames;
        for (size_t i = 0; i < opens.size(); ++i) {
            session[i] = (uint32_t)(opens.size() - 1 - i);
            table[session[i]] = opens[i].key;
            senders.push_back(opens[i].sender);
            frames.emplace_back(opens[i].frame);
        }
        const auto r = B::control_frames_open(table, session, frames, senders);
        const auto k = B::classify_frames(table, session, frames);
        for (size_t i = 0; i < opens.size(); ++i) {
            out[opens[i].at] = std::to_string((int)r[i].status) + " " + std::to_string((int)r[i].version) + " " +
                               std::to_string((int)r[i].type) + " " + std::to_string((int)r[i].accepted) + " " +
                               hex(r[i].chunk_id) + " " + hex(r[i].peer_id) + " " + std::to_string((int)r[i].sender_match) +
                               " " + std::to_string((int)k[i]);
        }
    }
    for (const auto& l : out) std::cout << l << "\n";
    return 0;
}
