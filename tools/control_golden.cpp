// control_golden.cpp -- driver of tools/gen_control_golden.py: runs the REFERENCE's
// protocol::encode_signed / decode_signed, HmacSha256 and ChaCha20 (compiled from the reference
// checkout where it lies, never copied here) on the operations it reads from stdin, one per line,
// and prints one result line each:
//   request <version> <chunk_id> <requester> <key>        -> encode_signed of that Request, hex
//   ack <version> <accepted> <chunk_id> <peer_id> <key>   -> encode_signed of that Acknowledge, hex
//   decode <signed> <key>     -> decode_signed: "none", "other <type>",
//                                "request <version> <chunk_id> <requester>" or
//                                "ack <version> <accepted> <chunk_id> <peer_id>"
//   sign <message> <key>      -> message || HmacSha256::compute(key, message), hex
//   chacha <key> <nonce> <data> -> ChaCha20::apply from counter 0, hex
#include <array>
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
        if (op == "request" || op == "ack") {
            unsigned version = 0, accepted = 0;
            std::string cid, pid, key;
            in >> version;
            if (op == "ack") in >> accepted;
            in >> cid >> pid >> key;
            protocol::Message m{};
            m.version = (std::uint8_t)version;
            if (op == "request") {
                protocol::RequestPayload p{};
                p.chunk_id = array_of<ChunkId>(cid);
                p.requester = array_of<PeerId>(pid);
                m.type = protocol::MessageType::Request;
                m.payload = p;
            } else {
                protocol::AcknowledgePayload p{};
                p.chunk_id = array_of<ChunkId>(cid);
                p.peer_id = array_of<PeerId>(pid);
                p.accepted = accepted != 0;
                m.type = protocol::MessageType::Acknowledge;
                m.payload = p;
            }
            const auto k = unhex(key);
            std::cout << hex(protocol::encode_signed(m, std::span<const std::uint8_t>(k))) << "\n";
        } else if (op == "decode") {
            std::string sg, key;
            in >> sg >> key;
            const auto s = unhex(sg), k = unhex(key);
            const auto m = protocol::decode_signed(std::span<const std::uint8_t>(s), std::span<const std::uint8_t>(k));
            if (!m) {
                std::cout << "none\n";
            } else if (const auto* p = std::get_if<protocol::RequestPayload>(&m->payload)) {
                std::cout << "request " << (unsigned)m->version << " " << hex(p->chunk_id) << " " << hex(p->requester) << "\n";
            } else if (const auto* a = std::get_if<protocol::AcknowledgePayload>(&m->payload)) {
                std::cout << "ack " << (unsigned)m->version << " " << (a->accepted ? 1 : 0) << " " << hex(a->chunk_id) << " "
                          << hex(a->peer_id) << "\n";
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
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}
