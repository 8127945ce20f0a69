// handshake_golden.cpp -- driver of tools/gen_handshake_golden.py: runs the REFERENCE's
// KeyExchange, KeyManager and Sha256 (compiled from the reference checkout where it lies, never
// copied here) on the operations it reads from stdin, one per line, and prints one result line each:
//   public <private>                               -> KeyExchange::compute_public
//   valid <public>                                 -> KeyExchange::validate_public, 0 / 1
//   secret <private> <remote public>               -> derive_shared_secret, hex
//   material <secret hex> <material hex>           -> current_key after register_session_with_material
//   rotate <secret hex> <registered ns> <now ns>   -> rotate_if_needed with a 1 s interval, hex or "none"
//   sha <message hex>                              -> Sha256::digest, hex ("-" = empty message)
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <span>
#include <sstream>
#include <string>
#include <vector>

#include "ephemeralnet/crypto/Sha256.hpp"
#include "ephemeralnet/network/KeyExchange.hpp"
#include "ephemeralnet/network/KeyManager.hpp"

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
        std::snprintf(buf, sizeof buf, "%02x", (unsigned)b);
        out += buf;
    }
    return out;
}

static crypto::Key key_of(const std::string& h) {
    crypto::Key k{};
    const auto v = unhex(h);
    for (std::size_t i = 0; i < 32 && i < v.size(); ++i) k.bytes[i] = v[i];
    return k;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        in >> op;
        if (op == "public") {
            std::uint32_t priv = 0;
            in >> priv;
            std::cout << network::KeyExchange::compute_public(priv) << "\n";
        } else if (op == "valid") {
            std::uint32_t pub = 0;
            in >> pub;
            std::cout << (network::KeyExchange::validate_public(pub) ? 1 : 0) << "\n";
        } else if (op == "secret") {
            std::uint32_t priv = 0, remote = 0;
            in >> priv >> remote;
            std::cout << hex(network::KeyExchange::derive_shared_secret(priv, remote).bytes) << "\n";
        } else if (op == "material" || op == "rotate") {
            std::string secret;
            in >> secret;
            PeerId peer{};
            peer[0] = 1;
            network::KeyManager km(std::chrono::seconds(1));
            const auto epoch = std::chrono::steady_clock::time_point{};
            if (op == "material") {
                std::string material;
                in >> material;
                const auto m = unhex(material);
                km.register_session_with_material(peer, key_of(secret), std::span<const std::uint8_t>(m), epoch);
                std::cout << hex(*km.current_key(peer)) << "\n";
            } else {
                std::int64_t registered = 0, now = 0;
                in >> registered >> now;
                const std::array<std::uint8_t, 8> m{};
                km.register_session_with_material(peer, key_of(secret), std::span<const std::uint8_t>(m),
                                                  epoch + std::chrono::nanoseconds(registered));
                const auto key = km.rotate_if_needed(peer, epoch + std::chrono::nanoseconds(now));
                std::cout << (key ? hex(*key) : std::string("none")) << "\n";
            }
        } else if (op == "sha") {
            std::string msg;
            in >> msg;
            const auto m = unhex(msg);
            std::cout << hex(crypto::Sha256::digest(std::span<const std::uint8_t>(m))) << "\n";
        } else {
            std::cout << "?\n";
        }
    }
    return 0;
}
