// handshake_api_test.cpp -- crypto::batch::key_exchange / handshake_accept on the device
// (tests/test_gpu_handshake.py compares the output with tests/golden/handshake.json and the
// restatement).  Reads blocks from stdin and prints one line per record:
//   kx <n> <secrets|nosecrets>      then n lines "<private> <remote public>"
//       -> "<public> <secret hex>"  ("<public> -" without remotes)
//   accept <local id hex> <local private> <difficulty> <now ns> <n>
//                                   then n lines "<peer id hex> <remote public> <work nonce>"
//       -> "<verdict> <shared secret hex> <session key hex>"
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "ephemeralnet/crypto/Batch.hpp"

using namespace ephemeralnet;
using namespace ephemeralnet::crypto;

static std::array<std::uint8_t, 32> unhex32(const std::string& s) {
    std::array<std::uint8_t, 32> a{};
    for (int i = 0; i < 32; ++i) a[i] = (std::uint8_t)std::stoul(s.substr(2 * i, 2), nullptr, 16);
    return a;
}

static std::string hex32(const std::array<std::uint8_t, 32>& a) {
    char buf[65];
    for (int i = 0; i < 32; ++i) std::snprintf(buf + 2 * i, 3, "%02x", a[i]);
    return std::string(buf, 64);
}

int main() {
    std::string op;
    while (std::cin >> op) {
        if (op == "kx") {
            std::size_t n = 0;
            std::string mode;
            std::cin >> n >> mode;
            std::vector<std::uint32_t> privates(n), remotes(n);
            for (std::size_t i = 0; i < n; ++i) std::cin >> privates[i] >> remotes[i];
            const bool secrets = mode != "nosecrets";
            const auto r = batch::key_exchange(privates, secrets ? std::span<const std::uint32_t>(remotes)
                                                                 : std::span<const std::uint32_t>());
            if (r.publics.size() != n || r.secrets.size() != (secrets ? n : 0)) {
                std::cout << "bad sizes\n";
                return 1;
            }
            for (std::size_t i = 0; i < n; ++i)
                std::cout << r.publics[i] << " " << (secrets ? hex32(r.secrets[i].bytes) : std::string("-")) << "\n";
        } else if (op == "accept") {
            std::string lid;
            std::uint32_t priv = 0;
            unsigned difficulty = 0;
            std::int64_t now = 0;
            std::size_t n = 0;
            std::cin >> lid >> priv >> difficulty >> now >> n;
            std::vector<batch::HandshakeRequest> reqs(n);
            for (auto& q : reqs) {
                std::string peer;
                std::cin >> peer >> q.remote_public >> q.work_nonce;
                q.peer_id = unhex32(peer);
            }
            const auto res = batch::handshake_accept(unhex32(lid), priv, (std::uint8_t)difficulty,
                                                     std::chrono::steady_clock::time_point{} +
                                                         std::chrono::nanoseconds(now),
                                                     reqs);
            if (res.size() != n) {
                std::cout << "bad sizes\n";
                return 1;
            }
            for (const auto& r : res)
                std::cout << (unsigned)r.verdict << " " << hex32(r.shared_secret.bytes) << " " << hex32(r.session_key)
                          << "\n";
        } else {
            std::cout << "?\n";
            return 1;
        }
    }
    return 0;
}
