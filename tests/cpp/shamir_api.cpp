// shamir_api.cpp -- the scalar Shamir drop-in (include/ephemeralnet/crypto/Shamir.hpp, reference
// signatures) of libenet_crypto.so, driven by tests/test_shamir_api.py.  One operation per stdin
// line, one result line each; std::invalid_argument prints "throw", anything else escapes.
//   split <t> <n> <secret hex>            -> "<index>:<value hex>" per share
//   combine <t> <index>:<value hex> ...   -> "<secret hex>"
//   roundtrip <t> <n> <secret hex>        -> "1" when split gives n shares with indices 1..n and
//                                            the first t, the last t reversed and more than t
//                                            shares each combine to the secret
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "ephemeralnet/crypto/Shamir.hpp"

using ephemeralnet::crypto::Shamir;
using ephemeralnet::crypto::ShamirShare;

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
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        unsigned t = 0;
        in >> op >> t;
        try {
            if (op == "split" || op == "roundtrip") {
                unsigned n = 0;
                std::string hex;
                in >> n >> hex;
                const auto secret = unhex32(hex);
                const auto shares = Shamir::split(secret, (std::uint8_t)t, (std::uint8_t)n);
                if (op == "split") {
                    for (std::size_t i = 0; i < shares.size(); ++i)
                        std::cout << (i ? " " : "") << (unsigned)shares[i].index << ":" << hex32(shares[i].value);
                    std::cout << "\n";
                    continue;
                }
                bool ok = shares.size() == n;
                for (std::size_t i = 0; ok && i < shares.size(); ++i) ok = shares[i].index == i + 1;
                if (ok) {
                    std::vector<ShamirShare> first(shares.begin(), shares.begin() + t);
                    std::vector<ShamirShare> last(shares.end() - t, shares.end());
                    std::reverse(last.begin(), last.end());
                    std::vector<ShamirShare> more = last;  // more than t: only the first t count
                    ShamirShare junk{};
                    junk.index = last[0].index;            // a duplicate index behind the threshold
                    junk.value.fill(0xA5);
                    more.push_back(junk);
                    ok = Shamir::combine(first, (std::uint8_t)t) == secret &&
                         Shamir::combine(last, (std::uint8_t)t) == secret &&
                         Shamir::combine(more, (std::uint8_t)t) == secret &&
                         Shamir::combine(shares, (std::uint8_t)t) == secret;
                }
                std::cout << (ok ? "1" : "0") << "\n";
            } else if (op == "combine") {
                std::vector<ShamirShare> shares;
                std::string tok;
                while (in >> tok) {
                    const auto colon = tok.find(':');
                    ShamirShare s{};
                    s.index = (std::uint8_t)std::stoul(tok.substr(0, colon));
                    s.value = unhex32(tok.substr(colon + 1));
                    shares.push_back(s);
                }
                std::cout << hex32(Shamir::combine(shares, (std::uint8_t)t)) << "\n";
            } else {
                std::cout << "?\n";
            }
        } catch (const std::invalid_argument&) {
            std::cout << "throw\n";
        }
    }
    return 0;
}
