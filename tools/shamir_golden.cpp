// shamir_golden.cpp -- driver of tools/gen_shamir_golden.py: runs the REFERENCE's Shamir::split /
// Shamir::combine (compiled from the reference checkout where it lies, never copied here) on the
// operations it reads from stdin, one per line, and prints one result line each:
//   split <threshold> <share_count> <secret hex>      -> "<index>:<value hex>" per share
//   combine <threshold> <index>:<value hex> ...       -> "<secret hex>", or "throw" on
//                                                        std::invalid_argument
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
            if (op == "split") {
                unsigned n = 0;
                std::string secret;
                in >> n >> secret;
                const auto shares = Shamir::split(unhex32(secret), (std::uint8_t)t, (std::uint8_t)n);
                for (std::size_t i = 0; i < shares.size(); ++i)
                    std::cout << (i ? " " : "") << (unsigned)shares[i].index << ":" << hex32(shares[i].value);
                std::cout << "\n";
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
