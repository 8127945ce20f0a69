// shamir_host_bench.cpp -- the scalar Shamir::split / Shamir::combine on one host thread, 65 536
// calls each at 3-of-5 (profiles/shamir_bench.json "host").  The same program, the same inputs,
// built twice:
//   drop-in:    g++ -O2 -std=c++20 -I include tools/shamir_host_bench.cpp \
//                   -L ephemeralnet_amd -lenet_crypto -Wl,-rpath,$PWD/ephemeralnet_amd
//   reference:  g++ -O2 -std=c++20 -I <reference>/include tools/shamir_host_bench.cpp \
//                   <reference>/src/crypto/Shamir.cpp
#include <array>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "ephemeralnet/crypto/Shamir.hpp"

using ephemeralnet::crypto::Shamir;
using ephemeralnet::crypto::ShamirShare;

int main(int argc, char** argv) {
    const int n = 65536;
    const char* label = argc > 1 ? argv[1] : "";
    std::vector<std::array<std::uint8_t, 32>> secrets(n);
    std::uint64_t s = 42;
    for (auto& sec : secrets)
        for (auto& b : sec) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            b = (std::uint8_t)(s >> 56);
        }
    std::vector<std::vector<ShamirShare>> shares(n);
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    for (int i = 0; i < n; ++i) shares[i] = Shamir::split(secrets[i], 3, 5);
    const auto t1 = clk::now();
    for (int i = 0; i < n; ++i) shares[i] = {shares[i][4], shares[i][1], shares[i][2]};
    unsigned bad = 0;
    double best = 1e30;
    for (int rep = 0; rep < 5; ++rep) {
        const auto c0 = clk::now();
        for (int i = 0; i < n; ++i) bad += Shamir::combine(shares[i], 3) != secrets[i];
        const double ms = std::chrono::duration<double, std::milli>(clk::now() - c0).count();
        if (ms < best) best = ms;
    }
    const double split_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    std::printf("{\"build\": \"%s\", \"calls\": %d, \"split_ms\": %.2f, \"split_us_per_call\": %.3f, "
                "\"combine_ms_best_of_5\": %.2f, \"combine_us_per_call\": %.3f, \"wrong\": %u}\n",
                label, n, split_ms, 1e3 * split_ms / n, best, 1e3 * best / n, bad);
    return bad != 0;
}
