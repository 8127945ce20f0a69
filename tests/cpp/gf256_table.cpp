// gf256_table.cpp -- csrc/gf256.hpp against the exp / log-table definition of GF(2^8)/0x11D
// (generator 2): all 256 x 256 products, all 255 inverses, and the SWAR forms (four packed bytes times a
// scalar byte, times four packed bytes, and their inverses) against scalar multiplies.  Plain host C++ (tests/test_shamir_api.py builds it with g++ alone; it may also be
// built with -fsanitize=address,undefined and run directly).
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "gf256.hpp"

namespace gf = enet::gf256;

static uint8_t g_exp[512], g_log[256];

static uint8_t table_mul(uint8_t a, uint8_t b) {
    if (a == 0 || b == 0) return 0;
    return g_exp[(g_log[a] + g_log[b]) % 255];
}

static uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int check_swar(uint32_t a, uint8_t b) {
    const uint32_t got = gf::mul4(a, b);
    uint32_t want = 0;
    for (int k = 0; k < 4; ++k) want |= (uint32_t)gf::mul((uint8_t)(a >> (8 * k)), b) << (8 * k);
    if (got != want) {
        std::printf("mul4(%08x, %02x) = %08x, four scalar multiplies give %08x\n", a, b, got, want);
        return 1;
    }
    return 0;
}

// the packed-by-packed multiply and inverse against the scalar ones, byte by byte
static int check_packed(uint32_t a, uint32_t b) {
    uint32_t want = 0, winv = 0;
    for (int k = 0; k < 4; ++k) {
        want |= (uint32_t)gf::mul((uint8_t)(a >> (8 * k)), (uint8_t)(b >> (8 * k))) << (8 * k);
        winv |= (uint32_t)gf::inv((uint8_t)(a >> (8 * k))) << (8 * k);
    }
    if (gf::mul4x4(a, b) != want || gf::inv4(a) != winv) {
        std::printf("mul4x4(%08x, %08x) = %08x (want %08x), inv4 = %08x (want %08x)\n", a, b, gf::mul4x4(a, b), want,
                    gf::inv4(a), winv);
        return 1;
    }
    return 0;
}

int main() {
    unsigned x = 1;
    for (int i = 0; i < 255; ++i) {
        g_exp[i] = (uint8_t)x;
        g_log[x] = (uint8_t)i;
        x <<= 1;
        if (x & 0x100u) x ^= 0x11Du;
    }
    if (x != 1) {
        std::printf("2 does not generate the field\n");
        return 1;
    }
    int bad = 0;
    for (unsigned a = 0; a < 256; ++a)
        for (unsigned b = 0; b < 256; ++b)
            if (gf::mul((uint8_t)a, (uint8_t)b) != table_mul((uint8_t)a, (uint8_t)b)) {
                if (bad++ < 5)
                    std::printf("mul(%02x, %02x) = %02x, tables give %02x\n", a, b, gf::mul((uint8_t)a, (uint8_t)b),
                                table_mul((uint8_t)a, (uint8_t)b));
            }
    for (unsigned a = 1; a < 256; ++a) {
        const uint8_t want = g_exp[(255 - g_log[a]) % 255];
        if (gf::inv((uint8_t)a) != want || table_mul((uint8_t)a, gf::inv((uint8_t)a)) != 1) {
            if (bad++ < 5) std::printf("inv(%02x) = %02x, tables give %02x\n", a, gf::inv((uint8_t)a), want);
        }
        if (gf::xtime((uint8_t)a) != table_mul((uint8_t)a, 2)) ++bad;
    }
    if (gf::inv(0) != 0) ++bad;  // a^254 of 0: the kernels rely on it for a zero denominator
    uint64_t seed = 2024;
    for (int i = 0; i < 20000; ++i) {
        const uint64_t r = splitmix(seed);
        bad += check_swar((uint32_t)r, (uint8_t)(r >> 32));
        bad += check_packed((uint32_t)r, (uint32_t)(r >> 32));
    }
    for (uint32_t a : {0x00000000u, 0xFFFFFFFFu, 0x80808080u, 0x01000080u})
        for (uint32_t b : {0x00000000u, 0xFFFFFFFFu, 0x80808080u, 0x0201FF80u}) bad += check_packed(a, b);
    for (unsigned a = 0; a < 256; ++a) bad += check_packed(a * 0x01000001u + 0x00020300u, 0x01010101u * a);
    for (unsigned b = 0; b < 256; ++b)
        for (uint32_t a : {0x00000000u, 0xFFFFFFFFu, 0x80808080u, 0x80000000u, 0x00000080u, 0x80FF0001u})
            bad += check_swar(a, (uint8_t)b);
    static_assert(gf::mul(0x80, 2) == 0x1D && gf::mul4(0x80808080u, 2) == 0x1D1D1D1Du, "reduction by 0x11D");
    if (bad) {
        std::printf("%d mismatches\n", bad);
        return 1;
    }
    std::printf("gf256 ok\n");
    return 0;
}
