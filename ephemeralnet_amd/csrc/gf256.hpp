// gf256.hpp -- GF(2^8) with the reference Shamir field: reduction polynomial x^8+x^4+x^3+x^2+1
// (0x11D, kFieldPolynomial, src/crypto/Shamir.cpp:10), generator 2.  NOT the AES field (0x11B).
// The single definition of the field for the kernels (shamir.hip), the scalar drop-in
// (shamir_host.cpp) and the tests (tests/cpp/gf256_table.cpp).  Plain C++, no HIP header: usable from
// host and device code.
//
// No table is indexed by data (the reference multiplies through log / exp tables indexed by
// share bytes, Shamir.cpp:41-49): every operation below is a fixed sequence of shifts, ANDs and
// XORs whose memory accesses and branches do not depend on its operands.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define ENET_GF_HD __host__ __device__ inline
#else
#define ENET_GF_HD inline
#endif

namespace enet::gf256 {

constexpr uint32_t kPoly = 0x11Du;

// a * x
ENET_GF_HD constexpr uint8_t xtime(uint8_t a) {
    return (uint8_t)((uint32_t)(a << 1) ^ ((0u - (uint32_t)(a >> 7)) & kPoly));
}

// a * b: shift and conditional xor, 8 branch-free steps
ENET_GF_HD constexpr uint8_t mul(uint8_t a, uint8_t b) {
    uint32_t r = 0, x = a;
    for (int k = 0; k < 8; ++k) {
        r ^= x & (0u - ((uint32_t)(b >> k) & 1u));
        x = ((x << 1) ^ ((0u - (x >> 7)) & kPoly)) & 0xFFu;
    }
    return (uint8_t)r;
}

// SWAR: the four packed bytes of a, each times x
ENET_GF_HD constexpr uint32_t xtime4(uint32_t a) {
    return ((a & 0x7F7F7F7Fu) << 1) ^ (((a >> 7) & 0x01010101u) * 0x1Du);
}

// SWAR: the four packed bytes of a, each times the scalar byte b
ENET_GF_HD constexpr uint32_t mul4(uint32_t a, uint8_t b) {
    uint32_t r = 0;
    for (int k = 0; k < 8; ++k) {
        r ^= a & (0u - ((uint32_t)(b >> k) & 1u));
        a = xtime4(a);
    }
    return r;
}

// SWAR: the four packed bytes of a times the four packed bytes of b, byte by byte
ENET_GF_HD constexpr uint32_t mul4x4(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int k = 0; k < 8; ++k) {
        r ^= a & (((b >> k) & 0x01010101u) * 0xFFu);
        a = xtime4(a);
    }
    return r;
}

// a^254 = a^-1 (0 -> 0): a^2 * a^4 * ... * a^128
ENET_GF_HD constexpr uint8_t inv(uint8_t a) {
    uint8_t s = mul(a, a), r = s;
    for (int k = 0; k < 6; ++k) {
        s = mul(s, s);
        r = mul(r, s);
    }
    return r;
}

// SWAR: the inverses of four packed bytes
ENET_GF_HD constexpr uint32_t inv4(uint32_t a) {
    uint32_t s = mul4x4(a, a), r = s;
    for (int k = 0; k < 6; ++k) {
        s = mul4x4(s, s);
        r = mul4x4(r, s);
    }
    return r;
}

}  // namespace enet::gf256
