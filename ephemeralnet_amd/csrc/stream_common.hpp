// stream_common.hpp -- shape constants of the streaming kernel (stream.hip).
#pragma once
#include <type_traits>

#include "records_body.hpp"

namespace enet {

constexpr uint32_t kStreamLanes = 512;    // record lanes per workgroup (8 compute waves)
constexpr uint32_t kStreamWG = 768;       // + 4 memory waves
constexpr int kStreamSteps = 76;          // keystream barriers per stage (19 lockstep half-rounds)

__device__ __forceinline__ void stream_barrier() { asm volatile("s_barrier" ::: "memory"); }

// Holds a value at this point of the asm volatile order (no instruction): what computes it cannot
// sink below, what consumes it cannot rise above.
#define ENET_PIN(v) asm volatile("" : "+v"(v))

// Placement variant (stream_issue poly 2 / 3): the Poly1305 of one stage -- the eight 16-byte blocks of the
// run in w -- cut into 72 pieces of 3-7 instructions, piece s run by the step hook of keystream
// step s (chacha_half_lockstep2), steps 72-75 empty.  Block s / 9 is poly32_block's arithmetic
// word for word, in nine pieces (the message add, the four column sums, the carries, the fold);
// every piece begins by pinning what it consumes and ends by pinning what it produced, so each
// sits in its own barrier interval, and no carry flag crosses a pin.  BAR_AFTER: the hook ends with the step's s_barrier (the lockstep
// statement is then the barrier-free one), so the piece runs behind the step's rotates.
template <bool BAR_AFTER>
struct PolySpreadHook {
    uint32_t (&h)[5];
    const PolyR32& R;
    const uint32_t (&w)[32];
    uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0, a4 = 0, x0 = 0, x1 = 0, x2 = 0, x3 = 0, c = 0, t4 = 0, f = 0;
    uint64_t d0 = 0, e1 = 0, e2 = 0, e3 = 0;

    __device__ __forceinline__ PolySpreadHook(uint32_t (&h_)[5], const PolyR32& R_, const uint32_t (&w_)[32])
        : h(h_), R(R_), w(w_) {}

    __device__ __forceinline__ void pin_a() {
        ENET_PIN(a0); ENET_PIN(a1); ENET_PIN(a2); ENET_PIN(a3); ENET_PIN(a4);
    }
    template <int S>
    __device__ __forceinline__ void piece() {
        constexpr int b = 4 * ((S % 72) / 9), q = S < 72 ? S % 9 : -1;
        unsigned cy;
        if constexpr (q == 0) {
            ENET_PIN(h[0]); ENET_PIN(h[1]); ENET_PIN(h[2]); ENET_PIN(h[3]); ENET_PIN(h[4]);
            a0 = __builtin_addc(h[0], w[b], 0u, &cy);
            a1 = __builtin_addc(h[1], w[b + 1], cy, &cy);
            a2 = __builtin_addc(h[2], w[b + 2], cy, &cy);
            a3 = __builtin_addc(h[3], w[b + 3], cy, &cy);
            a4 = h[4] + 1u + cy;
            ENET_PIN(a0); ENET_PIN(a1); ENET_PIN(a2); ENET_PIN(a3); ENET_PIN(a4);
        } else if constexpr (q == 1) {
            pin_a();
            d0 = (uint64_t)a0 * R.r0 + (uint64_t)a1 * R.s3 + (uint64_t)a2 * R.s2 + (uint64_t)a3 * R.s1;
            ENET_PIN(d0);
        } else if constexpr (q == 2) {
            pin_a();
            e1 = (uint64_t)a0 * R.r1 + (uint64_t)a1 * R.r0 + (uint64_t)a2 * R.s3 + (uint64_t)a3 * R.s2 +
                 (uint64_t)a4 * R.s1;
            ENET_PIN(e1);
        } else if constexpr (q == 3) {
            pin_a();
            e2 = (uint64_t)a0 * R.r2 + (uint64_t)a1 * R.r1 + (uint64_t)a2 * R.r0 + (uint64_t)a3 * R.s3 +
                 (uint64_t)a4 * R.s2;
            ENET_PIN(e2);
        } else if constexpr (q == 4) {
            pin_a();
            e3 = (uint64_t)a0 * R.r3 + (uint64_t)a1 * R.r2 + (uint64_t)a2 * R.r1 + (uint64_t)a3 * R.r0 +
                 (uint64_t)a4 * R.s3;
            ENET_PIN(e3);
        } else if constexpr (q == 5) {
            ENET_PIN(d0); ENET_PIN(e1); ENET_PIN(e2);
            x0 = (uint32_t)d0;
            x1 = __builtin_addc((uint32_t)e1, (uint32_t)(d0 >> 32), 0u, &cy);
            c = (uint32_t)(e1 >> 32) + cy;
            x2 = __builtin_addc((uint32_t)e2, c, 0u, &cy);
            c = (uint32_t)(e2 >> 32) + cy;
            ENET_PIN(x1); ENET_PIN(x2); ENET_PIN(c);
        } else if constexpr (q == 6) {
            ENET_PIN(e3); ENET_PIN(c); ENET_PIN(a4);
            x3 = __builtin_addc((uint32_t)e3, c, 0u, &cy);
            c = (uint32_t)(e3 >> 32) + cy;
            t4 = a4 * R.r0 + c;
            ENET_PIN(x3); ENET_PIN(t4);
        } else if constexpr (q == 7) {
            ENET_PIN(t4);
            f = (t4 >> 2) * 5u;
            t4 &= 3u;
            ENET_PIN(f); ENET_PIN(t4);
        } else if constexpr (q == 8) {
            ENET_PIN(x0); ENET_PIN(x1); ENET_PIN(x2); ENET_PIN(x3); ENET_PIN(f); ENET_PIN(t4);
            h[0] = __builtin_addc(x0, f, 0u, &cy);
            h[1] = __builtin_addc(x1, 0u, cy, &cy);
            h[2] = __builtin_addc(x2, 0u, cy, &cy);
            h[3] = __builtin_addc(x3, 0u, cy, &cy);
            h[4] = t4 + cy;
            ENET_PIN(h[0]); ENET_PIN(h[1]); ENET_PIN(h[2]); ENET_PIN(h[3]); ENET_PIN(h[4]);
        }
    }
    template <int S>
    __device__ __forceinline__ void operator()(std::integral_constant<int, S>) {
        piece<S>();
        if (BAR_AFTER) stream_barrier();
    }
};

}  // namespace enet
