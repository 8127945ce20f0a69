// The routing rule of the record engine (csrc/record_route.hpp choose_record_route: per-lane,
// run-staged, line-staged, lockstep or streaming kernel, whole workgroups and rest) against a table
// worked out by hand from the kernels' requirements: host C++ only, exit status 0 when every row
// agrees.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "record_route.hpp"

using enet::RecordKind;

namespace {

// the flags capi.cpp rec_params gives a staging variant (enet_set_staging)
struct Flags { int coop, coop_lines, lockstep, stream; };
constexpr Flags kSt1{1, 1, 1, 1};  // default
constexpr Flags kSt4{1, 0, 0, 0};  // plain run staging
constexpr Flags kSt5{5, 0, 0, 0};  // lockstep run staging only
constexpr Flags kSt0{0, 0, 0, 0};  // per-lane only

struct Row {
    int id;
    uint32_t P;
    bool frame_none;
    uint32_t n;
    uint64_t L;  // uniform_len
    bool order;
    Flags f;
    RecordKind want;
    uint32_t full, rest;
};

const char* name(RecordKind k) {
    switch (k) {
    case RecordKind::PerLane: return "PerLane";
    case RecordKind::RunStaged: return "RunStaged";
    case RecordKind::LineStaged: return "LineStaged";
    case RecordKind::Lockstep: return "Lockstep";
    case RecordKind::Stream: return "Stream";
    }
    return "?";
}

int logp_of(uint32_t P) { return P == 1 ? 0 : P == 2 ? 1 : P == 4 ? 2 : P == 8 ? 3 : 4; }

// records per workgroup of a kind: 512 lanes for the lockstep and streaming kernels, else 256
uint32_t per_wg_of(RecordKind k, uint32_t P) {
    return (k == RecordKind::Lockstep || k == RecordKind::Stream ? 512u : 256u) / P;
}

int bad = 0;

void check(const Row& w) {
    const enet::RecordRoute r = enet::choose_record_route(logp_of(w.P), w.frame_none, w.n, w.L, w.order, w.f.coop,
                                                          w.f.coop_lines, w.f.lockstep, w.f.stream);
    const bool ok = r.kind == w.want && r.full == w.full && r.rest == w.rest && r.per_wg == per_wg_of(w.want, w.P) &&
                    (uint64_t)r.full * r.per_wg + r.rest == w.n;
    std::printf("row %4d: P %2u L %9llu n %8u coop %d%d%d%d -> %-10s per_wg %3u full %5u rest %3u%s\n", w.id, w.P,
                (unsigned long long)w.L, w.n, w.f.coop, w.f.coop_lines, w.f.lockstep, w.f.stream, name(r.kind),
                r.per_wg, r.full, r.rest, ok ? "" : "   <-- MISMATCH");
    if (!ok) {
        std::printf("          wanted %s, full %u, rest %u\n", name(w.want), w.full, w.rest);
        ++bad;
    }
}

}  // namespace

int main() {
    constexpr uint64_t T24 = 1ull << 24;
    const Row rows[] = {
        // (65536, n, 8 lanes): 40 records fill no 64-record workgroup of the 512-lane kernels, so
        // staging 1 and 5 run all of them per lane; the 256-thread kernel holds 32
        {1, 8, true, 40, 65536, false, kSt1, RecordKind::PerLane, 0, 40},
        {2, 8, true, 40, 65536, false, kSt5, RecordKind::PerLane, 0, 40},
        {3, 8, true, 40, 65536, false, kSt4, RecordKind::RunStaged, 1, 8},
        {4, 8, true, 40, 65536, false, kSt0, RecordKind::PerLane, 0, 40},
        {5, 8, true, 72, 65536, false, kSt1, RecordKind::Stream, 1, 8},
        {6, 8, true, 72, 65536, false, kSt5, RecordKind::Lockstep, 1, 8},
        {7, 8, true, 72, 65536, false, kSt4, RecordKind::RunStaged, 2, 8},
        // one whole 512-lane workgroup is the least the streaming kernel takes: n = 512/P - 1
        // against 512/P, every P, at L = 128 P (the 256-thread kernel still fills one workgroup)
        {10, 1, true, 511, 128, false, kSt1, RecordKind::PerLane, 0, 511},
        {11, 1, true, 512, 128, false, kSt1, RecordKind::Stream, 1, 0},
        {12, 2, true, 255, 256, false, kSt1, RecordKind::PerLane, 0, 255},
        {13, 2, true, 256, 256, false, kSt1, RecordKind::Stream, 1, 0},
        {14, 4, true, 127, 512, false, kSt1, RecordKind::PerLane, 0, 127},
        {15, 4, true, 128, 512, false, kSt1, RecordKind::Stream, 1, 0},
        {16, 8, true, 63, 1024, false, kSt1, RecordKind::PerLane, 0, 63},
        {17, 8, true, 64, 1024, false, kSt1, RecordKind::Stream, 1, 0},
        {18, 16, true, 31, 2048, false, kSt1, RecordKind::PerLane, 0, 31},
        {19, 16, true, 32, 2048, false, kSt1, RecordKind::Stream, 1, 0},
        {20, 16, true, 31, 2048, false, kSt4, RecordKind::RunStaged, 1, 15},
        {21, 1, true, 511, 128, false, kSt4, RecordKind::RunStaged, 1, 255},
        {22, 8, true, 63, 1024, false, kSt5, RecordKind::PerLane, 0, 63},
        {23, 8, true, 64, 1024, false, kSt5, RecordKind::Lockstep, 1, 0},
        // the streaming kernel moves stages of 128 bytes per lane: L = 128 P against 128 P +- 64
        {30, 1, true, 600, 128, false, kSt1, RecordKind::Stream, 1, 88},
        {31, 1, true, 600, 64, false, kSt1, RecordKind::Lockstep, 1, 88},
        {32, 1, true, 600, 192, false, kSt1, RecordKind::Lockstep, 1, 88},
        {33, 2, true, 600, 256, false, kSt1, RecordKind::Stream, 2, 88},
        {34, 2, true, 600, 192, false, kSt1, RecordKind::Lockstep, 2, 88},
        {35, 2, true, 600, 320, false, kSt1, RecordKind::Lockstep, 2, 88},
        {36, 16, true, 100, 2048, false, kSt1, RecordKind::Stream, 3, 4},
        {37, 16, true, 100, 1984, false, kSt1, RecordKind::Lockstep, 3, 4},
        {38, 16, true, 100, 2112, false, kSt1, RecordKind::Lockstep, 3, 4},
        // 32-bit arena offsets in the streaming kernel: L n = 2^32 - 128 is the last it takes
        {40, 1, true, (1u << 25) - 1, 128, false, kSt1, RecordKind::Stream, 65535, 511},
        {41, 1, true, 1u << 25, 128, false, kSt1, RecordKind::Lockstep, 65536, 0},
        {42, 2, true, (1u << 20) - 1, 4096, false, kSt1, RecordKind::Stream, 4095, 255},
        {43, 2, true, 1u << 20, 4096, false, kSt1, RecordKind::Lockstep, 4096, 0},
        // line staging: one lane, staging 1 only, L no multiple of 64 but of 4, below 2^24, and
        // 32-bit line offsets (L n < 0xFFFFFF00)
        {50, 1, true, 1000, 1500, false, kSt1, RecordKind::LineStaged, 3, 232},
        {51, 1, true, 1000, 1472, false, kSt1, RecordKind::Lockstep, 1, 488},   // L & 63 == 0
        {52, 1, true, 1000, 1502, false, kSt1, RecordKind::Lockstep, 1, 488},   // L & 3 != 0
        {53, 1, true, 1000, 1501, false, kSt1, RecordKind::Lockstep, 1, 488},
        {54, 2, true, 1000, 1500, false, kSt1, RecordKind::Lockstep, 3, 232},   // two lanes
        {55, 1, true, 1000, 1500, false, kSt4, RecordKind::RunStaged, 3, 232},  // staging 4: no lines
        {56, 1, true, 1000, 1500, false, kSt5, RecordKind::Lockstep, 1, 488},
        {57, 1, true, 256, T24 - 4, false, kSt1, RecordKind::LineStaged, 1, 0},  // L n = 0xFFFFFC00
        {58, 1, true, 512, T24 + 4, false, kSt1, RecordKind::Lockstep, 1, 0},    // L >= 2^24
        {59, 1, true, 2863311, 1500, false, kSt1, RecordKind::LineStaged, 11184, 207},  // L n = 0xFFFFFCE4
        {60, 1, true, 2863312, 1500, false, kSt1, RecordKind::Lockstep, 5592, 208},     // L n = 0x1000002C0
        {61, 1, true, 255, 1500, false, kSt1, RecordKind::PerLane, 0, 255},  // no whole workgroup
        // an order list, a frame mode or a batch that is not uniform: per lane, whatever the flags
        {70, 2, true, 300, 4096, false, kSt1, RecordKind::Stream, 1, 44},
        {71, 2, true, 300, 4096, true, kSt1, RecordKind::PerLane, 0, 300},
        {72, 2, false, 300, 4096, false, kSt1, RecordKind::PerLane, 0, 300},
        {73, 2, true, 300, 0, false, kSt1, RecordKind::PerLane, 0, 300},
        {74, 1, true, 1000, 1500, true, kSt1, RecordKind::PerLane, 0, 1000},
        {75, 1, false, 1000, 1500, false, kSt1, RecordKind::PerLane, 0, 1000},
        {76, 2, true, 300, 4100, true, kSt5, RecordKind::PerLane, 0, 300},
        {77, 2, false, 300, 4100, false, kSt4, RecordKind::PerLane, 0, 300},
        {78, 4, true, 0, 4096, false, kSt1, RecordKind::PerLane, 0, 0},
        // the flags one by one: no streaming -> lockstep; no lockstep either -> plain run staging
        {80, 2, true, 300, 4096, false, Flags{1, 1, 1, 0}, RecordKind::Lockstep, 1, 44},
        {81, 2, true, 300, 4096, false, Flags{1, 1, 0, 0}, RecordKind::RunStaged, 2, 44},
        {82, 1, true, 1000, 1500, false, Flags{1, 0, 1, 1}, RecordKind::Lockstep, 1, 488},
        {83, 1, true, 1000, 1500, false, Flags{1, 1, 0, 0}, RecordKind::LineStaged, 3, 232},
    };
    for (const Row& w : rows) check(w);

    // The shapes of tests/test_gpu_uniform_matrix.py, from its description: L = 64 P B - r and
    // n = full (512 / P) + 3 records with full = max(2, ceil((P B + 1) / (512 / P))).
    //   staging 1: r == 0 with B = 2, 4, 6 is the streaming kernel (1, 2, 3 stages); one lane with
    //              r == 44 is line-staged; everything else lockstep
    //   staging 5: lockstep; staging 4: the 256-thread kernel (twice the workgroups); 0: per lane
    int id = 1000;
    for (uint32_t P : {1u, 2u, 4u, 8u, 16u})
        for (uint32_t B : {2u, 4u, 5u, 6u})
            for (uint32_t r : {0u, 1u, 44u}) {
                const uint32_t per = 512u / P;
                uint32_t full = (P * B + 1 + per - 1) / per;
                if (full < 2) full = 2;
                const uint32_t n = full * per + 3;
                const uint64_t L = 64ull * P * B - r;
                RecordKind k1 = RecordKind::Lockstep;
                if (r == 0 && B != 5) k1 = RecordKind::Stream;
                else if (P == 1 && r == 44) k1 = RecordKind::LineStaged;
                const uint32_t full1 = k1 == RecordKind::LineStaged ? 2 * full : full;
                check({id++, P, true, n, L, false, kSt1, k1, full1, 3});
                check({id++, P, true, n, L, false, kSt5, RecordKind::Lockstep, full, 3});
                check({id++, P, true, n, L, false, kSt4, RecordKind::RunStaged, 2 * full, 3});
                check({id++, P, true, n, L, false, kSt0, RecordKind::PerLane, 0, n});
            }
    std::printf("%d rows, %d mismatches\n", (int)(sizeof rows / sizeof rows[0]) + id - 1000, bad);
    return bad ? 1 : 0;
}
