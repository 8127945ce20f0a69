// record_route.hpp -- which record kernel a launch of the record engine runs on (records.hip
// launch_one), as a pure function of the batch's shape and the staging flags.  No HIP here: host
// tests compile this header alone (tests/cpp/record_route_table.cpp).
#pragma once

#include <stdint.h>

namespace enet {

constexpr uint32_t kRouteWG = 256;      // threads of a plain record workgroup (kWG)
constexpr uint32_t kRouteWideWG = 512;  // record lanes of a lockstep / streaming workgroup (kStreamLanes)

enum class RecordKind : int {
    PerLane = 0,     // records_kernel<.., COOP 0>: every lane loads and stores its own blocks
    RunStaged = 1,   // records_kernel<.., COOP 1>: 256-thread workgroups, runs staged through LDS
    LineStaged = 2,  // records_kernel<0, .., COOP 4>: one lane per record, whole aligned lines
    Lockstep = 3,    // records_kernel_l (COOP 5): run staging in 512-thread lockstep workgroups
    Stream = 4,      // stream_kernel (stream.hip)
};
constexpr int kRecordKinds = 5;

// `kind` runs records [0, full * per_wg) in `full` whole workgroups of per_wg records; the `rest`
// records after them run per lane (a launch of their own).  kind == PerLane: full == 0, every
// record is in rest.
struct RecordRoute {
    RecordKind kind;
    uint32_t per_wg, full, rest;
};

// logp: log2 of the lanes per record (0..4); frame_none: not a frame mode; n: records of the launch;
// uniform_len: the length every record has by the caller's hints (0 = not uniform); has_order: the
// batch carries an order list; coop / coop_lines / lockstep / stream: RecParams' staging flags
// (capi.cpp rec_params).
// The streaming kernel takes uniform batches of L % (128 P) == 0 whose arenas stay below 4 GiB
// (32-bit offsets) and that fill at least one 512-lane workgroup.  The staged kernels take the
// other uniform batches, over whole workgroups: line staging for one-lane records that are no
// multiple of 64 bytes (4-byte-aligned starts, 24-bit lengths, 32-bit line offsets), else run
// staging, in lockstep 512-thread workgroups unless a plain variant is asked for.
inline RecordRoute choose_record_route(int logp, bool frame_none, uint32_t n, uint64_t uniform_len,
                                       bool has_order, int coop, int coop_lines, int lockstep, int stream) {
    const uint32_t lanes = 1u << logp;
    const uint64_t L = uniform_len;
    if (frame_none && (stream & 1) && L != 0 && !has_order && L % (128ull * lanes) == 0 &&
        L * (uint64_t)n <= 0xFFFFFFFFull && n >= kRouteWideWG / lanes) {
        const uint32_t per_wg = kRouteWideWG >> logp;
        const uint32_t full = n / per_wg;
        return {RecordKind::Stream, per_wg, full, n - full * per_wg};
    }
    if (frame_none && uniform_len != 0 && !has_order && coop >= 1) {
        // Cooperative kernels over whole workgroups of records (no dead owners, no store
        // predicates); the remaining records go through the per-lane kernel.
        // Line staging (COOP 4) for one-lane records that are not 64-byte multiples: 1 M
        // records, 1 GPU, GiB/s line vs run staging -- 1500 B 746 vs 590, 1504 B 762 vs 689,
        // 1400 B 750 vs 613; 1472 B 775 vs 789, 1536 B 835 vs 839 (tools/c3ab.sh).
        const bool lines = logp == 0 && coop == 1 && coop_lines && (uniform_len & 63u) != 0 &&
                           (uniform_len & 3u) == 0 && uniform_len < (1u << 24) &&
                           uniform_len * (uint64_t)n < 0xFFFFFF00ull;
        // Lockstep keystream in 512-thread workgroups (COOP 5) unless a plain variant is asked
        // for: C2 837 -> 864, C4 868 -> 913 GiB/s; not with line staging, where it measured
        // 765 -> 751 at C3 (the line-staging lockstep variant, retired in round 6)
        const bool lock = coop == 5 || (coop == 1 && lockstep && !lines);
        const uint32_t wg = lock ? kRouteWideWG : kRouteWG;
        const uint32_t per_wg = wg >> logp;
        const uint32_t full = n / per_wg;
        if (full)
            return {lines ? RecordKind::LineStaged : lock ? RecordKind::Lockstep : RecordKind::RunStaged,
                    per_wg, full, n - full * per_wg};
    }
    return {RecordKind::PerLane, kRouteWG >> logp, 0u, n};
}

}  // namespace enet
