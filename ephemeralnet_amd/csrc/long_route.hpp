// long_route.hpp -- which path a batch of records takes (record engine or the sequence-parallel
// tiles of segments.hip), as a pure function of the batch's hints.  No HIP here: host tests
// compile this header alone (tests/cpp/route_table.cpp).
#pragma once

#include <stdint.h>

namespace enet {

constexpr int kMaxLanesPerRecord = 16;
enum RecMode : int { MODE_XOR = 0, MODE_SEAL = 1, MODE_OPEN = 2 };
constexpr uint64_t kSegMin = 256u << 10;   // records this long take the tiles (choose_long_route)
constexpr uint64_t kSegTileBytes = 64u << 10;

// hints say every record has the same length: total == n * max (record i then starts at
// offsets[0] + i * max, since records are contiguous by construction)
inline bool hints_uniform(uint32_t count, uint32_t max_len_hint, uint64_t total_bytes_hint) {
    return total_bytes_hint == (uint64_t)count * max_len_hint;
}

enum class LongRoute {
    RecordEngine,  // launch_records over every record
    UniformXor,    // one launch of tile workgroups (launch_seg_uniform_xor), nothing else
    UniformAead,   // one launch too (launch_seg_uniform_aead)
    PlanTiles,     // plan + tile kernels for the records >= long_min, the record engine for the rest
};
struct RouteChoice { LongRoute route; uint64_t long_min; };

// seg_min_setting (enet_set_seg_min): -1 auto; otherwise every record of at least this many bytes
// takes the tiles, whatever the hints say (tests / tuning; INT64_MAX = never).
// Auto: a batch whose longest record (hint) is >= kSegMin takes the tiles for its records >=
// kSegMin -- unless it is uniform and wide enough that 16 lanes per record already fill the chip
// (n * 16 >= 131 072 lanes: the record / streaming kernels run those at the C2 rate).
// A batch the hints call uniform and long, in batch order, is one launch.  Known defects, kept
// (ADVICE.md item 3): the uniform routes do not require max_len_hint != 0, so setting 0 with
// hints 0 / 0 is a UniformXor launch of no tiles; and only the AEAD route caps its tile count.
inline RouteChoice choose_long_route(int mode, bool has_order, uint32_t count, uint32_t max_len_hint,
                                     uint64_t total_bytes_hint, int64_t seg_min_setting) {
    const bool uniform = hints_uniform(count, max_len_hint, total_bytes_hint);
    uint64_t long_min = kSegMin;
    bool wanted = max_len_hint >= kSegMin && !(uniform && (uint64_t)count * kMaxLanesPerRecord >= 131072u);
    if (seg_min_setting >= 0) {
        long_min = (uint64_t)seg_min_setting;
        wanted = seg_min_setting != INT64_MAX;
    }
    const bool aead = mode == MODE_SEAL || mode == MODE_OPEN;
    if (!wanted || !(mode == MODE_XOR || aead)) return {LongRoute::RecordEngine, long_min};
    if (!has_order && uniform && max_len_hint >= long_min) {
        const uint64_t tiles = (uint64_t)count * ((max_len_hint + kSegTileBytes - 1) / kSegTileBytes);
        if (!aead) return {LongRoute::UniformXor, long_min};
        if (tiles < 0x7FFFFFFFull) return {LongRoute::UniformAead, long_min};
    }
    return {LongRoute::PlanTiles, long_min};
}

}  // namespace enet
