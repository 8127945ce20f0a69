// long_route.hpp -- which path a batch of records takes (record engine or the sequence-parallel
// tiles of segments.hip), as a pure function of the batch's hints, and how the plan + tiles path
// lays out its scratch.  No HIP here: host tests compile this header alone
// (tests/cpp/route_table.cpp).
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
// A batch the hints call uniform and long, in batch order, is one launch -- when the hints say
// how long (max_len_hint != 0: hints 0 / 0 mean "unknown", and a launch sized by them would hold
// no tile at all) and the launch's tile count fits 31 bits, for XOR as for AEAD.  Every other
// batch that wants the tiles is planned: capacities from the hints (seg_layout), records beyond
// them with the record engine.
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
    if (!has_order && uniform && max_len_hint != 0 && max_len_hint >= long_min) {
        const uint64_t tiles = (uint64_t)count * ((max_len_hint + kSegTileBytes - 1) / kSegTileBytes);
        if (tiles < 0x7FFFFFFFull) return {aead ? LongRoute::UniformAead : LongRoute::UniformXor, long_min};
    }
    return {LongRoute::PlanTiles, long_min};
}

// A claimed record's entry of the plan + tiles path (segments.hip); entries are sorted by
// tile_base (claimed by CAS on one packed word).
struct SegEntry {
    uint32_t rec, tile_base, ntiles, arrived;
    uint32_t aad_len, nbits, pad0, pad1;
    uint32_t r[4], s[4];     // AEAD: one-time key halves (r unclamped words; s the pad)
    uint32_t pw[5 * 40];     // AEAD: r^(2^k) in 26-bit limbs, k < nbits
};

// The plan + tiles path's scratch (long_records.cpp seg_begin), as byte offsets into one buffer:
//   [0, 256)            the header word (count << 40 | tiles claimed)
//   [o_ent, o_cl)       ecap entries
//   [o_cl, o_cl + n)    the claim bytes, ONE PER POSITION of the launch (n = enet_records.count):
//                       byte k belongs to the k-th record the call processes, order[k] under a
//                       caller order, so its size never depends on the indices the order names
//   [o_part, bytes)     tcap tiles' partials of 32 bytes, 256-aligned
// Capacities come from the hints, and records past them stay with the record engine (never wrong
// bytes): at most total / long_min + 1 records can be long_min bytes or longer, and they hold at
// most total / 64 KiB whole tiles plus a ragged one each.  total_bytes_hint == 0 = unknown: up
// to 1024 records of max_len_hint bytes are assumed.
struct SegLayout {
    uint64_t ecap, tcap;
    uint64_t o_ent, o_cl, o_part, bytes;
};
inline SegLayout seg_layout(uint32_t count, uint32_t max_len_hint, uint64_t total_bytes_hint, uint64_t long_min) {
    const uint64_t n = count;
    const uint64_t total = total_bytes_hint ? total_bytes_hint : (n < 1024u ? n : 1024u) * max_len_hint;
    SegLayout l{};
    const uint64_t by_hint = long_min ? total / long_min + 1 : n;
    l.ecap = by_hint < n ? by_hint : n;
    const uint64_t tiles = total / kSegTileBytes + l.ecap + 1;
    l.tcap = tiles < 0xFFFFFFFFull ? tiles : 0xFFFFFFFFull;
    l.o_ent = 256;
    l.o_cl = l.o_ent + l.ecap * sizeof(SegEntry);
    l.o_part = (l.o_cl + n + 255) & ~uint64_t(255);
    l.bytes = l.o_part + l.tcap * 32;
    return l;
}

// Launch sizes of the plan + tiles path (long_records.cpp seg_begin).  Both kernels walk their work
// in grid strides past these caps: the plan kernel (256 positions per workgroup) beyond
// 256 * kSegPlanBlocksMax = 262 144 positions, the tile kernel (one tile per workgroup and trip)
// beyond kSegTileBlocksMax tiles of capacity.
constexpr uint32_t kSegPlanThreads = 256;
constexpr uint32_t kSegPlanBlocksMax = 1024;
constexpr uint32_t kSegTileBlocksMax = 4096;
struct SegGrid { uint32_t plan_blocks, tile_blocks; };
inline SegGrid seg_grid(uint32_t count, const SegLayout& l) {
    const uint64_t pb = ((uint64_t)count + kSegPlanThreads - 1) / kSegPlanThreads;
    return {(uint32_t)(pb < kSegPlanBlocksMax ? pb : kSegPlanBlocksMax),
            (uint32_t)(l.tcap < kSegTileBlocksMax ? l.tcap : kSegTileBlocksMax)};
}

// Which claim byte the record at position pos of the launch (record index rec) owns: the plan
// kernel writes it and records_body reads it through this one rule.  By position: pos < count
// always, while rec is whatever the caller's order names (one length class of a larger batch).
constexpr uint32_t seg_claim_slot(uint32_t pos, uint32_t /*rec*/) { return pos; }

}  // namespace enet
