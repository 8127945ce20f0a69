// The routing rule for long records (csrc/long_route.hpp choose_long_route) and the scratch
// layout and launch sizes of the plan + tiles path (seg_layout, seg_claim_slot, seg_grid) against tables worked out by hand
// from the rules: host C++ only, exit status 0 when every row agrees.
#include <cstdint>
#include <cstdio>

#include "long_route.hpp"

using enet::LongRoute;

namespace {

constexpr uint64_t KiB = 1024, MiB = 1024 * KiB;
constexpr uint64_t kAny = ~0ull;  // long_min not pinned by the row

struct Row {
    int id;
    int64_t setting;
    int mode;
    bool order;
    uint32_t count;
    uint64_t M;  // max_len_hint
    uint64_t S;  // total_bytes_hint
    LongRoute want;
    uint64_t want_long_min;
};

const char* name(LongRoute r) {
    switch (r) {
    case LongRoute::RecordEngine: return "RecordEngine";
    case LongRoute::UniformXor: return "UniformXor";
    case LongRoute::UniformAead: return "UniformAead";
    case LongRoute::PlanTiles: return "PlanTiles";
    }
    return "?";
}

// seg_layout: the scratch of one plan + tiles call.  E = sizeof(SegEntry) = 216 words = 864.
struct LayoutRow {
    int id;
    uint32_t count;
    uint64_t M, S, long_min;
    uint64_t ecap, tcap, o_cl, o_part, bytes;
    uint32_t first_rec;  // the call's order names records first_rec .. first_rec + count - 1
};

int layout_rows() {
    static_assert(sizeof(enet::SegEntry) == 864, "SegEntry: 8 + 8 + 200 words");
    const LayoutRow rows[] = {
        // 512 records named out of 1024 (indices 512 .. 1023): 508 of 40 bytes and 65 553 +
        // 131 072 + 196 607 + 200 000, S = 20 320 + 593 232 = 613 552.  S / 64 KiB = 9:
        // ecap = min(512, 9 + 1) = 10, tcap = 9 + 10 + 1 = 20, o_cl = 256 + 10 E = 8 896,
        // o_part = roundup256(8 896 + 512 = 9 408) = 9 472, bytes = 9 472 + 20 * 32 = 10 112.
        // (The 11 tiles those four records claim put live partials at [9 472, 9 824): a claim byte
        // indexed by RECORD would sit at 8 896 + 576 .. 927 inside them, at 8 896 + 1 023 = 9 919
        // for the last record.)
        {101, 512, 200000, 613552, 65536, 10, 20, 8896, 9472, 10112, 512},
        // long_min == 0: every record may be claimed (ecap = n); lengths 0, 1, 100, 65 537, 200 000:
        // S = 265 638, S / 64 KiB = 4, tcap = 4 + 5 + 1 = 10, o_cl = 256 + 5 E = 4 576,
        // o_part = roundup256(4 581) = 4 608, bytes = 4 608 + 320
        {102, 5, 200000, 265638, 0, 5, 10, 4576, 4608, 4928, 0},
        // the same batch with unknown hints (0 / 0): total = 0, ecap = 5, tcap = 0 + 5 + 1 = 6
        {103, 5, 0, 0, 0, 5, 6, 4576, 4608, 4800, 0},
        // unknown hints and a threshold: total = 0, ecap = min(3, 0 + 1) = 1, tcap = 2,
        // o_cl = 256 + E = 1 120, o_part = roundup256(1 123) = 1 280
        {104, 3, 0, 0, 65536, 1, 2, 1120, 1280, 1344, 0},
        // total_bytes_hint == 0 with a known longest record: total = min(n, 1024) * M =
        // 1024 * 307 200 = 314 572 800; ecap = min(2000, 1200 + 1), tcap = 4800 + 1201 + 1,
        // o_cl = 256 + 1201 E = 1 037 920, o_part = roundup256(1 039 920) = 1 040 128
        {105, 2000, 307200, 0, 262144, 1201, 6002, 1037920, 1040128, 1232192, 70000},
        // the claim bytes end exactly on a 256-byte line (8 896 + 320 = 9 216), and one past it
        {106, 320, 200000, 613552, 65536, 10, 20, 8896, 9216, 9856, 0xFFFFFEC0u},
        {107, 321, 200000, 613552, 65536, 10, 20, 8896, 9472, 10112, 1},
        // the shapes of tests/test_gpu_tile_limits.py (their launch sizes: grid_rows below).
        // 4 300 records under long_min 0, 4 293 of them 0 .. 4 095 bytes and seven of 65 536 ..
        // 1 MiB: S = 4 386 479, S / 64 KiB = 66, ecap = n, tcap = 66 + 4 300 + 1; the entries alone
        // (4 300 E = 3 715 200 bytes) are past the 256 KiB floor of the plan scratch
        {108, 4300, 1048576, 4386479, 0, 4300, 4367, 3715456, 3719936, 3859680, 0},
        // 257 MiB + 17 and 300 KiB under the automatic threshold: S / 256 KiB + 1 = 1 030 > n,
        // S / 64 KiB = 4 116, tcap = 4 116 + 2 + 1; 133 856 bytes, inside the floor
        {109, 2, 269484049, 269791249, 262144, 2, 4119, 1984, 2048, 133856, 0},
        // 262 444 records of 1 .. 3 bytes but three (262 244, 65 537, 307 200), threshold 64 KiB:
        // S / 64 KiB = 17, ecap 18, tcap 36; the claim bytes are [15 808, 278 252), those of the
        // positions from 262 144 on (the plan kernel's second trip) [277 952, 278 252)
        {110, 262444, 307200, 1159863, 65536, 18, 36, 15808, 278272, 279424, 0},
        // the first 320 records of row 108's batch: its partials start at 277 248, so tiles 22 .. 31
        // of it lie on row 110's second-trip claim bytes
        {111, 320, 65536, 237664, 0, 320, 324, 276736, 277248, 287616, 0},
    };
    int bad = 0;
    for (const LayoutRow& w : rows) {
        const enet::SegLayout l = enet::seg_layout(w.count, (uint32_t)w.M, w.S, w.long_min);
        bool ok = l.ecap == w.ecap && l.tcap == w.tcap && l.o_ent == 256 && l.o_cl == w.o_cl &&
                  l.o_part == w.o_part && l.bytes == w.bytes;
        // the invariants behind the figures: entries, then one claim byte per position, then the
        // partials on a 256-byte line of their own, tcap * 32 bytes of them
        ok = ok && l.o_cl == l.o_ent + l.ecap * sizeof(enet::SegEntry) && l.o_part % 256 == 0 &&
             l.o_part >= l.o_cl + w.count && l.o_part < l.o_cl + w.count + 256 &&
             l.bytes == l.o_part + l.tcap * 32 && l.ecap <= w.count;
        // every claim byte the kernels touch lies in [o_cl, o_cl + count), short of the partials,
        // whichever records the order names
        uint64_t worst = 0;
        for (uint32_t pos = 0; pos < w.count; ++pos) {
            const uint64_t at = l.o_cl + enet::seg_claim_slot(pos, w.first_rec + pos);
            if (at > worst) worst = at;
        }
        const bool inside = worst < l.o_cl + w.count && worst < l.o_part;
        std::printf("layout %d: ecap %llu tcap %llu o_cl %llu o_part %llu bytes %llu, last claim byte %llu%s\n", w.id,
                    (unsigned long long)l.ecap, (unsigned long long)l.tcap, (unsigned long long)l.o_cl,
                    (unsigned long long)l.o_part, (unsigned long long)l.bytes, (unsigned long long)worst,
                    ok && inside ? "" : "   <-- MISMATCH");
        if (!ok)
            std::printf("        wanted ecap %llu tcap %llu o_cl %llu o_part %llu bytes %llu\n",
                        (unsigned long long)w.ecap, (unsigned long long)w.tcap, (unsigned long long)w.o_cl,
                        (unsigned long long)w.o_part, (unsigned long long)w.bytes);
        if (!inside)
            std::printf("        a claim byte lies outside [%llu, %llu)\n", (unsigned long long)l.o_cl,
                        (unsigned long long)(l.o_cl + w.count));
        bad += !(ok && inside);
    }
    return bad;
}

// seg_grid: the launch sizes of the plan + tiles path, capped at kSegPlanBlocksMax workgroups of
// 256 positions and kSegTileBlocksMax tile workgroups; the kernels stride past the caps.
struct GridRow {
    int id;
    uint32_t count;
    uint64_t M, S, long_min;
    uint32_t plan_blocks, tile_blocks;
};

int grid_rows() {
    static_assert(enet::kSegPlanBlocksMax == 1024 && enet::kSegTileBlocksMax == 4096 && enet::kSegPlanThreads == 256,
                  "the caps the rows below were worked out for");
    const GridRow rows[] = {
        // under both caps: ceil(512 / 256) = 2 plan workgroups, tcap = 20 tile workgroups (row 101)
        {201, 512, 200000, 613552, 65536, 2, 20},
        {202, 1, 0, 0, 0, 1, 2},
        // the last n that fits one plan trip, and the first that does not
        {203, 262144, 3, 786432, 65536, 1024, 26},
        {204, 262145, 3, 786435, 65536, 1024, 26},
        // layout rows 108 .. 110: 4 367 and 4 119 tiles of capacity on 4 096 workgroups (a second
        // trip of the tile loop); 262 444 positions on 1 024 plan workgroups (a second trip there)
        {205, 4300, 1048576, 4386479, 0, 17, 4096},
        {206, 2, 269484049, 269791249, 262144, 1, 4096},
        {207, 262444, 307200, 1159863, 65536, 1024, 36},
        // exactly at the tile cap: tcap = 4 093 + 2 + 1 = 4 096 (S = 4 093 * 64 KiB)
        {208, 2, 268238848, 268238848 + 1, 262144, 1, 4096},
    };
    int bad = 0;
    for (const GridRow& w : rows) {
        const enet::SegLayout l = enet::seg_layout(w.count, (uint32_t)w.M, w.S, w.long_min);
        const enet::SegGrid g = enet::seg_grid(w.count, l);
        const bool ok = g.plan_blocks == w.plan_blocks && g.tile_blocks == w.tile_blocks;
        std::printf("grid %d: plan %u tiles %u (tcap %llu)%s\n", w.id, g.plan_blocks, g.tile_blocks,
                    (unsigned long long)l.tcap, ok ? "" : "   <-- MISMATCH");
        if (!ok) std::printf("        wanted plan %u tiles %u\n", w.plan_blocks, w.tile_blocks);
        bad += !ok;
    }
    return bad;
}

}  // namespace

int main() {
    using enet::MODE_OPEN;
    using enet::MODE_SEAL;
    using enet::MODE_XOR;
    const Row rows[] = {
        // auto (-1): long records (hint >= 256 KiB) take the tiles; uniform in batch order is one launch
        {1, -1, MODE_XOR, false, 4, 300 * KiB, 4 * 300 * KiB, LongRoute::UniformXor, kAny},
        {2, -1, MODE_XOR, true, 4, 300 * KiB, 4 * 300 * KiB, LongRoute::PlanTiles, 262144},
        {3, -1, MODE_SEAL, false, 8, 1 * MiB, 8 * MiB, LongRoute::UniformAead, kAny},
        {4, -1, MODE_OPEN, false, 4, 300 * KiB, 1 * MiB, LongRoute::PlanTiles, kAny},
        {5, -1, MODE_SEAL, false, 4, 262143, 4 * 262143ull, LongRoute::RecordEngine, kAny},
        // uniform and wide: count * 16 lanes >= 131 072 stays with the record engine
        {6, -1, MODE_SEAL, false, 8192, 262144, 8192 * 262144ull, LongRoute::RecordEngine, kAny},
        {7, -1, MODE_SEAL, false, 8191, 262144, 8191 * 262144ull, LongRoute::UniformAead, kAny},
        {8, -1, MODE_XOR, false, 8192, 262144, 8192 * 262144ull - 1, LongRoute::PlanTiles, kAny},
        // forced settings
        {9, INT64_MAX, MODE_SEAL, false, 1, 32 * MiB, 32 * MiB, LongRoute::RecordEngine, kAny},
        {10, 0, MODE_XOR, false, 12, 262244, 1000000, LongRoute::PlanTiles, 0},
        {11, 1000, MODE_SEAL, false, 5, 500, 2500, LongRoute::PlanTiles, 1000},
        // 40000 * 65536 tiles >= 0x7FFFFFFF: the AEAD launch's tile cap
        {12, 0, MODE_SEAL, false, 40000, 4294967295ull, 40000 * 4294967295ull, LongRoute::PlanTiles, kAny},
        // hints 0 / 0 mean "unknown", not "uniform of length 0": a one-launch route sized by them
        // would hold no tile and write nothing.  Planned instead (rows 22, 23: seal and open).
        {13, 0, MODE_XOR, false, 3, 0, 0, LongRoute::PlanTiles, 0},
        // the frame modes (3, 4) never take the tiles
        {14, -1, 3, false, 4, 300 * KiB, 4 * 300 * KiB, LongRoute::RecordEngine, kAny},
        // the XOR launch has row 12's tile cap too (its grid would not launch)
        {15, 0, MODE_XOR, false, 40000, 4294967295ull, 40000 * 4294967295ull, LongRoute::PlanTiles, kAny},
        // beyond the issue's rows: the other side of each threshold
        {16, -1, MODE_OPEN, false, 4, 262144, 4 * 262144ull, LongRoute::UniformAead, 262144},
        {17, -1, MODE_XOR, false, 8192, 262144, 8192 * 262144ull, LongRoute::RecordEngine, kAny},
        {18, 1000, MODE_SEAL, false, 5, 1000, 5000, LongRoute::UniformAead, 1000},
        {19, 1000, MODE_OPEN, true, 5, 1000, 5000, LongRoute::PlanTiles, 1000},
        {20, INT64_MAX, MODE_XOR, false, 4, 300 * KiB, 4 * 300 * KiB, LongRoute::RecordEngine, (uint64_t)INT64_MAX},
        {21, 0, 4, false, 4, 300 * KiB, 4 * 300 * KiB, LongRoute::RecordEngine, kAny},
        {22, 0, MODE_SEAL, false, 3, 0, 0, LongRoute::PlanTiles, 0},
        {23, 0, MODE_OPEN, false, 3, 0, 0, LongRoute::PlanTiles, 0},
        // unknown hints under the automatic rule never want the tiles; a known length under
        // setting 0 is still one launch, and the largest tile count under the cap is too
        {24, -1, MODE_SEAL, false, 3, 0, 0, LongRoute::RecordEngine, kAny},
        {25, 0, MODE_XOR, false, 3, 1, 3, LongRoute::UniformXor, 0},
        {26, 0, MODE_XOR, false, 32767, 4294967295ull, 32767 * 4294967295ull, LongRoute::UniformXor, kAny},
        {27, 0, MODE_XOR, false, 32768, 4294967295ull, 32768 * 4294967295ull, LongRoute::PlanTiles, kAny},
    };
    int bad = 0;
    for (const Row& w : rows) {
        const enet::RouteChoice c =
            enet::choose_long_route(w.mode, w.order, w.count, (uint32_t)w.M, w.S, w.setting);
        const bool ok = c.route == w.want && (w.want_long_min == kAny || c.long_min == w.want_long_min);
        std::printf("row %2d: %-12s long_min %llu%s\n", w.id, name(c.route), (unsigned long long)c.long_min,
                    ok ? "" : "   <-- MISMATCH");
        if (!ok) {
            std::printf("        wanted %s", name(w.want));
            if (w.want_long_min != kAny) std::printf(", long_min %llu", (unsigned long long)w.want_long_min);
            std::printf("\n");
            ++bad;
        }
    }
    bad += layout_rows();
    bad += grid_rows();
    return bad ? 1 : 0;
}
