// The routing rule for long records (csrc/long_route.hpp choose_long_route) against a table
// worked out by hand from the rule: host C++ only, exit status 0 when every row agrees.
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
        // Known defect, pinned: the uniform routes do not require
        // max_len_hint != 0, so setting 0 with hints 0 / 0 is a UniformXor launch with L = 0, a
        // silent no-op.  The XOR route has no tile-count cap either (row 15).
        {13, 0, MODE_XOR, false, 3, 0, 0, LongRoute::UniformXor, kAny},
        // the frame modes (3, 4) never take the tiles
        {14, -1, 3, false, 4, 300 * KiB, 4 * 300 * KiB, LongRoute::RecordEngine, kAny},
        {15, 0, MODE_XOR, false, 40000, 4294967295ull, 40000 * 4294967295ull, LongRoute::UniformXor, kAny},
        // beyond the issue's rows: the other side of each threshold
        {16, -1, MODE_OPEN, false, 4, 262144, 4 * 262144ull, LongRoute::UniformAead, 262144},
        {17, -1, MODE_XOR, false, 8192, 262144, 8192 * 262144ull, LongRoute::RecordEngine, kAny},
        {18, 1000, MODE_SEAL, false, 5, 1000, 5000, LongRoute::UniformAead, 1000},
        {19, 1000, MODE_OPEN, true, 5, 1000, 5000, LongRoute::PlanTiles, 1000},
        {20, INT64_MAX, MODE_XOR, false, 4, 300 * KiB, 4 * 300 * KiB, LongRoute::RecordEngine, (uint64_t)INT64_MAX},
        {21, 0, 4, false, 4, 300 * KiB, 4 * 300 * KiB, LongRoute::RecordEngine, kAny},
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
    return bad ? 1 : 0;
}
