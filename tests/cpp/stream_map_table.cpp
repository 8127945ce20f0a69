// The lane map of the streaming kernel (csrc/stream_map.hpp) against its rule written out again
// here: thread t of a workgroup serves record-lane t / R of record wg R + t % R, R = 512 / P.
// Host C++ only, exit status 0 and " 0 mismatches" when everything agrees.
//   1. For P = 1..16 the map is a bijection from t in [0, 512) onto (record of the workgroup,
//      record-lane), stream_thread is its inverse, and the lane index is uniform per wave for
//      P <= 8 and per half-wave for P = 16.
//   2. For L in {128 P, 256 P, 4096} and every stage: the 128 bytes that op s of memory wave m
//      moves for one of its 8 owners are the stage's run of the thread whose LDS run the op lands
//      in (the memory wave's lane-linear 1 KiB group 1024 s of its 16 KiB part), by the compute
//      side's own offset rec L + j L / P + 128 st; every run lies inside [0, n L) for the first
//      and the last workgroup of the launch, and the runs of a launch tile [0, n L) exactly once.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "stream_map.hpp"

namespace {

int bad = 0;

void fail(const char* what, int logp, uint32_t a, uint32_t b, uint32_t c) {
    if (bad < 20) std::printf("MISMATCH %s: logp %d, %u %u %u\n", what, logp, a, b, c);
    ++bad;
}

void bijection(int logp) {
    const uint32_t P = 1u << logp, R = 512u / P;
    for (uint32_t wg : {0u, 1u, 255u, 70000u}) {
        std::vector<int> seen(512, 0);
        for (uint32_t t = 0; t < 512; ++t) {
            const enet::StreamLane m = enet::stream_lane(logp, wg, t);
            if (m.rec != wg * R + t % R || m.j != t / R) fail("rule", logp, wg, t, m.rec);
            if (m.j >= P || m.rec < wg * R || m.rec >= (wg + 1) * R) { fail("range", logp, wg, t, m.j); continue; }
            ++seen[(m.rec - wg * R) * P + m.j];
            if (enet::stream_thread(logp, m.rec - wg * R, m.j) != t) fail("inverse", logp, wg, t, m.j);
            // uniform per wave (P <= 8) or per half-wave (P = 16)
            const uint32_t first = logp < 4 ? (t & ~63u) : (t & ~31u);
            if (enet::stream_lane(logp, wg, first).j != m.j) fail("uniform", logp, wg, t, m.j);
        }
        for (uint32_t k = 0; k < 512; ++k)
            if (seen[k] != 1) fail("bijection", logp, wg, k, (uint32_t)seen[k]);
    }
}

void table(int logp, uint32_t L, uint32_t nwg) {
    const uint32_t P = 1u << logp, R = 512u / P, n = nwg * R;
    const uint32_t S = L / (128u * P);
    const uint64_t total = (uint64_t)n * L;
    std::vector<uint8_t> cover(nwg <= 2 ? total / 128 : 0, 0);
    for (uint32_t wg : {0u, nwg - 1}) {
        for (uint32_t m = 0; m < 4; ++m)
            for (int s = 0; s < 16; ++s)
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    // where the op's lane lands in the input slab: the owner of that LDS run
                    const uint32_t lds = 2u * m * 8192u + 1024u * (uint32_t)s + 16u * lane;
                    const uint32_t t = lds / 128u;
                    const uint32_t owner = enet::stream_mem_owner(m, s, lane);
                    if (owner != t || t / 64u != 2u * m + ((uint32_t)s >> 3) || t % 64u != 8u * ((uint32_t)s & 7u) + lane / 8u)
                        fail("owner", logp, m, (uint32_t)s, lane);
                    const uint32_t off = enet::stream_lane_offset(logp, L, enet::stream_lane(logp, wg, owner));
                    // the compute side's rule for thread t, from the formulas
                    const uint64_t rec = (uint64_t)wg * R + t % R, j = t / R;
                    const uint64_t want = rec * L + j * (L / P);
                    if (off != want) fail("offset", logp, wg, t, off);
                    for (uint32_t st = 0; st < S; ++st) {
                        const uint64_t at = want + 128ull * st;
                        if (at + 128 > total || at % 128 != 0) fail("bounds", logp, wg, t, st);
                        else if (!cover.empty() && lane % 8 == 0) ++cover[at / 128];
                    }
                }
        if (nwg == 1) break;
    }
    for (size_t k = 0; k < cover.size(); ++k)
        if (cover[k] != 1) fail("tiling", logp, (uint32_t)k, cover[k], L);
}

}  // namespace

int main() {
    int cases = 0;
    for (int logp = 0; logp <= 4; ++logp) {
        bijection(logp);
        const uint32_t P = 1u << logp;
        for (uint32_t L : {128u * P, 256u * P, 4096u}) {
            if (L % (128u * P)) continue;
            // one and two workgroups (every run of the launch counted), and the largest launch
            // whose arena stays below 4 GiB (32-bit offsets: the last workgroup's must not wrap)
            const uint32_t R = 512u / P;
            const uint32_t most = (uint32_t)(0xFFFFFFFFull / ((uint64_t)L * R));
            for (uint32_t nwg : {1u, 2u, most}) {
                table(logp, L, nwg);
                ++cases;
            }
        }
    }
    std::printf("stream map: %d cases, %d mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
