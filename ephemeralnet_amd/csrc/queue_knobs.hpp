// queue_knobs.hpp -- every hook the tools build (-DENET_TOOLS_BUILD, libenet_crypto_tools.so) adds
// to the frame queues, and every ENET_QUEUE_* variable it reads.  The product build sees only the
// empty inlines and the constants at the bottom.
//   ENET_QUEUE_FAKE_US=<us>   a stand-in for the device on a CPU-only host: a pass "runs" for that
//                             long and computes nothing (outputs are garbage, opens report ok), so
//                             the submitting threads' CPU per frame can be measured without a GPU
//                             (tools/queue_bench)
//   ENET_QUEUE_FAKE_COMPUTE=1 ... and the worker computes it on the host engine first (real bytes:
//                             tests/cpp/queue_stress checks device-style passes, evictions
//                             included, on a CPU-only host)
//   ENET_QUEUE_PROF=1         TSC cycles per phase of submit() / get(), summed over threads,
//                             printed at exit
//   ENET_QUEUE_STALL_OVERFLOW_US=<us>  a submitter whose reservation found its pass full sleeps
//                             that long before closing it -- the preemption window of ADVICE r05's
//                             stale close, made wide for tests/cpp/queue_stress
//   ENET_QUEUE_STAGE=0 / 1    force zero-copy / staged device passes
//   ENET_QUEUE_SHARDS=1..8, ENET_QUEUE_SHARD_BY=l3 | thread   the submitters' shards
//   ENET_QUEUE_AUTO_BACKLOG=<frames>   AUTO's per-thread backlog threshold
#pragma once

#include <cstdint>

#ifdef ENET_TOOLS_BUILD
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include <immintrin.h>
#endif

namespace enet::fq {

// the phases the profile times
enum Phase : int {
    kSubmitState, kSubmitReserve, kSubmitFill, kSubmitNotify, kGetClaim, kGetWait, kGetCopy, kGetRelease,
    kSubmitOpenPass, kSubmitPassFull, kOpenLock, kOpenReuse, kOpenAllocate, kOpenWait, kOpenRaced,
    kGetReleaseStore, kPhases
};

#ifdef ENET_TOOLS_BUILD
inline int env_int(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}
inline double fake_us() {
    static const double v = [] {
        const char* e = std::getenv("ENET_QUEUE_FAKE_US");
        return e ? std::atof(e) : 0.0;
    }();
    return v;
}

inline const char* const kPhaseName[kPhases] = {"submit: ticket state", "submit: reserve (atomic add)",
                                                "submit: fill slot", "submit: notify", "get: claim",
                                                "get: wait (pass not done)", "get: copy result", "get: release",
                                                "submit: open a pass", "submit: pass full / closed",
                                                "open_pass: lock mu_", "open_pass: reuse a released pass",
                                                "open_pass: allocate a pass", "open_pass: wait for a pass",
                                                "open_pass: another opened it", "get: release store"};
inline std::atomic<std::uint64_t> g_prof_c[kPhases], g_prof_n[kPhases];
inline bool prof_on() {
    static const bool v = std::getenv("ENET_QUEUE_PROF") != nullptr;
    return v;
}
struct ProfThread {
    std::uint64_t c[kPhases] = {}, n[kPhases] = {};
    ~ProfThread() {
        for (int i = 0; i < kPhases; ++i) {
            g_prof_c[i] += c[i];
            g_prof_n[i] += n[i];
        }
    }
};
inline ProfThread& thread_prof() {
    thread_local ProfThread p;
    return p;
}
struct ProfReport {
    ~ProfReport() {
        if (!prof_on()) return;
        const auto w0 = std::chrono::steady_clock::now();
        const std::uint64_t c0 = __rdtsc();
        while (std::chrono::steady_clock::now() - w0 < std::chrono::milliseconds(20)) {
        }
        const double ghz = (double)(__rdtsc() - c0) / 2e7;
        for (int i = 0; i < kPhases; ++i)
            std::fprintf(stderr, "[enet queue prof] %-26s %12llu calls %8.1f ns/call %8.3f s\n", kPhaseName[i],
                         (unsigned long long)g_prof_n[i].load(),
                         (double)g_prof_c[i].load() / ghz / std::max<double>(1, (double)g_prof_n[i].load()),
                         (double)g_prof_c[i].load() / ghz * 1e-9);
    }
};
inline ProfReport g_prof_report;
inline std::uint64_t prof_t() { return prof_on() ? __rdtsc() : 0; }
inline void prof_add(Phase i, std::uint64_t& t0) {
    if (!prof_on()) return;
    const std::uint64_t t = __rdtsc();
    thread_prof().c[i] += t - t0;
    thread_prof().n[i] += 1;
    t0 = t;
}
inline void stall_overflow() {
    static const int us = env_int("ENET_QUEUE_STALL_OVERFLOW_US", 0);
    if (us > 0) std::this_thread::sleep_for(std::chrono::microseconds(us));
}
// The stand-in device's pass: `compute` it (ENET_QUEUE_FAKE_COMPUTE) or report every open ok
// (`ok`: the pass's n ok bytes, null when sealing), then let fake_us() pass
template <class Compute>
void fake_device_pass(Compute&& compute, std::uint8_t* ok, std::uint32_t n) {
    const auto t0 = std::chrono::steady_clock::now();
    if (std::getenv("ENET_QUEUE_FAKE_COMPUTE")) compute();
    else if (ok) std::memset(ok, 1, n);
    while (std::chrono::steady_clock::now() - t0 < std::chrono::duration<double, std::micro>(fake_us()))
        std::this_thread::sleep_for(std::chrono::microseconds(20));
}
// -1: not forced
inline int stage_override() {
    static const int v = env_int("ENET_QUEUE_STAGE", -1);
    return v;
}
inline unsigned shards_override(unsigned dflt, unsigned max) {
    return std::min<unsigned>(max, (unsigned)std::max(1, env_int("ENET_QUEUE_SHARDS", (int)dflt)));
}
inline bool shard_by_l3_override(bool dflt) {
    const char* e = std::getenv("ENET_QUEUE_SHARD_BY");
    return e ? std::strcmp(e, "l3") == 0 : dflt;
}
inline std::int32_t auto_backlog_override(std::int32_t dflt) { return env_int("ENET_QUEUE_AUTO_BACKLOG", dflt); }
#else
constexpr double fake_us() { return 0.0; }
inline std::uint64_t prof_t() { return 0; }
inline void prof_add(Phase, std::uint64_t&) {}
inline void stall_overflow() {}
template <class Compute>
void fake_device_pass(Compute&&, std::uint8_t*, std::uint32_t) {}
constexpr int stage_override() { return -1; }
constexpr unsigned shards_override(unsigned dflt, unsigned) { return dflt; }
constexpr bool shard_by_l3_override(bool dflt) { return dflt; }
constexpr std::int32_t auto_backlog_override(std::int32_t dflt) { return dflt; }
#endif

}  // namespace enet::fq
