// records.hip -- record kernels and their launch scheduling (gfx950); the body is in
// records_body.hpp.
#include <atomic>

#include "record_route.hpp"
#include "records_body.hpp"

namespace enet {


template <int LOGP, int MODE, int FRAME, int COOP>
__global__ __launch_bounds__(kWG) void records_kernel(RecParams p) {
    records_body<LOGP, MODE, FRAME, COOP>(p);
}

// 512-thread workgroups with the lockstep keystream (COOP 5, run staging)
template <int LOGP, int MODE>
__global__ __launch_bounds__(512) void records_kernel_l(RecParams p) {
    records_body<LOGP, MODE, FR_NONE, 5>(p);
}

// records handed to launches of each RecordKind in this process (enet_record_route_counts)
static std::atomic<uint64_t> g_route_records[kRecordKinds];

void record_route_counts(uint64_t out[kRecordKinds]) {
    for (int k = 0; k < kRecordKinds; ++k) out[k] = g_route_records[k].load(std::memory_order_relaxed);
}

static_assert(kRouteWG == (uint32_t)kWG, "record_route.hpp and the record kernels disagree on the workgroup");

template <int LOGP, int MODE, int FRAME>
static hipError_t launch_one(const RecParams& p, hipStream_t s) {
    const uint64_t lanes = (uint64_t)p.n << LOGP;
    const uint32_t blocks = (uint32_t)((lanes + kWG - 1) / kWG);
    if (blocks == 0) return hipSuccess;
    // which kernel runs the whole workgroups, and how many records are left for the per-lane one
    const RecordRoute rt = choose_record_route(LOGP, FRAME == FR_NONE, p.n, p.uniform_len, p.order != nullptr,
                                               p.coop, p.coop_lines, p.lockstep, p.stream);
    if (rt.kind == RecordKind::PerLane) {
        g_route_records[(int)RecordKind::PerLane].fetch_add(p.n, std::memory_order_relaxed);
        hipLaunchKernelGGL((records_kernel<LOGP, MODE, FRAME, 0>), dim3(blocks), dim3(kWG), 0, s, p);
        return hipGetLastError();
    }
    if constexpr (FRAME == FR_NONE) {
        RecParams q = p;
        q.n = rt.full * rt.per_wg;
        g_route_records[(int)rt.kind].fetch_add(q.n, std::memory_order_relaxed);
        switch (rt.kind) {
            case RecordKind::Stream:
                if (hipError_t e = launch_stream(MODE, q, 1u << LOGP, rt.full, s)) return e;
                break;
            case RecordKind::LineStaged:
                hipLaunchKernelGGL((records_kernel<0, MODE, FR_NONE, 4>), dim3(rt.full), dim3(kWG), 0, s, q);
                break;
            case RecordKind::Lockstep:
                hipLaunchKernelGGL((records_kernel_l<LOGP, MODE>), dim3(rt.full), dim3(512), 0, s, q);
                break;
            default:
                hipLaunchKernelGGL((records_kernel<LOGP, MODE, FR_NONE, 1>), dim3(rt.full), dim3(kWG), 0, s, q);
                break;
        }
        if (rt.rest) {
            RecParams r = p;
            r.n = rt.rest;
            r.rec_base = rt.full * rt.per_wg;
            g_route_records[(int)RecordKind::PerLane].fetch_add(rt.rest, std::memory_order_relaxed);
            hipLaunchKernelGGL((records_kernel<LOGP, MODE, FR_NONE, 0>),
                               dim3((uint32_t)((((uint64_t)rt.rest << LOGP) + kWG - 1) / kWG)),
                               dim3(kWG), 0, s, r);
        }
    }
    return hipGetLastError();
}

template <int MODE, int FRAME>
static hipError_t launch_mode(const RecParams& p, uint32_t lanes, hipStream_t s) {
    switch (lanes) {
        case 1: return launch_one<0, MODE, FRAME>(p, s);
        case 2: return launch_one<1, MODE, FRAME>(p, s);
        case 4: return launch_one<2, MODE, FRAME>(p, s);
        case 8: return launch_one<3, MODE, FRAME>(p, s);
        case 16: return launch_one<4, MODE, FRAME>(p, s);
        default: return hipErrorInvalidValue;
    }
}

// mode: MODE_XOR / MODE_SEAL / MODE_OPEN, plus frame variants encoded as 3 (seal) / 4 (open)
hipError_t launch_records(int mode, const RecParams& p, uint32_t lanes, hipStream_t s) {
    switch (mode) {
        case MODE_XOR: return launch_mode<MODE_XOR, FR_NONE>(p, lanes, s);
        case MODE_SEAL: return launch_mode<MODE_SEAL, FR_NONE>(p, lanes, s);
        case MODE_OPEN: return launch_mode<MODE_OPEN, FR_NONE>(p, lanes, s);
        case 3: return launch_mode<MODE_XOR, FR_SEAL>(p, lanes, s);
        case 4: return launch_mode<MODE_XOR, FR_OPEN>(p, lanes, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace enet
