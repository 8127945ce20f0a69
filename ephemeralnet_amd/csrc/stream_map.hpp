// stream_map.hpp -- which record and which record-lane each of the 512 record lanes of a streaming
// workgroup (stream.hip) serves, and which of them each memory-wave instruction moves.  No HIP
// here: the host test compiles this header alone (tests/cpp/stream_map_table.cpp); the functions
// are constexpr, which hipcc compiles for both sides.
//
// A record of P = 1 << logp lanes: record-lane j owns bytes [j L/P, (j + 1) L/P).  A workgroup
// holds R = 512 >> logp records.  Thread t = 64 wave + lane serves record-lane j = t / R of record
// wg R + t % R: lane j of every record of the workgroup sits in wave group j, so j is uniform
// per wave for P <= 8 (C2, P = 2: waves 0-3 are j = 0, waves 4-7 j = 1) and per half-wave for
// P = 16, and what only one lane of a record has to do (the one-time key, the tag) whole waves skip.
#pragma once

#include <stdint.h>

namespace enet {

constexpr uint32_t kMapLanes = 512;  // record lanes per workgroup (kStreamLanes)
constexpr uint32_t kMapRun = 128;    // bytes a lane moves per stage (kRun)

struct StreamLane {
    uint32_t rec;  // record of the launch
    uint32_t j;    // lane of the record, 0 = its leader
};

// thread t (0..511) of workgroup wg
constexpr StreamLane stream_lane(int logp, uint32_t wg, uint32_t t) {
    const uint32_t R = kMapLanes >> logp;
    return {wg * R + (t & (R - 1u)), t >> (9 - logp)};
}

// the thread of a workgroup that serves record-lane j of its q-th record: stream_lane's inverse
constexpr uint32_t stream_thread(int logp, uint32_t q, uint32_t j) { return q + j * (kMapLanes >> logp); }

// arena offset (from the first record's start) of the lane's stage 0; stage st lies kMapRun st on
constexpr uint32_t stream_lane_offset(int logp, uint32_t L, StreamLane m) {
    return m.rec * L + m.j * (L >> logp);
}

// Memory wave m (0..3) moves the runs of compute waves 2m and 2m + 1 in 16 ops per stage: op s is
// instruction s & 7 of compute wave 2m + (s >> 3), 8 owners' whole 128-byte runs, its lane `lane`
// one 16-byte chunk of owner 8 (s & 7) + lane / 8 of that wave.  The thread that owns the chunk:
constexpr uint32_t stream_mem_owner(uint32_t m, int s, uint32_t lane) {
    return 64u * (2u * m + ((uint32_t)s >> 3)) + 8u * ((uint32_t)s & 7u) + (lane >> 3);
}

}  // namespace enet
