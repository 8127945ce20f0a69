// host_batch.hpp -- the host-memory batch runtime: records that start and end in HOST memory
// (socket / relay buffers, chunk files: SessionManager.cpp:337-388, 703-854; Node.cpp:1414-1417,
// 1641-1655) through the MI355X kernels, at PCIe rate.
//
// An engine belongs to one device (a pipeline owns one; crypto::batch calls share a small set per
// device).  A job (one crypto::batch call, one enet_pipeline_* call) is cut into chunks on record
// boundaries; every chunk goes through S slots of pinned, device-mapped staging:
//     gather  (host worker threads: caller records -> the slot's pinned arena, per-record small
//              arrays rebased into the slot's pinned small block)
//     device  (the kernel(s), reading / writing the pinned staging over PCIe or the device arenas
//              behind SDMA copies -- see Mode)
//     scatter (host worker threads: the slot's pinned output -> the caller's records / vectors,
//              small outputs -> the caller's arrays)
// and the three stages of consecutive chunks overlap.  The staging lives on the device's NUMA
// node and the worker threads run on that node's CPUs, sized from the process's CPU budget
// (host_topo.hpp).  Inputs and outputs that are already
// device-accessible (pinned by hipHostMalloc / enet_host_alloc, or registered) skip the
// gather / scatter copies: the device stage works on them in place.
#pragma once

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <span>
#include <vector>

namespace enet::hb {

// ENET_HOST_TRACE=1: one stderr line per job / per queue with where its wall time went (diagnosis)
inline bool trace_on() {
    static const bool v = [] {
        const char* e = std::getenv("ENET_HOST_TRACE");
        return e && e[0] == '1';
    }();
    return v;
}
inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

enum class Op : int {
    Xor,           // ChaCha20::apply (counters: start counter per record, nullable = 0)
    AeadSeal,      // RFC 8439 seal -> tags_out
    AeadOpen,      // RFC 8439 open (tags_in) -> ok_out
    AeadHmacSeal,  // C5: AEAD + HMAC-SHA256(key, pt) -> tags_out, macs_out
    AeadHmacOpen,  // C5 open: tags_in, macs_in -> ok_out
    FrameSeal,     // body = ChaCha20_{K,N,0}(m || HMAC_K(m)); |out| = |in| + 32
    FrameOpen,     // -> macs_out (nullable), ok_out; |out| = |in| - 32
    WireSeal,      // nonce || BE32 || body; |out| = |in| + 48
    WireOpen,      // nonce from the frame -> ok_out; |out| = |in| - 48
    ChunkStore,    // ChaCha20 from LE32(id) + SHA-256(pt) -> macs_out (chunk hashes); ids given
    ChunkFetch,    // decrypt + SHA-256 check against macs_in -> ok_out
};

// |out_i| as a function of |in_i|
int64_t out_delta(Op op);

// A copy into pinned staging the device reads next: AVX-512 non-temporal stores from 512 bytes
// (no read-for-ownership of the destination, the caches left to the caller), memcpy below.  The
// caller issues a store fence (_mm_sfence) before publishing the bytes.
void copy_streaming(uint8_t* d, const uint8_t* s, size_t n);

struct Job {
    Op op = Op::Xor;
    size_t n = 0;
    // input record i: in_spans[i] when in_spans is non-empty, else in_base[in_off[i] .. in_off[i+1])
    std::span<const std::span<const uint8_t>> in_spans;
    const uint8_t* in_base = nullptr;
    const uint64_t* in_off = nullptr;
    // output record i (|out_i| = max(0, |in_i| + out_delta(op))): out_vecs[i] (resized here) when
    // set, else out_base[out_off[i] .. out_off[i+1]) (the caller's offsets must give that length)
    std::vector<std::vector<uint8_t>>* out_vecs = nullptr;
    // ... or out_each[i] (one caller-owned vector per record, e.g. queued requests; resized here)
    std::span<std::vector<uint8_t>* const> out_each;
    uint8_t* out_base = nullptr;
    const uint64_t* out_off = nullptr;
    // per-record small inputs (host memory)
    const uint8_t* keys = nullptr;      // [n][32]; [1][32] when key_stride == 0; the table for sessions
    uint32_t key_stride = 32;
    const uint8_t* nonces = nullptr;    // [n][12] (WireOpen: unused)
    const uint32_t* counters = nullptr; // Xor: [n] start counters, nullable
    const uint8_t* tags_in = nullptr;   // [n][16]
    const uint8_t* macs_in = nullptr;   // [n][32]: AeadHmacOpen MACs, ChunkFetch expected hashes
    const uint8_t* ids = nullptr;       // [n][32]: chunk ids (ChunkStore / ChunkFetch)
    // session-keyed frames (WireSeal / WireOpen): keys is a table of n_sessions keys
    const uint32_t* session = nullptr;
    uint32_t n_sessions = 0;
    // per-record small outputs (host memory, nullable where the op allows)
    uint8_t* tags_out = nullptr;        // [n][16]
    uint8_t* macs_out = nullptr;        // [n][32]
    uint8_t* ok_out = nullptr;          // [n]
};

// How the device stage moves the bytes (enet_host_set_mode; ENET_HOST_MODE=zc|splitk|zcout):
//   ZeroCopy    -- the kernels read the pinned input and write the pinned output directly over
//                  PCIe (no DMA, no device arenas); both directions move at once inside one launch
//   SdmaSplitK  -- H2D copies on an "up" stream, the kernels on their own stream(s) (two for
//                  hash-chain-bound jobs, so consecutive chunks' ~2 ms chains overlap), D2H copies
//                  on a "down" stream, events between them: neither copy direction ever waits
//                  behind a kernel and no two streams share one of the box's four hardware queues
//   SdmaInZcOut -- H2D by SDMA as SdmaSplitK, the kernels writing their outputs straight into
//                  pinned host memory (no D2H copies at all)
// Values 1 and 2 (per-slot SDMA round trips, every kernel on the H2D stream) were measured and
// retired in round 5 (DESIGN_HISTORY.md); the numbering is kept for the C ABI.
enum class Mode : int { ZeroCopy = 0, SdmaSplitK = 3, SdmaInZcOut = 4 };
bool valid_mode(int m);

struct Config {
    uint64_t chunk_bytes = 0;  // 0: the mode's default
    uint32_t slots = 0;        // 0: the mode's default
    int mode = -1;             // -1: process default (env / enet_host_set_mode / probe)
};

class Engine;
Engine* create_engine(int dev, const Config& cfg);
void destroy_engine(Engine* e);
// Runs the job to completion; throws std::invalid_argument / std::runtime_error / std::bad_alloc.
void run(Engine& e, const Job& job);
// The crypto::batch calls of the whole process: a job runs on a free engine of the device's
// shared set (up to kSharedEngines, created on demand), so concurrent callers do not queue behind
// one another's gather / scatter.
constexpr unsigned kSharedEngines = 4;
void run_shared(int dev, const Job& job);

// The fixed mode (ENET_HOST_MODE, else enet_host_set_mode), or -1: auto.  Auto runs SdmaSplitK,
// except for jobs whose output the device writes in place (caller-pinned output arenas): there
// the better of SdmaSplitK and SdmaInZcOut depends on the HIP runtime the process loaded
// (PyTorch's bundled runtime ran C2 at 29.5 / 35.6 GiB/s per direction in modes 3 / 4, the system
// runtime 39.7 / 36.6; gathered output 35-36 / 33.6 on torch's), so each device's first
// such jobs of >= 64 MiB alternate the two modes, two each, and the better rate is kept.
int fixed_mode();
void set_default_mode(int m);  // 0 / 3 / 4 fixed; -1 auto (forgets the decisions)
struct AutoRates {
    double splitk_gibs = 0, zcout_gibs = 0;  // best job rate seen in each mode
    int samples_splitk = 0, samples_zcout = 0;
    int mode = -1;                           // the decision (-1: not yet)
    unsigned epoch = 0;
};
// The decision from the two rates (pure; CPU-tested): 4 when it is > 3 % faster, else 3; -1
// while either is missing
int mode_for(const AutoRates& r);
AutoRates auto_rates(int dev);
// A synthetic A/B on `dev` (256 MiB of 4 KiB AEAD seals, pinned in and out, best of three per
// mode) whose decision becomes the device's auto decision
AutoRates probe_mode(int dev);

struct EngineStats {
    uint64_t jobs = 0, chunks = 0, records = 0, in_bytes = 0, out_bytes = 0;
    uint64_t gathered_bytes = 0, scattered_bytes = 0;  // copied by the host workers
    uint64_t direct_in = 0, direct_out = 0;             // chunks whose side ran in place
    uint64_t pinned_bytes = 0;                          // staging this engine holds
    int device_node = -1;    // NUMA node of the device (-1 unknown)
    int target_node = -1;    // node the staging is placed on (-1: hipHostMalloc decides)
    int staging_node = -1;   // node its first staging page actually is on (-1 none / unknown)
    uint32_t workers = 0;    // pool threads (0 until the first gather / scatter)
    uint32_t cpu_budget = 0;
    int spin = 0;
    int mode = -1;           // mode of the last job
};
EngineStats stats(const Engine& e);

}  // namespace enet::hb
