// long_records.cpp -- routing of a batch between the record engine and the sequence-parallel
// path (segments.hip) for long records, and the scratch memory that path needs.
#include "long_records.hpp"

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

namespace enet {
namespace {

std::atomic<int64_t> g_seg_min{-1};      // enet_set_seg_min (long_route.hpp seg_min_setting)
std::atomic<uint64_t> g_seg_batches{0};  // batches that took the tiles (enet_seg_batches)

// One grow-only buffer from scratch_pool().
struct Buf {
    void* ptr = nullptr;
    size_t cap = 0;
};

// Per-stream state of the tile paths, one per (device, raw stream handle), grown on demand,
// stream-ordered, and otherwise reused: a launch makes no allocation (a stream-ordered allocate /
// free pair per call cost ~4 us of gap between launches).
//   counters: arrival counters of the one-launch AEAD path (seg_uniform_aead_kernel), zeroed when
//     allocated and reset by each record's last arriver, so they are zero whenever a launch on
//     that stream starts;
//   partials: that path's per-tile partials;
//   plan: the plan + tiles path's scratch (seg_begin), all initialised by the plan kernel.
// Assumes the handle names ONE in-order queue, executing eagerly, whose calls are issued one at
// a time: then the launches that share a buffer run in order, and a buffer replaced on growth is
// freed behind its last user.  Not so for hipStreamPerThread or NULL under a
// per-thread default stream (one handle, concurrent queues: launches race on counters and
// partials), under graph capture (the table keeps a graph-owned allocation), and for two threads
// on one stream when one of them grows a buffer the other's launch is about to use.
struct StreamScratch {
    int dev;
    hipStream_t st;
    Buf counters, partials, plan;
};

// The calling stream's scratch; lk holds the table's mutex on success, for as long as s is used.
int scratch_of(hipStream_t st, std::unique_lock<std::mutex>& lk, StreamScratch*& s) {
    static std::mutex mu;
    static std::vector<StreamScratch> table;
    int dev = 0;
    if (hipError_t e = hipGetDevice(&dev)) return hip_status(e, "aead tiles: hipGetDevice");
    lk = std::unique_lock<std::mutex>(mu);
    auto it = std::find_if(table.begin(), table.end(), [&](auto& x) { return x.dev == dev && x.st == st; });
    if (it == table.end()) it = table.insert(it, StreamScratch{dev, st, {}, {}, {}});
    s = &*it;
    return ENET_OK;
}

// b holds at least `bytes` afterwards: reused, or replaced by max(bytes, floor) fresh bytes
// (zeroed if `zero`), the old buffer freed on the caller's stream.  path names the caller in
// the no-pool error.
int grow(Buf& b, size_t bytes, size_t floor, bool zero, hipStream_t st, const char* what, const char* path) {
    if (b.cap >= bytes) return ENET_OK;
    hipMemPool_t pool = scratch_pool();
    if (!pool) return fail(ENET_EHIP, (std::string(path) + ": no memory pool for the current device").c_str());
    const size_t cap = std::max(bytes, floor);
    void* mem = nullptr;
    if (hipError_t e = hipMallocFromPoolAsync(&mem, cap, pool, st)) return hip_status(e, what);
    if (zero)
        if (hipError_t e = hipMemsetAsync(mem, 0, cap, st)) return hip_status(e, what);
    if (b.ptr) (void)hipFreeAsync(b.ptr, st);
    b.ptr = mem;
    b.cap = cap;
    return ENET_OK;
}

// Every field RecParams and SegParams share; the caller adds its scratch pointers and caps.
// More than some routes had copied by hand, to no effect: the uniform routes run only with
// order == nullptr, the AEAD kernels ignore counters (seg_counter is 1 for them), and aad, tag_in,
// tag_out and ok are null in an XOR RecParams.
SegParams seg_params(int mode, const RecParams& p) {
    SegParams q{};
    q.mode = mode;
    q.n = p.n;
    q.in_off = p.in_off;
    q.out_off = p.out_off;
    q.in = p.in;
    q.out = p.out;
    q.keys = p.keys;
    q.key_stride = p.key_stride;
    q.nonces = p.nonces;
    q.counters = p.counters;
    q.counter_stride = p.counter_stride;
    q.aad = p.aad;
    q.aad_off = p.aad_off;
    q.tag_in = p.tag_in;
    q.tag_out = p.tag_out;
    q.ok = p.ok;
    q.order = p.order;
    return q;
}

// RFC 8439 seal / open over a batch the hints call uniform and long: one launch (the last tile
// of each record to arrive combines, and zeroes a failed open itself)
int run_uniform_aead(int mode, const enet_records* r, const RecParams& p, hipStream_t st, const char* what) {
    const uint64_t L = r->max_len_hint;
    const uint64_t tiles = (uint64_t)r->count * ((L + kSegTileBytes - 1) / kSegTileBytes);
    const uint64_t words = (uint64_t)r->count * seg_uniform_arrival_words();
    if (words > UINT32_MAX) return fail(ENET_EINVAL, "aead tiles: too many records for one launch");
    std::unique_lock<std::mutex> lk;
    StreamScratch* s = nullptr;
    if (int e = scratch_of(st, lk, s)) return e;
    if (int e = grow(s->counters, 4 * (size_t)words, 4 * 1024, true, st, "aead tiles: counters", "aead tiles")) return e;
    if (int e = grow(s->partials, (size_t)tiles * 32, 64u << 10, false, st, "aead tiles: scratch", "aead tiles")) return e;
    uint32_t* arrivals = static_cast<uint32_t*>(s->counters.ptr);
    uint32_t* partials = static_cast<uint32_t*>(s->partials.ptr);
    lk.unlock();
    SegParams q = seg_params(mode, p);
    q.partials = partials;
    g_seg_batches.fetch_add(1, std::memory_order_relaxed);
    return hip_status(launch_seg_uniform_aead(q, L, arrivals, st), what);
}

// Plan + tile kernels for the batch's long records; p.skip marks them for the record engine.
int seg_begin(int mode, const enet_records* r, RecParams& p, uint64_t long_min, hipStream_t st) {
    const uint32_t n = r->count;
    // capacities from the hints, one claim byte per position of the launch (long_route.hpp)
    const SegLayout lay = seg_layout(n, r->max_len_hint, r->total_bytes_hint, long_min);
    std::unique_lock<std::mutex> lk;
    StreamScratch* s = nullptr;
    if (int e = scratch_of(st, lk, s)) return e;
    if (int e = grow(s->plan, (size_t)lay.bytes, 256u << 10, false, st, "sequence-parallel scratch", "sequence-parallel scratch")) return e;
    uint8_t* base = static_cast<uint8_t*>(s->plan.ptr);
    lk.unlock();
    SegParams q = seg_params(mode, p);
    q.hdr = reinterpret_cast<unsigned long long*>(base);
    q.entries = reinterpret_cast<SegEntry*>(base + lay.o_ent);
    q.claimed = base + lay.o_cl;
    q.partials = reinterpret_cast<uint32_t*>(base + lay.o_part);
    q.entry_cap = (uint32_t)lay.ecap;
    q.tile_cap = (uint32_t)lay.tcap;
    q.long_min = long_min;
    const SegGrid grid = seg_grid(n, lay);  // capped: both kernels stride past the caps
    p.skip = q.claimed;
    // per-lane path: the staged paths assume every record is theirs.  It also makes the record
    // engine ONE launch over positions 0 .. n-1 (rec_base == 0), which is what lets the plan
    // kernel and records_body agree on claimed[position]
    p.uniform_len = 0;
    g_seg_batches.fetch_add(1, std::memory_order_relaxed);
    return hip_status(launch_seg(q, grid.plan_blocks, grid.tile_blocks, st), "sequence-parallel launch");
}

}  // namespace

void set_seg_min(int64_t bytes) { g_seg_min.store(bytes, std::memory_order_relaxed); }
uint64_t seg_batches() { return g_seg_batches.load(std::memory_order_relaxed); }

// Scratch comes from a library-private, stream-ordered pool per device (hipMallocFromPoolAsync /
// hipFreeAsync on the caller's stream): no synchronisation, capturable, and concurrent calls on
// different streams get their own.  Freed memory stays in the pool.
hipMemPool_t scratch_pool() {
    static std::mutex mu;
    static hipMemPool_t pools[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!pools[dev]) {
        hipMemPoolProps props{};
        props.allocType = hipMemAllocationTypePinned;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        hipMemPool_t pl = nullptr;
        if (hipMemPoolCreate(&pl, &props) != hipSuccess) return nullptr;
        uint64_t keep = UINT64_MAX;
        (void)hipMemPoolSetAttribute(pl, hipMemPoolAttrReleaseThreshold, &keep);
        pools[dev] = pl;
    }
    return pools[dev];
}

int run_records(int mode, const enet_records* r, RecParams& p, hipStream_t st, const char* what) {
    const RouteChoice c = choose_long_route(mode, r->order != nullptr, r->count, r->max_len_hint,
                                            r->total_bytes_hint, g_seg_min.load(std::memory_order_relaxed));
    switch (c.route) {
    case LongRoute::UniformXor:  // a record that is not as hinted is run whole by its tile-0 workgroup
        g_seg_batches.fetch_add(1, std::memory_order_relaxed);
        return hip_status(launch_seg_uniform_xor(seg_params(mode, p), r->max_len_hint, st), what);
    case LongRoute::UniformAead:
        return run_uniform_aead(mode, r, p, st, what);
    case LongRoute::PlanTiles:
        if (int e = seg_begin(mode, r, p, c.long_min, st)) return e;
        break;
    case LongRoute::RecordEngine: break;
    }
    const uint32_t lanes = choose_lanes(r->count, r->total_bytes_hint, r->max_len_hint);
    return hip_status(launch_records(mode, p, lanes, st), what);
}

}  // namespace enet
