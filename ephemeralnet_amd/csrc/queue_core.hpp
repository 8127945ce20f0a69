// queue_core.hpp -- one direction of a frame queue: its passes, the submit path (inline: once per
// frame) and the workers that run the passes (queue_core.cpp).
#pragma once

#include <cstring>
#include <deque>

#include <hip/hip_runtime.h>
#include <sched.h>

#include "host_batch.hpp"
#include "host_topo.hpp"
#include "queue_knobs.hpp"
#include "queue_slots.hpp"

namespace enet::fq {

using ephemeralnet::crypto::batch::FrameQueueOptions;
using ephemeralnet::crypto::batch::FrameQueueStats;

inline double now_us() { return 1e6 * enet::hb::now_s(); }

// Submitting threads are spread over a few open passes (shards), each with its own reservation
// word: one shared word measured 3.6-4.7 failed compare-and-swaps per frame at 16 threads
// (profiles/r05b_queue_bench_cas.jsonl), and every attempt moves the cache line, across sockets too.
// Which shard a submitting thread uses: the L3 domain (CCD) of the CPU it runs on, modulo 8
// shards, so the threads sharing a reservation word and a pass's lines mostly share a cache (an
// atomic add or a slot write on a line another CCD owns is a cross-die transfer).  On the box,
// 16 threads x 256 frames in flight: 11.2-12.1 M frames/s at 0.45-0.49 us of CPU per frame vs
// 9.5-9.7 M at 0.53-0.60 with 4 shards by thread order (profiles/r05i_queue_shards.jsonl).
// Without L3 information in sysfs: the thread's arrival order.
constexpr unsigned kMaxShards = 8;
struct ShardPlan {
    unsigned n = shards_override(8, kMaxShards);
    // the CPU -> L3 map (read once, kept here: no call out of this unit per frame); null: by thread
    const std::vector<int>* l3 = shard_by_l3_override(true) ? &enet::topo::l3_of_cpu() : nullptr;
};
inline std::atomic<unsigned> g_next_shard{0};
inline unsigned my_shard(const ShardPlan& plan) {
    if (plan.l3) {
        const int c = sched_getcpu();
        const auto& m = *plan.l3;
        if (c >= 0 && (std::size_t)c < m.size() && m[(std::size_t)c] >= 0) return (unsigned)m[(std::size_t)c] % plan.n;
    }
    thread_local const unsigned s = g_next_shard.fetch_add(1, std::memory_order_relaxed);
    return s % plan.n;
}

class Core {
public:
    Core(const FrameQueueOptions& o, bool open_dir);
    // Stops the workers, runs what is left, and copies every uncollected result into its ticket:
    // tickets may outlive the queue
    ~Core();

    bool has_device() const { return has_device_; }
    FrameQueueStats stats();
    // a frame served on its caller's thread (host engine): one frame, one host pass
    void count_direct() { direct_.fetch_add(1, std::memory_order_relaxed); }

    // Reserve a slot of this thread's shard's open pass for `in` (one atomic add), fill it,
    // return its ticket
    FrameTicket submit(const std::uint8_t key[32], std::span<const std::uint8_t> in) {
        const std::uint64_t len = in.size();
        Shard& sh = shards_[my_shard(plan_)];
        std::uint64_t pt = prof_t();
        // the nonce is drawn before any slot is reserved: NonceSource::refill may throw
        // (std::random_device), and a reserved slot never filled would stall its pass's worker
        // in spin_until forever
        std::uint8_t nonce[12];
        if (!open_dir_) nonce_source().draw(nonce);
        auto* ts = new_state();
        ts->st.store(kInPass, std::memory_order_relaxed);
        count_submission(ts, open_dir_);
        prof_add(kSubmitState, pt);
        for (;;) {
            Pass* p = sh.open.load(std::memory_order_acquire);
            if (!p) {
                prof_add(kSubmitReserve, pt);
                open_pass(sh);
                prof_add(kSubmitOpenPass, pt);
                continue;
            }
            // the generation this reservation lands in, or an older one (then close_full below
            // leaves the pass alone; the retry reads the current one)
            const std::uint64_t g0 = p->gen.load(std::memory_order_acquire);
            const std::uint64_t v = p->res.fetch_add((1ull << kSlotShift) | len, std::memory_order_acq_rel);
            if (v & kClosedBit) {  // taken by a worker: the shard's next open pass
                prof_add(kSubmitReserve, pt);
                if (sh.open.load(std::memory_order_acquire) == p) std::this_thread::yield();
                prof_add(kSubmitPassFull, pt);
                continue;
            }
            const std::uint32_t idx = (std::uint32_t)((v >> kSlotShift) & kSlotMask);
            const std::uint64_t used = v & kBytesMask;
            if (idx >= p->cap_frames || used + len > p->cap_in) {
                // full: this and every later reservation of the pass is past its end; the first
                // one marks the cut (a slot index below capacity), whoever closes it runs it
                if (idx < p->cap_frames)  // the pass cannot run before this mark: its generation is still ours
                    p->recs[idx].fill.store(p->gen.load(std::memory_order_relaxed) << 2 | kOverflow, std::memory_order_release);
                overflows_.fetch_add(1, std::memory_order_relaxed);
                prof_add(kSubmitReserve, pt);
                stall_overflow();
                close_full(p, g0);
                prof_add(kSubmitPassFull, pt);
                continue;
            }
            if (idx == 0) p->first_us.store((std::int64_t)now_us(), std::memory_order_relaxed);
            prof_add(kSubmitReserve, pt);
            fill_slot(*p, idx, used, key, nonce, in, ts);
            prof_add(kSubmitFill, pt);
            if (idx == 0 || idx + 1 == target_frames_ || (used < target_bytes_ && used + len >= target_bytes_)) {
                std::lock_guard<std::mutex> lk(mu_);  // no lost wake-up: workers check under mu_
                work_cv_.notify_one();
                prof_add(kSubmitNotify, pt);
            }
            return FrameTicket(ts);
        }
    }

private:
    struct Shard {
        alignas(64) std::atomic<Pass*> open{nullptr};  // read by every submit
        // takeable(): the open pass's slot count when last looked at (under mu_; its own line)
        alignas(64) const Pass* seen_pass = nullptr;
        std::uint64_t seen_n = 0;
        double seen_us = 0;
    };
    // what a worker thread keeps between passes
    struct Device {
        bool ok = false;
        hipStream_t stream = nullptr;
        hipEvent_t ev = nullptr;
        double kern_ema_us = 0;          // this worker's recent device-pass kernel time
        std::uint8_t* dstage = nullptr;  // device copy of a pass's input side (staged passes)
    };

    void fill_slot(Pass& p, std::uint32_t idx, std::uint64_t at, const std::uint8_t key[32],
                   const std::uint8_t nonce[12], std::span<const std::uint8_t> in, FrameTicket::State* ts) {
        SlotRec& r = p.recs[idx];  // this slot's own cache lines
        const std::uint64_t gen = p.gen.load(std::memory_order_relaxed);  // stable: the pass cannot run before this slot is filled
        r.in_at = at;
        r.len = in.size();
        r.ticket = ts;
        std::memcpy(r.key, key, 32);
        if (!open_dir_) std::memcpy(r.nonce, nonce, 12);
        if (!in.empty()) enet::hb::copy_streaming(p.h + p.o_in + at, in.data(), in.size());
        _mm_sfence();  // the streamed lines are visible before the fill word says so
        ts->pass = &p;
        ts->idx = idx;
        ts->gen = gen;
        r.tk.store(gen << 3 | kPending, std::memory_order_relaxed);
        r.fill.store(gen << 2 | kFilled, std::memory_order_release);
    }

    // passes: queue_core.cpp
    std::unique_ptr<Pass> make_pass();
    static bool released(Pass& p);
    std::uint64_t evict(Pass& p, bool* complete = nullptr);
    void reopen(Shard& sh, Pass& p);
    bool install(Shard& sh, Pass* p);
    void open_pass(Shard& sh);
    static bool close_pass(Pass& p);
    void close_full(Pass* p, std::uint64_t gen);
    // workers
    void start_workers();
    bool takeable(Shard& sh, const Pass& p);
    void work();
    std::uint64_t gather_slots(Pass& p);
    void host_run(Pass& p);
    void run_on_device(Pass& p, Device& dev, std::uint64_t max_len);
    bool run_pass(Pass& p, Device* dev = nullptr);

    FrameQueueOptions opt_;
    bool open_dir_;
    bool has_device_ = false;
    std::size_t max_passes_ = 24;
    std::uint64_t target_frames_ = 1024, target_bytes_ = 2u << 20;
    std::mutex mu_;
    std::condition_variable work_cv_, free_cv_;
    const ShardPlan plan_;
    Shard shards_[kMaxShards];
    std::vector<std::unique_ptr<Pass>> passes_;
    std::deque<Pass*> closed_, done_;
    std::size_t inflight_ = 0;
    std::size_t allocating_ = 0;  // passes being allocated (outside mu_)
    bool watching_ = false;       // a worker polls the open passes' arrivals
    bool stop_ = false;
    std::vector<std::thread> workers_;
    FrameQueueStats st_{};
    std::atomic<std::uint64_t> direct_{0};
    std::atomic<std::uint64_t> overflows_{0};  // reservations that found their pass full
    double dev_passes_ = 0, sum_pass_us_ = 0, sum_kernel_us_ = 0, sum_fill_us_ = 0;
};

}  // namespace enet::fq
