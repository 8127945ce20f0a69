// queue_slots.hpp -- the lock-free half of the frame queues: the words a submitting thread, a
// ticket and the queue's workers share about one slot of a pass, the pass and its memory layout,
// the per-thread ticket-state cache and the counters of AUTO's routing.  Everything a thread does
// once per frame is inline here (0.38-0.48 us of CPU per frame).
//
// WHO MAY WRITE WHAT.  g = the pass's generation when the slot was reserved; a word of an older
// generation reads as "empty" to everyone, so a reused slot can never be acted on by a ticket or
// an evictor of an earlier frame.
//
//   SlotRec::fill = g << 2 | ...      (submitter -> worker)
//     empty -> kFilled      the submitter that reserved the slot, after its copy (release; the
//                           streamed lines fenced first)
//     empty -> kOverflow    the first reservation past the pass's capacity (a slot index below
//                           capacity): marks the cut.  The worker reads fill in gather_slots().
//
//   SlotRec::tk = g << 3 | ...        (ticket <-> queue)
//     empty     -> kPending   the submitter, in fill_slot, before `fill` publishes the slot
//     kPending  -> kClaimed   the ticket (get, get(out), ready): CAS.  It reads the pass, then
//     kClaimed  -> kReleased    get / get(out): the result is copied out
//     kClaimed  -> kPending     ready(): only looked
//     kPending  -> kViewing   the ticket (view): CAS.  The pass cannot be reused or evicted until
//     kViewing  -> kReleased    release(), get() or the ticket's end
//     kPending  -> kReleased  the ticket, dropped uncollected: CAS
//     kPending  -> kEvicting  the queue (Core::evict, from open_pass or ~Core): CAS.  It copies the
//                             result into the ticket's State, stores State::st = kHasResult, then
//     kEvicting -> kEvicted
//   kReleased and kEvicted are final for the generation.  An evictor that finds kClaimed waits (a
//   read in progress ends in kPending or kReleased); one that finds kViewing leaves the slot and
//   reports the pass incomplete.  A ticket whose CAS from kPending fails is being or has been
//   evicted: it waits for State::st == kHasResult and reads its State.
//
//   FrameTicket::State::st    kInPass: the submitter, before the slot is published; kHasResult: a
//     ticket born with its result, the evictor (release store, its last access to the State), or
//     free_state.  Only the ticket frees its State, and never between kEvicting and kHasResult.
//
//   Pass::res = closed | slots << 40 | input bytes.  Submitters fetch_add their reservation;
//     close_pass sets the closed bit once (a worker under the queue's mu_, close_full under mu_ for
//     the generation its reservation was made in, ~Core); reopen() (under mu_) bumps Pass::gen and
//     then stores 0.
//   Pass::state   kOpen (reopen) -> kClosed (close_pass) -> kDone (the worker, when the results are
//     in the pass; under Pass::mu for the waiters' condition variable).
#pragma once

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <memory>
#include <mutex>
#include <optional>
#include <span>
#include <thread>
#include <vector>

#include <immintrin.h>

#include "ephemeralnet/crypto/Batch.hpp"
#include "wire_host.hpp"

namespace enet::fq {

struct Pass;

enum : std::uint64_t {  // SlotRec::tk
    kPending = 1,   // in the pass, not collected
    kClaimed = 2,   // its ticket is reading the pass (get / ready)
    kReleased = 3,  // collected or dropped: the pass may be reused
    kEvicting = 4,  // the queue is copying the result into the ticket's State
    kEvicted = 5,   // ... done: the pass may be reused
    kViewing = 6,   // its ticket holds a zero-copy view of the result (FrameTicket::view)
};
enum : std::uint64_t { kFilled = 1, kOverflow = 2 };  // SlotRec::fill
enum : int { kInPass = 0, kHasResult = 1 };           // FrameTicket::State::st
enum : int { kOpen = 0, kClosed = 1, kDone = 2 };     // Pass::state
constexpr std::uint64_t kClosedBit = 1ull << 63;
constexpr int kSlotShift = 40;  // res = closed | slots << 40 | input bytes used (< 2^40)
constexpr std::uint64_t kBytesMask = (1ull << kSlotShift) - 1;
constexpr std::uint64_t kSlotMask = (1ull << 23) - 1;

}  // namespace enet::fq

namespace ephemeralnet::crypto::batch {

// A ticket's state: owned, allocated and freed by the ticket (the submitting thread, normally),
// never by the queue.
struct FrameTicket::State {
    std::atomic<int> st{enet::fq::kHasResult};
    enet::fq::Pass* pass = nullptr;
    std::uint32_t idx = 0;
    std::uint64_t gen = 0;
    bool viewing = false;  // the slot is kViewing: this ticket holds a view into the pass
    // AUTO's routing signals this ticket is counted in until it is collected or dropped (on
    // whatever thread): its submitting thread's backlog, and its shard of the process-wide count
    std::shared_ptr<std::atomic<std::int32_t>> backlog;
    std::atomic<std::int64_t>* inflight = nullptr;
    std::optional<std::vector<std::uint8_t>> result;
};

}  // namespace ephemeralnet::crypto::batch

namespace enet::fq {

using ephemeralnet::crypto::batch::FrameTicket;
using Bytes = std::span<const std::uint8_t>;

struct alignas(128) SlotRec {
    std::atomic<std::uint64_t> fill{0};  // gen << 2 | kFilled / kOverflow
    std::atomic<std::uint64_t> tk{0};    // gen << 3 | kPending .. kViewing
    std::uint64_t in_at = 0;             // input offset in the pass arena
    std::uint64_t len = 0;               // input bytes
    FrameTicket::State* ticket = nullptr;
    std::uint8_t key[32];
    std::uint8_t nonce[12];
};

// the slot's fill state in generation gen, once its submitter has written it
inline std::uint64_t spin_until(const std::atomic<std::uint64_t>& f, std::uint64_t gen) {
    for (int i = 0;; ++i) {
        const std::uint64_t v = f.load(std::memory_order_acquire);
        if ((v >> 2) == gen) return v & 3;
        if (i < 1024) _mm_pause();
        else std::this_thread::yield();  // its submitter was preempted mid-copy
    }
}

// One device pass: a block of (pinned, device-mapped) memory laid out as a wire-frame batch.
struct Pass {
    bool open_dir = false;      // FrameReceiveQueue (frames in, messages out)
    std::uint8_t* h = nullptr;  // host view of the block
    std::uint8_t* d = nullptr;  // device view (nullptr: plain heap memory, host engine only)
    bool pinned = false;        // h from topo::alloc_pinned
    std::size_t bytes = 0;
    std::uint32_t cap_frames = 0;
    std::uint64_t cap_in = 0;
    std::uint64_t o_inoff = 0, o_outoff = 0, o_keys = 0, o_nonces = 0, o_ok = 0, o_macs = 0, o_in = 0, o_out = 0;
    // The layout for F frames and cap_in input bytes (sets the o_* offsets, the capacities and
    // `bytes`; the caller allocates h).  The input side -- offsets, keys, nonces, input arena -- is
    // one contiguous prefix, [0, o_in + input bytes): what a staged pass copies to the device.
    void lay_out(std::uint32_t F, std::uint64_t in_bytes) {
        std::uint64_t at = 0;
        auto take = [&](std::uint64_t& where, std::uint64_t b) {
            where = at;
            at = (at + b + 255) & ~std::uint64_t(255);
        };
        take(o_inoff, 8ull * (F + 1));
        take(o_outoff, 8ull * (F + 1));
        take(o_keys, 32ull * F);
        take(o_nonces, 12ull * F);
        take(o_ok, F);
        take(o_macs, 32ull * F);
        take(o_in, in_bytes);
        take(o_out, in_bytes + kWire * (std::uint64_t)F);
        bytes = at;
        cap_frames = F;
        cap_in = in_bytes;
    }
    // [cap_frames] what each submitter writes about its slot, one 128-byte record per slot: the
    // offsets / keys / nonces arrays the kernel reads pack 2-10 slots per cache line, and filling
    // them from the submitting threads shared every such line between neighbouring slots; the
    // worker packs them from these records when the pass runs
    std::unique_ptr<SlotRec[]> recs;
    alignas(64) std::atomic<std::uint64_t> res{kClosedBit};
    alignas(64) std::atomic<std::int64_t> first_us{0};
    std::atomic<int> state{kDone};
    // generation: +1 each time the pass is reopened (under the queue's mu_; read without it by a
    // submitter, before its reservation, to tie a later close_full to that generation)
    std::atomic<std::uint64_t> gen{0};
    std::uint32_t reserved = 0;  // reservations made before the close (some may be overflows)
    std::uint32_t n = 0;         // final slot count (set when the pass runs)
    std::uint32_t rel_scan = 0;  // released(): slots [0, rel_scan) are known released (under mu_)
    std::uint64_t in_used = 0;   // final input bytes
    double closed_at = 0;
    std::mutex mu;
    std::condition_variable cv;  // waiters for kDone

    std::uint64_t* in_off() const { return reinterpret_cast<std::uint64_t*>(h + o_inoff); }
    std::uint64_t* out_off() const { return reinterpret_cast<std::uint64_t*>(h + o_outoff); }
    // output bytes of a frame with `in` input bytes, and the output offset of slot idx
    std::uint64_t out_len(std::uint64_t in) const { return open_dir ? in - kWire : in + kWire; }
    std::uint64_t out_at(std::uint64_t in_at, std::uint32_t idx) const {
        return open_dir ? in_at - kWire * idx : in_at + kWire * idx;
    }
    void wait_done() {
        for (int i = 0; i < 64; ++i) {  // a pass takes ~100 us: only a short spin, then sleep
            if (state.load(std::memory_order_acquire) == kDone) return;
            _mm_pause();
        }
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return state.load(std::memory_order_acquire) == kDone; });
    }
    // the slot's result where it lies (pass done); nullopt: the frame did not open
    std::optional<Bytes> result(std::uint32_t i) const {
        const std::uint64_t a = in_off()[i], b = in_off()[i + 1];
        if (open_dir && h[o_ok + i] != 1) return std::nullopt;
        return Bytes(h + o_out + out_at(a, i), out_len(b - a));
    }
    ~Pass();
};

// a result as its own vector, and into a caller's vector (cleared when there is none)
inline std::optional<std::vector<std::uint8_t>> to_vector(std::optional<Bytes> r) {
    if (!r) return std::nullopt;
    return std::vector<std::uint8_t>(r->data(), r->data() + r->size());
}
inline bool assign_to(std::optional<Bytes> r, std::vector<std::uint8_t>& out) {
    if (r) out.assign(r->data(), r->data() + r->size());
    else out.clear();
    return r.has_value();
}

// Ticket states come from a per-thread cache: the ticket that frees a state is normally on the
// thread that allocated it (the submitter collects its own frames), so a state goes back to the
// cache it came from; a malloc / free pair per frame measured ~100 ns on the box (r05g profile).
inline thread_local int t_cache_state = 0;  // 0 untouched, 1 live, 2 destroyed (trivially destructible)
struct StateCache {
    std::vector<FrameTicket::State*> v;
    ~StateCache() {
        t_cache_state = 2;
        for (auto* x : v) delete x;
        v.clear();
    }
};
// (function-local: a namespace-scope inline thread_local with a destructor is reached through an
// out-of-line init call on every access)
inline StateCache& state_cache() {
    thread_local StateCache c;
    return c;
}

// The AUTO policy's signals (use_queue_async), counted for every non-blocking submission whatever
// its route and uncounted when its ticket is collected or dropped, on any thread:
//  * the submitting thread's backlog -- a counter the thread shares with its tickets, so a ticket
//    collected by another thread (a reader thread submits, a writer thread collects) or after the
//    submitter exited decrements the right one (a thread-local count only grew on the
//    submitting side of such a split, sending trickle loads to the device);
//  * the process-wide count per direction (many session threads, each with a
//    few frames in flight), sharded over cache lines by thread so submitters do not share one.
struct ThreadBacklog {
    std::shared_ptr<std::atomic<std::int32_t>> c = std::make_shared<std::atomic<std::int32_t>>(0);
};
inline ThreadBacklog& thread_backlog() {
    thread_local ThreadBacklog b;
    return b;
}
struct alignas(64) PaddedCount {
    std::atomic<std::int64_t> v{0};
};
constexpr unsigned kCountShards = 16;
inline PaddedCount g_inflight[2][kCountShards];
inline std::atomic<unsigned> g_next_count_shard{0};
inline std::atomic<std::int64_t>* inflight_slot(bool open_dir) {
    thread_local const unsigned sh = g_next_count_shard.fetch_add(1, std::memory_order_relaxed) % kCountShards;
    return &g_inflight[open_dir ? 1 : 0][sh].v;
}
inline void count_submission(FrameTicket::State* s, bool open_dir) {
    s->backlog = thread_backlog().c;
    s->backlog->fetch_add(1, std::memory_order_relaxed);
    s->inflight = inflight_slot(open_dir);
    s->inflight->fetch_add(1, std::memory_order_relaxed);
}

inline FrameTicket::State* new_state() {
    if (t_cache_state == 0) {
        state_cache().v.reserve(1024);
        t_cache_state = 1;
    }
    if (t_cache_state != 1 || state_cache().v.empty()) return new FrameTicket::State();
    FrameTicket::State* x = state_cache().v.back();
    state_cache().v.pop_back();
    return x;
}
inline void free_state(FrameTicket::State* x) {
    if (x->backlog) {
        x->backlog->fetch_sub(1, std::memory_order_relaxed);
        x->backlog.reset();
    }
    if (x->inflight) {
        x->inflight->fetch_sub(1, std::memory_order_relaxed);
        x->inflight = nullptr;
    }
    x->result.reset();
    x->viewing = false;
    x->st.store(kHasResult, std::memory_order_relaxed);
    if (t_cache_state == 1 && state_cache().v.size() < 8192) state_cache().v.push_back(x);
    else delete x;
}

// The ticket word of a ticket's slot
inline std::atomic<std::uint64_t>& tk_of(const FrameTicket::State* s) { return s->pass->recs[s->idx].tk; }

// Take a pending slot for its ticket (kPending -> `to`: kClaimed to read it, kViewing to keep a
// view, kReleased to drop it); false once it is being or has been evicted
inline bool claim(FrameTicket::State* s, std::uint64_t to = kClaimed) {
    std::uint64_t e = s->gen << 3 | kPending;
    return tk_of(s).compare_exchange_strong(e, s->gen << 3 | to, std::memory_order_acq_rel);
}
inline void set_tk(FrameTicket::State* s, std::uint64_t st) {
    tk_of(s).store(s->gen << 3 | st, std::memory_order_release);
}
// an evicted ticket's result is in its State once st says so
inline void await_evicted(const FrameTicket::State* s) {
    while (s->st.load(std::memory_order_acquire) != kHasResult) _mm_pause();
}
// Does the ticket read its result from the pass (it holds the slot: claimed now, or under its own
// view)?  false: the result is in the State (a ready ticket, or evicted -- awaited here)
inline bool hold(FrameTicket::State* s) {
    if (s->viewing) return true;
    if (s->st.load(std::memory_order_acquire) != kHasResult && claim(s)) return true;
    await_evicted(s);
    return false;
}

}  // namespace enet::fq
