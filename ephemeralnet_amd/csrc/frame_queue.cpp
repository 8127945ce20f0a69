// frame_queue.cpp -- the cross-session frame queues of Batch.hpp: FrameTicket,
// FrameQueue, FrameReceiveQueue and the AUTO routing rule.
//
// Reference: SessionManager::send (src/network/SessionManager.cpp:337-388), receive_loop
// (:703-854) and protocol::encode_signed / decode_signed (src/protocol/Message.cpp:305-328): one
// frame per call on the session's own thread.
//
// Design (round 5).  A queue direction owns a few PASSES: blocks of pinned, device-mapped host
// memory laid out as one wire-frame batch (offsets, keys, nonces, ok / MAC arrays, input arena,
// output arena).  A submitting thread
//   1. reserves the next slot of its shard's open pass with ONE atomic add on a packed word
//      (closed bit | slot count | input bytes used) -- the output offset follows from the slot
//      index (frames are +48 / -48 bytes), so nothing else is shared;
//   2. copies its message / frame into the pass arena and its key, nonce, offset and length
//      into the slot's own 128-byte record (no cache line shared with a neighbouring slot), then
//      sets the record's state;
//   3. gets a FrameTicket (a small heap State shared with the pass).
// A worker thread takes an open pass once it reaches a quarter of the size limits, when no frame
// has arrived for 30 us, or 250 us after its first frame; closes it (the same word: no slot can be
// reserved after), waits for the slots' states, packs the records into the offsets / keys /
// nonces arrays, and runs enet_wire_seal_batch / _open_batch on the pass in place (its own HIP
// stream; the kernel reads a small pass over PCIe, a large one from a device copy of its input
// side, and writes the results into the pass).  Each ticket copies its own result out of the pass on its
// owner's thread.  A pass is reused once every ticket of it has collected or dropped its result;
// when every pass is referenced, the oldest finished one is evicted (its uncollected results
// copied into their tickets).  Round 4's queue built every pass in its worker (a gather of every
// request through the batch runtime's pool, a scatter into per-request vectors, a promise per
// frame): ~300 us and ~100 frames per pass at 4 096 frames in flight, 1.29 M frames/s sealed.
//
// Where things live: queue_slots.hpp the slot / ticket words, the pass and its layout, the state
// cache and AUTO's counters; queue_core.hpp / .cpp one direction's submit path, pass recycling and
// workers; wire_host.hpp one frame on the host engine and the nonce generator; queue_knobs.hpp the
// tools build's hooks; host_topo.cpp the CPU -> L3 map behind the shards.
#include <algorithm>
#include <array>
#include <future>

#include "enet_crypto.h"
#include "queue_core.hpp"
#include "scalar.hpp"

namespace ephemeralnet::crypto::batch {

using namespace enet::fq;

namespace {

// a ticket whose result is known on the caller's thread (counted like a queued one: AUTO's signals
// see every non-blocking submission, whichever route served it)
FrameTicket ready_ticket(std::optional<std::vector<std::uint8_t>> r, bool open_dir, bool counted = true) {
    auto* s = new_state();
    s->result = std::move(r);
    if (counted) count_submission(s, open_dir);
    return FrameTicket(s);
}

// Non-blocking submissions: the queue under DEVICE; under AUTO when the device is there and either
//  * the submitting thread holds >= 320 uncollected frames -- where the device queue overtakes the
//    host engine in frames/s for a few deep submitters (box, 1 500-byte frames, 16 threads, sealed /
//    opened M frames/s device vs the stitched host engine: x 256 in flight 10.9-11.0 / 11.7-11.8 vs
//    13.2-13.3 / 11.9-12.6, x 384 12.6-12.8 / 13.0 vs 13.2 / 11.9-12.8, x 512 13.4-14.0 / 13.5-13.7
//    vs 11.9-13.1 / 12.8; profiles/r05_seal_crossover_hi.jsonl; below ~64 per thread the device is
//    5-100x slower, profiles/r05s_crossover.jsonl), or
//  * the process holds >= 320 uncollected frames per CPU of its budget in this direction -- many
//    session threads with a few frames each: the host engine's rate is bounded by the CPUs
//    (~0.8 M frames/s each), the device queue's by the frames in flight (profiles/
//    r06_sessions_async.jsonl).
// Blocking seal() / open() never take the queue under AUTO: one frame per blocked session thread
// costs a thread wake-up per frame (7-11 us of CPU), and 64-768 blocked threads moved 0.2-2.2 M
// frames/s through the device queue against 7-10 M on the host engine
// (profiles/r06_sessions_blocking.jsonl).  The device costs a third of the CPU per frame once it
// is fed (0.35-0.44 vs 1.2-1.35 us): ENET_SCALAR_DEVICE is the choice for a relay whose cores have
// other work.
std::int64_t cpu_budget() {
    static const std::int64_t v = [] {
        std::int64_t b = (std::int64_t)enet::topo::allowed_cpus().size();
        if (const std::uint32_t q = enet::topo::cgroup_quota_cpus()) b = std::min<std::int64_t>(b, q);
        if (const std::uint32_t e = enet::topo::env_cpus()) b = std::min<std::int64_t>(b, e);
        return std::max<std::int64_t>(1, b);
    }();
    return v;
}
// the process-wide count of one direction, re-summed every 16th call on a thread (the shards sit on
// lines other threads write; one sum is 16 cache-line reads)
std::int64_t inflight_estimate(bool open_dir) {
    thread_local std::int64_t cached[2] = {0, 0};
    thread_local std::uint32_t calls[2] = {0, 0};
    const int d = open_dir ? 1 : 0;
    if ((calls[d]++ & 15u) == 0) {
        std::int64_t sum = 0;
        for (auto& c : g_inflight[d]) sum += c.v.load(std::memory_order_relaxed);
        cached[d] = sum;
    }
    return cached[d];
}
bool use_queue_async(const Core& c, bool open_dir) {
    const int pol = enet::scalar::g_policy.load();
    if (pol == ENET_SCALAR_DEVICE) return true;
    if (pol != ENET_SCALAR_AUTO || !c.has_device()) return false;
    static const std::int32_t backlog = auto_backlog_override(320);
    return thread_backlog().c->load(std::memory_order_relaxed) >= backlog ||
           inflight_estimate(open_dir) >= (std::int64_t)backlog * cpu_budget();
}

// One frame on the calling thread's host engine (policies auto and host): a blocked session thread
// seals its own frame -- one MTU frame costs a core ~1 us, while a device pass cannot return
// before one lane's serial HMAC over the frame (~70 us), and blocked callers bring one frame each
std::optional<std::vector<std::uint8_t>> seal_now(Core& c, const std::uint8_t key[32], std::span<const std::uint8_t> m) {
    std::uint8_t nonce[12];
    nonce_source().draw(nonce);
    enet::scalar::host_call();
    c.count_direct();
    return host_wire_seal(key, nonce, m);
}
std::optional<std::vector<std::uint8_t>> open_now(Core& c, const std::uint8_t key[32], std::span<const std::uint8_t> f) {
    enet::scalar::host_call();
    c.count_direct();
    std::optional<std::vector<std::uint8_t>> m(std::in_place, f.size() - kWire);
    if (!host_wire_open_into(key, f, m->data())) m.reset();
    return m;
}

// The collect sequence of get() and get(out), first half: wait for the ticket's result and expose
// it where it lies -- in its pass (in_pass; the slot claimed while the caller copies) or in the
// ticket's State (a ticket born ready, or evicted: awaited).  view() keeps its own short body: it
// takes the slot as kViewing, keeps it, and is not profiled.
std::optional<Bytes> expose(FrameTicket::State* s, bool& in_pass, std::uint64_t& pt) {
    in_pass = hold(s);
    if (in_pass) {
        prof_add(kGetClaim, pt);
        if (s->pass->state.load(std::memory_order_acquire) != kDone) {
            s->pass->wait_done();
            prof_add(kGetWait, pt);
        }
        return s->pass->result(s->idx);
    }
    if (!s->result) return std::nullopt;
    return Bytes(*s->result);
}
// ... second half: the slot released (the pass may be reused), the state freed, the ticket empty
void finish(FrameTicket::State*& s, bool in_pass, std::uint64_t& pt) {
    if (in_pass) {
        prof_add(kGetCopy, pt);
        set_tk(s, kReleased);
        prof_add(kGetReleaseStore, pt);
    }
    free_state(s);
    prof_add(kGetRelease, pt);
    s = nullptr;
}

}  // namespace

// ------------------------------------------------------------------------------ FrameTicket
FrameTicket& FrameTicket::operator=(FrameTicket&& o) noexcept {
    if (this != &o) {
        release();
        s_ = o.s_;
        o.s_ = nullptr;
    }
    return *this;
}

FrameTicket::~FrameTicket() { release(); }

// drops the ticket's claim on its slot (or view), frees its state; the ticket is empty after
void FrameTicket::release() noexcept {
    if (!s_) return;
    if (s_->viewing) set_tk(s_, kReleased);
    else if (s_->st.load(std::memory_order_acquire) != kHasResult && !claim(s_, kReleased))
        await_evicted(s_);  // the queue is evicting it into s_
    free_state(s_);
    s_ = nullptr;
}

bool FrameTicket::ready() const noexcept {
    if (!s_) return false;
    if (s_->viewing || s_->st.load(std::memory_order_acquire) == kHasResult) return true;
    if (!claim(s_)) return s_->st.load(std::memory_order_acquire) == kHasResult;
    const bool r = s_->pass->state.load(std::memory_order_acquire) == kDone;
    set_tk(s_, kPending);
    return r;
}

std::optional<std::vector<std::uint8_t>> FrameTicket::get() {
    if (!s_) return std::nullopt;
    bool in_pass;
    std::uint64_t pt = prof_t();
    const auto bytes = expose(s_, in_pass, pt);
    auto r = in_pass ? to_vector(bytes) : std::move(s_->result);  // its own vector: moved, not copied
    finish(s_, in_pass, pt);
    return r;
}

bool FrameTicket::get(std::vector<std::uint8_t>& out) {
    if (!s_) {
        out.clear();
        return false;
    }
    bool in_pass;
    std::uint64_t pt = prof_t();
    const bool ok = assign_to(expose(s_, in_pass, pt), out);
    finish(s_, in_pass, pt);
    return ok;
}

bool FrameTicket::view(std::span<const std::uint8_t>& out) {
    out = {};
    if (!s_) return false;
    if (!s_->viewing && s_->st.load(std::memory_order_acquire) != kHasResult) {
        if (claim(s_, kViewing)) {
            s_->viewing = true;
            if (s_->pass->state.load(std::memory_order_acquire) != kDone) s_->pass->wait_done();
        } else {
            await_evicted(s_);
        }
    }
    const auto bytes = s_->viewing ? s_->pass->result(s_->idx)
                       : s_->result ? std::optional<Bytes>(Bytes(*s_->result)) : std::nullopt;
    if (bytes) out = *bytes;
    return bytes.has_value();
}

// ------------------------------------------------------------------------------ send
struct FrameQueue::Impl {
    explicit Impl(const FrameQueueOptions& o) : core(o, false) {}
    Core core;
    // push / flush
    mutable std::mutex manual_mu;
    std::vector<std::array<std::uint8_t, 32>> keys;
    std::vector<std::vector<std::uint8_t>> messages;
};

FrameQueue::FrameQueue() : FrameQueue(FrameQueueOptions{}) {}
FrameQueue::FrameQueue(FrameQueueOptions options) : impl_(new Impl(options)) {}
FrameQueue::~FrameQueue() { delete impl_; }

std::optional<std::vector<std::uint8_t>> FrameQueue::seal(const std::array<std::uint8_t, 32>& session_key,
                                                          std::span<const std::uint8_t> message) {
    if (message.size() + kMac > kMaxPayloadSize) return std::nullopt;  // SessionManager.cpp:358-360
    if (enet::scalar::g_policy.load() != ENET_SCALAR_DEVICE) return seal_now(impl_->core, session_key.data(), message);
    return impl_->core.submit(session_key.data(), message).get();
}

FrameTicket FrameQueue::submit(const std::array<std::uint8_t, 32>& session_key, std::span<const std::uint8_t> message) {
    if (message.size() + kMac > kMaxPayloadSize) return ready_ticket(std::nullopt, false, false);
    if (!use_queue_async(impl_->core, false)) return ready_ticket(seal_now(impl_->core, session_key.data(), message), false);
    return impl_->core.submit(session_key.data(), message);
}

std::future<std::optional<std::vector<std::uint8_t>>> FrameQueue::seal_async(
    const std::array<std::uint8_t, 32>& session_key, std::vector<std::uint8_t> message) {
    auto t = submit(session_key, message);  // the message is in the pass already
    return std::async(std::launch::deferred, [t = std::move(t)]() mutable { return t.get(); });
}

bool FrameQueue::push(const std::array<std::uint8_t, 32>& session_key, std::span<const std::uint8_t> message) {
    if (message.size() + kMac > kMaxPayloadSize) return false;
    std::lock_guard<std::mutex> lk(impl_->manual_mu);
    impl_->keys.push_back(session_key);
    impl_->messages.emplace_back(message.begin(), message.end());
    return true;
}

std::size_t FrameQueue::size() const {
    std::lock_guard<std::mutex> lk(impl_->manual_mu);
    return impl_->messages.size();
}

std::vector<std::vector<std::uint8_t>> FrameQueue::flush() {
    std::vector<std::array<std::uint8_t, 32>> keys;
    std::vector<std::vector<std::uint8_t>> messages;
    {
        std::lock_guard<std::mutex> lk(impl_->manual_mu);
        keys.swap(impl_->keys);
        messages.swap(impl_->messages);
    }
    const std::size_t n = messages.size();
    std::vector<std::vector<std::uint8_t>> frames;
    if (n == 0) return frames;
    std::vector<Nonce> nonces(n);
    for (auto& x : nonces) nonce_source().draw(x.bytes.data());
    std::vector<std::span<const std::uint8_t>> ms(messages.begin(), messages.end());
    // one batch call (the host-memory runtime, crypto::batch::wire_seal); a failed device call is
    // finished on the host engine
    if (enet::scalar::g_policy.load() != ENET_SCALAR_HOST &&
        enet::scalar::try_device("FrameQueue::flush", [&] { frames = wire_seal(keys, nonces, ms); }))
        return frames;
    enet::scalar::host_call();
    frames.assign(n, {});
    for (std::size_t i = 0; i < n; ++i) frames[i] = host_wire_seal(keys[i].data(), nonces[i].bytes.data(), ms[i]);
    return frames;
}

FrameQueueStats FrameQueue::stats() const { return impl_->core.stats(); }

// ------------------------------------------------------------------------------ receive
struct FrameReceiveQueue::Impl {
    explicit Impl(const FrameQueueOptions& o) : core(o, true) {}
    Core core;
};

FrameReceiveQueue::FrameReceiveQueue() : FrameReceiveQueue(FrameQueueOptions{}) {}
FrameReceiveQueue::FrameReceiveQueue(FrameQueueOptions options) : impl_(new Impl(options)) {}
FrameReceiveQueue::~FrameReceiveQueue() { delete impl_; }

std::optional<std::vector<std::uint8_t>> FrameReceiveQueue::open(const std::array<std::uint8_t, 32>& session_key,
                                                                 std::span<const std::uint8_t> frame) {
    if (!frame_shape_ok(frame)) return std::nullopt;  // never reaches a pass
    if (enet::scalar::g_policy.load() != ENET_SCALAR_DEVICE) return open_now(impl_->core, session_key.data(), frame);
    return impl_->core.submit(session_key.data(), frame).get();
}

FrameTicket FrameReceiveQueue::submit(const std::array<std::uint8_t, 32>& session_key,
                                      std::span<const std::uint8_t> frame) {
    if (!frame_shape_ok(frame)) return ready_ticket(std::nullopt, true, false);
    if (!use_queue_async(impl_->core, true)) return ready_ticket(open_now(impl_->core, session_key.data(), frame), true);
    return impl_->core.submit(session_key.data(), frame);
}

std::future<std::optional<std::vector<std::uint8_t>>> FrameReceiveQueue::open_async(
    const std::array<std::uint8_t, 32>& session_key, std::vector<std::uint8_t> frame) {
    auto t = submit(session_key, frame);
    return std::async(std::launch::deferred, [t = std::move(t)]() mutable { return t.get(); });
}

FrameQueueStats FrameReceiveQueue::stats() const { return impl_->core.stats(); }

}  // namespace ephemeralnet::crypto::batch
