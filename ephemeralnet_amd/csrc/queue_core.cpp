// queue_core.cpp -- the cold half of a frame queue direction (queue_core.hpp): allocating,
// recycling and evicting passes, closing them, and the worker threads that run them on the device
// or the host engine.
#include "queue_core.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <stdexcept>
#include <system_error>

#include <sys/prctl.h>
#include <time.h>

#include "enet_crypto.h"
#include "scalar.hpp"
#include "staging.hpp"

namespace enet::fq {

namespace {

double thread_cpu_s() {
    timespec ts{};
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

// A large device pass is staged: its input side goes to device memory by one SDMA copy and the
// kernel reads HBM; smaller passes run zero-copy (the kernel reads the pinned pass over PCIe).  A
// sealing pass pays for the copy from ~640 frames, an opening pass from ~512 (tools/stage_ab.sh,
// profiles/r05_queue_stage_ab.jsonl, r05_queue_stage_ab_w8.jsonl; the table is in DESIGN_HISTORY 10).
bool stage_pass(std::uint32_t n, bool open_dir) {
    if (stage_override() >= 0) return stage_override() != 0;
    return n >= (open_dir ? 512u : 640u);
}

// a failed HIP call of a pass: the sticky error cleared, then the shared check's exception
void hip_ok(hipError_t e, const char* what) {
    if (e != hipSuccess) (void)hipGetLastError();
    enet::stage::hip_check(e, what);
}

bool is_open(const Pass* p) { return p && !(p->res.load(std::memory_order_acquire) & kClosedBit); }

}  // namespace

Pass::~Pass() {
    if (pinned) enet::topo::free_pinned(h);
    else delete[] h;
}

Core::Core(const FrameQueueOptions& o, bool open_dir) : opt_(o), open_dir_(open_dir) {
    opt_.max_frames = std::min<std::size_t>(std::max<std::size_t>(1, opt_.max_frames), 1u << 20);
    opt_.max_bytes = std::max<std::size_t>(opt_.max_bytes, 4096);
    opt_.max_inflight = std::min<std::size_t>(std::max<std::size_t>(1, opt_.max_inflight), 16);
    // passes: in flight + one open per shard + those still referenced by uncollected tickets
    // (up to ~28 at 16 threads x 256 in flight with a slow consumer); allocated on demand, each
    // sized to the close target below: small passes waste less of the pinned memory they hold
    max_passes_ = 8 * opt_.max_inflight + 2 * plan_.n;
    int count = 0;
    has_device_ = hipGetDeviceCount(&count) == hipSuccess && opt_.device >= 0 && opt_.device < count;
    if (!has_device_) (void)hipGetLastError();
    if (fake_us() > 0) has_device_ = true;
    const bool delay = opt_.max_delay.count() > 0;
    target_frames_ = std::max<std::size_t>(1, delay ? opt_.max_frames : opt_.max_frames / 4);
    target_bytes_ = delay ? opt_.max_bytes : std::max<std::size_t>(opt_.max_bytes / 4, 4096);
}

Core::~Core() {
    {
        std::lock_guard<std::mutex> lk(mu_);
        stop_ = true;
    }
    work_cv_.notify_all();
    for (auto& w : workers_)
        if (w.joinable()) w.join();
    // the workers ran every closed pass and every non-empty open one; a slot reserved while
    // the queue was being destroyed is finished here (on the host engine)
    for (auto& p : passes_) {
        if (p->state.load() != kDone && close_pass(*p)) {
            if (p->reserved) run_pass(*p);
            else p->state.store(kDone, std::memory_order_release);
        }
        bool complete = true;
        evict(*p, &complete);
        // a ticket still viewing this pass (FrameTicket::view not yet released): leave the
        // pass's memory to it rather than free it under the view
        if (!complete) (void)p.release();
    }
    if (enet::hb::trace_on() && st_.flushes)
        std::fprintf(stderr, "[enet queue] %s: %llu frames in %llu passes (%.1f per pass), %llu host passes, "
                     "%llu evicted, %zu passes allocated; device pass %.1f us = fill wait %.1f + kernel %.1f "
                     "+ queueing\n",
                     open_dir_ ? "open" : "seal", (unsigned long long)st_.frames,
                     (unsigned long long)st_.flushes, (double)st_.frames / (double)st_.flushes,
                     (unsigned long long)st_.host_flushes, (unsigned long long)st_.evicted, passes_.size(),
                     sum_pass_us_ / std::max<double>(1, dev_passes_), sum_fill_us_ / std::max<double>(1, dev_passes_),
                     sum_kernel_us_ / std::max<double>(1, dev_passes_));
}

FrameQueueStats Core::stats() {
    std::lock_guard<std::mutex> lk(mu_);
    FrameQueueStats s = st_;
    const std::uint64_t d = direct_.load(std::memory_order_relaxed);
    s.frames += d;
    s.flushes += d;
    s.host_flushes += d;
    s.pass_us = dev_passes_ ? sum_pass_us_ / dev_passes_ : 0;
    s.kernel_us = dev_passes_ ? sum_kernel_us_ / dev_passes_ : 0;
    s.cas_retries = overflows_.load(std::memory_order_relaxed);
    return s;
}

// ------------------------------------------------------------------------------ passes
// A pass for target_frames_ frames and max(target_bytes_, one maximum frame) input bytes
std::unique_ptr<Pass> Core::make_pass() {
    using ephemeralnet::crypto::batch::FrameQueue;
    auto p = std::make_unique<Pass>();
    p->open_dir = open_dir_;
    p->lay_out((std::uint32_t)target_frames_, std::max<std::uint64_t>(target_bytes_, FrameQueue::kMaxPayloadSize + 256));
    if (has_device_ && fake_us() > 0) {
        p->h = new std::uint8_t[p->bytes];
        p->d = p->h;
    } else if (has_device_) {
        try {
            void* dp = nullptr;
            p->h = static_cast<std::uint8_t*>(
                enet::topo::alloc_pinned(p->bytes, enet::topo::target_node(opt_.device), &dp));
            p->d = static_cast<std::uint8_t*>(dp);
            p->pinned = true;
        } catch (const std::bad_alloc&) {
            throw;
        } catch (const std::exception& e) {
            enet::scalar::device_failed("FrameQueue pass staging", e.what());
            p->h = nullptr;
            p->d = nullptr;
        }
    }
    if (!p->h) p->h = new std::uint8_t[p->bytes];
    p->recs = std::make_unique<SlotRec[]>(p->cap_frames);
    return p;
}

// is a finished pass free (every ticket of it collected or dropped)?  Under mu_.  A release is
// final until the pass is reopened, so the scan resumes where the last one stopped: each slot
// is looked at about once per pass (rescanning from slot 0 on every open_pass held mu_ for
// tens of microseconds with many partly collected passes)
bool Core::released(Pass& p) {
    if (p.state.load(std::memory_order_acquire) != kDone) return false;
    for (; p.rel_scan < p.n; ++p.rel_scan) {
        const std::uint64_t v = p.recs[p.rel_scan].tk.load(std::memory_order_acquire);
        const std::uint64_t g = p.gen.load(std::memory_order_relaxed);
        if (v != (g << 3 | kReleased) && v != (g << 3 | kEvicted)) return false;
    }
    return true;
}

// Copy every uncollected result of a finished pass into its ticket; afterwards no ticket reads
// the pass -- unless one holds a view (kViewing): *complete is then false and the pass must not
// be reused until that ticket releases it
std::uint64_t Core::evict(Pass& p, bool* complete) {
    std::uint64_t moved = 0;
    const std::uint64_t g = p.gen.load(std::memory_order_relaxed) << 3;
    if (complete) *complete = true;
    for (std::uint32_t i = 0; i < p.n; ++i) {
        SlotRec& r = p.recs[i];
        for (;;) {
            std::uint64_t e = g | kPending;
            if (r.tk.compare_exchange_strong(e, g | kEvicting, std::memory_order_acq_rel)) {
                FrameTicket::State* s = r.ticket;
                s->result = to_vector(p.result(i));
                s->st.store(kHasResult, std::memory_order_release);  // the ticket may free s now
                r.tk.store(g | kEvicted, std::memory_order_release);
                ++moved;
                break;
            }
            if (e == (g | kViewing)) {  // held by a view: cannot be moved
                if (complete) *complete = false;
                break;
            }
            if (e != (g | kClaimed)) break;  // collected or dropped
            _mm_pause();                     // a get() / ready() mid-read
        }
    }
    return moved;
}

// Make p the shard's open pass (its old tickets all released or evicted)
// O(1): the new generation retires every slot word of the old one
void Core::reopen(Shard& sh, Pass& p) {
    p.gen.store(p.gen.load(std::memory_order_relaxed) + 1, std::memory_order_release);
    p.n = 0;
    p.rel_scan = 0;
    p.reserved = 0;
    p.in_used = 0;
    p.first_us.store(0, std::memory_order_relaxed);
    p.state.store(kOpen, std::memory_order_relaxed);
    p.res.store(0, std::memory_order_release);
    sh.open.store(&p, std::memory_order_release);
}

// A pass obtained with mu_ let go meanwhile (allocated, evicted) becomes the shard's open pass --
// unless another submitter opened one in that time: then it is kept spare (false).  Wakes the
// submitters waiting for a pass.
bool Core::install(Shard& sh, Pass* p) {
    const bool mine = !is_open(sh.open.load(std::memory_order_acquire));
    if (mine) reopen(sh, *p);
    else done_.push_front(p);
    free_cv_.notify_all();
    return mine;
}

// A new open pass for the shard: a released finished one, a new one, or (all referenced) the
// oldest finished one evicted; waits while every pass is in flight
void Core::open_pass(Shard& sh) {
    std::uint64_t pt = prof_t();
    std::size_t evict_tries = 0;  // finished passes found held by a view this call
    std::unique_lock<std::mutex> lk(mu_);
    prof_add(kOpenLock, pt);
    start_workers();
    for (;;) {
        if (is_open(sh.open.load(std::memory_order_acquire))) {
            prof_add(kOpenRaced, pt);
            return;
        }
        for (auto it = done_.begin(); it != done_.end(); ++it)
            if (released(**it)) {
                Pass* p = *it;
                done_.erase(it);
                reopen(sh, *p);
                prof_add(kOpenReuse, pt);
                return;
            }
        if (passes_.size() + allocating_ < max_passes_) {
            prof_add(kOpenReuse, pt);
            ++allocating_;
            lk.unlock();
            std::unique_ptr<Pass> np;
            try {
                np = make_pass();
            } catch (...) {
                lk.lock();
                --allocating_;
                throw;
            }
            lk.lock();
            --allocating_;
            passes_.push_back(std::move(np));
            if (install(sh, passes_.back().get())) prof_add(kOpenAllocate, pt);
            return;
        }
        if (!done_.empty() && evict_tries < done_.size()) {
            Pass* p = done_.front();
            done_.pop_front();
            lk.unlock();
            bool complete = true;
            const std::uint64_t moved = evict(*p, &complete);
            lk.lock();
            st_.evicted += moved;
            if (!complete) {  // a ticket holds a view into it: try the next one
                done_.push_back(p);
                ++evict_tries;
                continue;
            }
            install(sh, p);
            return;
        }
        if (evict_tries) {  // every finished pass is held by a view: look again shortly
            evict_tries = 0;
            free_cv_.wait_for(lk, std::chrono::microseconds(100));
            continue;
        }
        prof_add(kOpenReuse, pt);
        free_cv_.wait(lk);  // every pass in flight: wait for one to finish
        prof_add(kOpenWait, pt);
    }
}

// Set p's closed bit; true when this call closed it (no reservation succeeds after it)
bool Core::close_pass(Pass& p) {
    const std::uint64_t v = p.res.fetch_or(kClosedBit, std::memory_order_acq_rel);
    if (v & kClosedBit) return false;
    p.reserved = (std::uint32_t)std::min<std::uint64_t>((v >> kSlotShift) & kSlotMask, 0xFFFFFFFFu);
    p.state.store(kClosed, std::memory_order_release);
    p.closed_at = now_us();
    return true;
}

// Close a pass a reservation found full.  Only the generation that reservation was made in:
// a submitter delayed between its reservation and this call may find the pass closed, run,
// released and reopened -- for another shard, too -- and closing that generation would leave
// the new owner's open pointer on a closed pass that no worker takes and no submitter
// reopens.  Once closed, no shard keeps it as its open pass.
void Core::close_full(Pass* p, std::uint64_t gen) {
    std::lock_guard<std::mutex> lk(mu_);  // reopen() runs under mu_: gen is stable here
    if (p->gen.load(std::memory_order_relaxed) != gen) return;
    if (close_pass(*p)) {
        for (auto& s : shards_)
            if (s.open.load(std::memory_order_relaxed) == p) s.open.store(nullptr, std::memory_order_release);
        closed_.push_back(p);
        work_cv_.notify_one();
    }
}

// ------------------------------------------------------------------------------ workers
// under mu_
void Core::start_workers() {
    if (!workers_.empty()) return;
    try {
        for (std::size_t w = 0; w < opt_.max_inflight; ++w) workers_.emplace_back([this] { work(); });
    } catch (const std::system_error&) {
        if (workers_.empty()) throw;
    }
}

// When a shard's open pass closes (max_delay 0): at a quarter of the size limits, when no
// frame has arrived for kGapUs (a lone caller or a burst that ended: not held back), or at
// kMaxLingerUs after its first frame -- a pass costs the device about the same for 100 frames
// or 1 000, so a steady stream is worth collecting.  With max_delay > 0: the size limits or max_delay.
constexpr double kGapUs = 30.0, kMaxLingerUs = 250.0;
// under mu_: should a free worker take the shard's open pass now?
bool Core::takeable(Shard& sh, const Pass& p) {
    const std::uint64_t r = p.res.load(std::memory_order_acquire);
    if (r & kClosedBit) return false;
    const std::uint64_t n = (r >> kSlotShift) & kSlotMask, b = r & kBytesMask;
    if (n == 0) return false;
    if (stop_ || n >= target_frames_ || b >= target_bytes_) return true;
    const double now = now_us();
    const double age = now - (double)p.first_us.load(std::memory_order_relaxed);
    if (opt_.max_delay.count() > 0) return age >= (double)opt_.max_delay.count();
    if (age >= kMaxLingerUs) return true;
    if (&p != sh.seen_pass || n != sh.seen_n) {  // still arriving: note it, look again later
        sh.seen_pass = &p;
        sh.seen_n = n;
        sh.seen_us = now;
        return false;
    }
    return now - sh.seen_us >= kGapUs;
}

void Core::work() {
    const bool fake = fake_us() > 0;
    Device dev;
    dev.ok = has_device_ && (fake || hipSetDevice(opt_.device) == hipSuccess);
    if (dev.ok && !fake) {
        dev.ok = hipStreamCreateWithFlags(&dev.stream, hipStreamNonBlocking) == hipSuccess &&
                 hipEventCreateWithFlags(&dev.ev, hipEventDisableTiming) == hipSuccess;
        if (!dev.ok) (void)hipGetLastError();
    }
    (void)prctl(PR_SET_TIMERSLACK, 1000ul, 0, 0, 0);  // fine-grained sleeps in run_on_device
    double cpu_seen = thread_cpu_s();
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
        Pass* p = nullptr;
        for (;;) {
            if (!closed_.empty()) {
                p = closed_.front();
                closed_.pop_front();
                break;
            }
            bool frames = false;
            for (unsigned si = 0; si < plan_.n; ++si) {
                Shard& sh = shards_[si];
                Pass* o = sh.open.load(std::memory_order_acquire);
                if (!o) continue;
                if (takeable(sh, *o)) {
                    if (close_pass(*o)) {
                        sh.open.store(nullptr, std::memory_order_release);
                        p = o;
                        break;
                    }
                    continue;
                }
                frames = frames || ((o->res.load(std::memory_order_acquire) >> kSlotShift) & kSlotMask) > 0;
            }
            if (p) break;
            if (stop_) {
                if (dev.dstage) (void)hipFree(dev.dstage);
                if (dev.ev) (void)hipEventDestroy(dev.ev);
                if (dev.stream) (void)hipStreamDestroy(dev.stream);
                return;
            }
            if (frames && !watching_) {  // one worker watches the open passes' arrivals
                watching_ = true;
                const double step = opt_.max_delay.count() > 0
                                        ? std::max<double>(1.0, (double)opt_.max_delay.count() / 4)
                                        : kGapUs / 2;
                work_cv_.wait_for(lk, std::chrono::microseconds((std::int64_t)step + 1));
                watching_ = false;
            } else {
                work_cv_.wait(lk);
            }
        }
        ++inflight_;
        lk.unlock();
        const bool host = run_pass(*p, &dev);
        const double cpu = thread_cpu_s();
        lk.lock();
        st_.worker_cpu_s += cpu - cpu_seen;
        cpu_seen = cpu;
        --inflight_;
        st_.frames += p->n;
        st_.flushes += 1;
        st_.host_flushes += host ? 1 : 0;
        done_.push_back(p);
        free_cv_.notify_all();
        work_cv_.notify_one();  // a peer may take an open pass now
    }
}

// A closed pass's filled prefix, packed into the arrays the kernel reads: sets p.n and p.in_used,
// returns the longest input.  Every reservation before the close writes its slot (filled, or the
// overflow mark where the pass ran full -- every later reservation is past the end too), so this
// waits for each slot's fill word in turn.
std::uint64_t Core::gather_slots(Pass& p) {
    const std::uint32_t lim = std::min(p.reserved, p.cap_frames);
    std::uint32_t n = lim;
    for (std::uint32_t i = 0; i < lim; ++i)
        if (spin_until(p.recs[i].fill, p.gen.load(std::memory_order_relaxed)) == kOverflow) {
            n = i;
            break;
        }
    std::uint64_t* io = p.in_off();
    std::uint64_t* oo = p.out_off();
    std::uint64_t mx = 0;
    for (std::uint32_t i = 0; i < n; ++i) {
        const SlotRec& r = p.recs[i];
        io[i] = r.in_at;
        oo[i] = p.out_at(r.in_at, i);
        std::memcpy(p.h + p.o_keys + 32ull * i, r.key, 32);
        if (!open_dir_) std::memcpy(p.h + p.o_nonces + 12ull * i, r.nonce, 12);
        mx = std::max(mx, r.len);
    }
    p.n = n;
    p.in_used = n ? p.recs[n - 1].in_at + p.recs[n - 1].len : 0;
    io[n] = p.in_used;
    oo[n] = p.out_at(p.in_used, n);
    return mx;
}

// the pass on the host engine, in place (same layout as the kernel's)
void Core::host_run(Pass& p) {
    for (std::uint32_t i = 0; i < p.n; ++i) {
        const std::uint64_t a = p.in_off()[i], b = p.in_off()[i + 1];
        std::span<const std::uint8_t> in(p.h + p.o_in + a, b - a);
        std::uint8_t* out = p.h + p.o_out + p.out_at(a, i);
        const std::uint8_t* key = p.h + p.o_keys + 32ull * i;
        if (open_dir_) p.h[p.o_ok + i] = host_wire_open_into(key, in, out) ? 1 : 0;
        else host_wire_seal_into(key, p.h + p.o_nonces + 12ull * i, in, out);
    }
}

// The wire-frame kernel over the pass, to completion; throws when a call fails.  Staged: the
// pass's input side (offsets, keys, nonces, messages: one contiguous prefix of the layout) goes
// to device memory by one SDMA copy and the kernel reads HBM; the results are still written
// straight into the pinned pass.
void Core::run_on_device(Pass& p, Device& dev, std::uint64_t max_len) {
    const std::uint8_t* din = p.d;
    if (stage_pass(p.n, open_dir_)) {
        if (!dev.dstage) {
            const hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev.dstage), p.o_out);
            if (e != hipSuccess) dev.dstage = nullptr;
            hip_ok(e, "hipMalloc");
        }
        hip_ok(hipMemcpyAsync(dev.dstage, p.h, p.o_in + p.in_used, hipMemcpyHostToDevice, dev.stream), "H2D pass");
        din = dev.dstage;
    }
    const enet_records r = enet::api::records_of(
        p.n, reinterpret_cast<const std::uint64_t*>(din + p.o_inoff),
        reinterpret_cast<const std::uint64_t*>(din + p.o_outoff), din + p.o_in, p.d + p.o_out, din + p.o_keys,
        open_dir_ ? nullptr : din + p.o_nonces, p.in_used, (std::uint32_t)std::min<std::uint64_t>(max_len, 0xFFFFFFFFu));
    const int rc = open_dir_ ? enet_wire_open_batch(&r, p.d + p.o_macs, p.d + p.o_ok, dev.stream)
                             : enet_wire_seal_batch(&r, dev.stream);
    if (rc != ENET_OK) throw std::runtime_error(enet_last_error());
    hip_ok(hipEventRecord(dev.ev, dev.stream), "hipEventRecord");
    // Poll with ~20 us sleeps (a blocking-sync event cost the worker 4x the CPU per frame,
    // profiles/r05c_queue_bench.jsonl); the first sleep covers most of this worker's recent
    // kernel time (a decaying average), so a pass costs a couple of wake-ups instead of ~10.
    const double first = 0.7 * dev.kern_ema_us - 20.0;
    if (first > 0) std::this_thread::sleep_for(std::chrono::microseconds((std::int64_t)first));
    hipError_t q;
    while ((q = hipEventQuery(dev.ev)) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(20));
    enet::stage::hip_check(q, "hipEventQuery");
}

// Run one closed pass: on the device (`dev`: the calling worker's) or, without one, under the
// HOST policy or after a failed launch, on the host engine (same layout); true when the host
// engine served it
bool Core::run_pass(Pass& p, Device* dev) {
    const double t0 = now_us();
    const std::uint64_t max_len = gather_slots(p);
    const double t1 = now_us();
    const char* what = open_dir_ ? "FrameReceiveQueue pass" : "FrameQueue pass";
    const bool want_dev = enet::scalar::g_policy.load() != ENET_SCALAR_HOST;
    const bool can_dev = dev && dev->ok && p.d;
    bool host = true;
    if (p.n && want_dev && !can_dev)  // counted like a failed launch (enet_scalar_get_stats)
        enet::scalar::device_failed(what, "no usable device or pinned staging");
    if (p.n && want_dev && can_dev && fake_us() > 0) {
        host = false;
        fake_device_pass([&] { host_run(p); }, open_dir_ ? p.h + p.o_ok : nullptr, p.n);
    } else if (p.n && want_dev && can_dev) {
        host = !enet::scalar::try_device(what, [&] { run_on_device(p, *dev, max_len); });
    }
    if (host && p.n) {
        enet::scalar::host_call();
        host_run(p);
    }
    const double t2 = now_us();
    {
        std::lock_guard<std::mutex> lk(p.mu);
        p.state.store(kDone, std::memory_order_release);
    }
    p.cv.notify_all();
    if (!host) {
        dev->kern_ema_us = dev->kern_ema_us > 0 ? 0.8 * dev->kern_ema_us + 0.2 * (t2 - t1) : t2 - t1;
        std::lock_guard<std::mutex> lk(mu_);
        dev_passes_ += 1;
        sum_pass_us_ += t2 - p.closed_at;
        sum_kernel_us_ += t2 - t1;
        sum_fill_us_ += t1 - t0;
    }
    return host;
}

}  // namespace enet::fq
