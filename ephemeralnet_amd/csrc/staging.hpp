// staging.hpp -- the per-thread device staging of the C++ drop-in: the buffers and the stream
// behind every crypto::batch / security::batch call that drives the C ABI itself
// (batch_staged.cpp) and behind the scalar API's device path (scalar_api.cpp), plus the two
// throwing checks every host translation unit uses.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <span>
#include <vector>

namespace enet::stage {

// throw std::runtime_error("enet: <what>: <reason>") unless the call succeeded
void hip_check(hipError_t e, const char* what);
void enet_check(int rc, const char* what);  // rc of the C ABI; the reason is enet_last_error()

// A call names the slot of each buffer itself: two buffers of one slot alias once they leave the
// host blob (above kZeroCopyMax), and a slot keeps the largest capacity it ever served.
enum Slot { S_IN = 0, S_OUT, S_INOFF, S_OUTOFF, S_KEYS, S_NONCES, S_CTR, S_TAGS, S_OK, S_AUX };

// Staging buffers + one stream per host thread, for the batch API and the scalar API's device
// path under ENET_SCALAR_DEVICE.  Buffers of up to kZeroCopyMax bytes come from one pinned,
// device-mapped, coherent host blob -- "uploading" is a host memcpy into it, the kernel reads
// its operands over PCIe and writes its results straight back, and "downloading" is a memcpy
// after the stream sync -- so a small call costs one launch and one sync instead of up to six
// pageable copies.  The blob is 256 KiB (every small call fits: ~10 slots of <= 8 KiB; ADVICE r02:
// 8 MiB per session thread pinned too much), allocated on the first small call of a thread.
// Larger buffers keep grow-only device slots and async copies.  The blob is bump-allocated and
// rewound at every sync (every API call ends with one), so no region is rewritten while a kernel
// of the same call may still read it.
struct Staging {
    static constexpr int kSlots = 10;
    static constexpr size_t kHostBlob = 256u << 10;
    static constexpr size_t kZeroCopyMax = 8u << 10;  // a serial SHA lane pays PCIe latency per block
    void* dev[kSlots] = {};
    size_t cap[kSlots] = {};
    hipStream_t stream = nullptr;
    uint8_t* host = nullptr;
    bool host_failed = false;
    size_t used = 0;
    struct Pending {
        void* dst;
        const void* src;
        size_t n;
    };
    std::vector<Pending> pend;

    ~Staging();
    bool in_host(const void* p) const {
        return host && p >= host && static_cast<const uint8_t*>(p) < host + kHostBlob;
    }
    void* get(int slot, size_t bytes);
    hipStream_t s();
    void h2d(void* d, const void* h, size_t n);
    void d2h(void* h, const void* d, size_t n);
    // room for `bytes` in `slot`, and the same filled with the caller's `bytes` at `src`
    template <class T = uint8_t>
    T* room(Slot slot, size_t bytes) {
        return static_cast<T*>(get(slot, bytes));
    }
    template <class T = uint8_t>
    T* up(Slot slot, const void* src, size_t bytes) {
        T* d = room<T>(slot, bytes);
        h2d(d, src, bytes);
        return d;
    }
    // Wait for the call's work, then run the deferred zero-copy downloads.  The pending list and
    // the blob are released BEFORE the status check: a failed sync must not leave pointers into
    // the caller's (about to be destroyed) vectors for the next call to write through.
    void sync();
    // drop queued downloads and rewind after a failed call
    void reset() noexcept {
        pend.clear();
        used = 0;
    }
};

// the calling thread's instance, one per thread for the whole library
Staging& staging();

// device memory also for a small buffer (Staging serves small buffers from host-resident staging)
constexpr size_t kDeviceOnly = Staging::kZeroCopyMax + 1;

// One Staging sequence: starts from a rewound staging (a previous call that threw may have left
// queued downloads) and rewinds it again before an exception leaves, so the next call starts clean.
template <class F>
auto staged(F&& f) -> decltype(f(staging())) {
    Staging& st = staging();
    st.reset();
    try {
        return f(st);
    } catch (...) {
        st.reset();
        throw;
    }
}

// Host-side packing of a list of byte spans into one arena + offsets.
struct Packed {
    std::vector<uint8_t> arena;
    std::vector<uint64_t> off;
};
Packed pack(std::span<const std::span<const uint8_t>> items);
// prefix sums of max(0, |item| + delta)
std::vector<uint64_t> offsets_of(std::span<const std::span<const uint8_t>> items, int64_t delta);

}  // namespace enet::stage
