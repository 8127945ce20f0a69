// staging.cpp -- the per-thread device staging of the C++ drop-in (staging.hpp).
#include "staging.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

#include "enet_crypto.h"

namespace enet::stage {

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw std::runtime_error(std::string("enet: ") + what + ": " + hipGetErrorString(e));
}

void enet_check(int rc, const char* what) {
    if (rc != ENET_OK) throw std::runtime_error(std::string("enet: ") + what + ": " + enet_last_error());
}

Staging::~Staging() {
    for (int i = 0; i < kSlots; ++i)
        if (dev[i]) (void)hipFree(dev[i]);
    if (host) (void)hipHostFree(host);
    if (stream) (void)hipStreamDestroy(stream);
}

void* Staging::get(int slot, size_t bytes) {
    bytes = std::max<size_t>(bytes, 64);
    if (bytes <= kZeroCopyMax && !host_failed) {
        if (!host && hipHostMalloc(reinterpret_cast<void**>(&host), kHostBlob,
                                   hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            host = nullptr;
            host_failed = true;
        }
        const size_t off = (used + 255) & ~size_t(255);
        if (host && off + bytes <= kHostBlob) {
            used = off + bytes;
            return host + off;
        }
    }
    if (cap[slot] < bytes) {
        if (dev[slot]) {
            (void)hipFree(dev[slot]);
            dev[slot] = nullptr;
            cap[slot] = 0;
        }
        size_t c = std::max(bytes, cap[slot] * 2);
        hip_check(hipMalloc(&dev[slot], c), "hipMalloc");
        cap[slot] = c;
    }
    return dev[slot];
}

hipStream_t Staging::s() {
    if (!stream) hip_check(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
    return stream;
}

void Staging::h2d(void* d, const void* h, size_t n) {
    if (!n) return;
    if (in_host(d)) std::memcpy(d, h, n);
    else hip_check(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s()), "H2D");
}

void Staging::d2h(void* h, const void* d, size_t n) {
    if (!n) return;
    if (in_host(d)) pend.push_back({h, d, n});
    else hip_check(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, s()), "D2H");
}

void Staging::sync() {
    std::vector<Pending> todo;
    todo.swap(pend);
    used = 0;
    hip_check(hipStreamSynchronize(s()), "hipStreamSynchronize");
    for (const Pending& q : todo) std::memcpy(q.dst, q.src, q.n);
}

Staging& staging() {
    thread_local Staging st;
    return st;
}

Packed pack(std::span<const std::span<const uint8_t>> items) {
    Packed p;
    p.off = offsets_of(items, 0);
    p.arena.resize(p.off.back());
    for (size_t i = 0; i < items.size(); ++i)
        if (!items[i].empty()) std::memcpy(p.arena.data() + p.off[i], items[i].data(), items[i].size());
    return p;
}

std::vector<uint64_t> offsets_of(std::span<const std::span<const uint8_t>> items, int64_t delta) {
    std::vector<uint64_t> off(items.size() + 1);
    uint64_t total = 0;
    for (size_t i = 0; i < items.size(); ++i) {
        off[i] = total;
        int64_t len = (int64_t)items[i].size() + delta;
        total += (uint64_t)std::max<int64_t>(len, 0);
    }
    off[items.size()] = total;
    return off;
}

}  // namespace enet::stage
