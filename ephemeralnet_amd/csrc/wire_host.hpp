// wire_host.hpp -- one wire frame on the host engine, as the frame queues serve it on a caller's
// thread or in a host pass: nonce(12) || BE32(|body|) || body (SessionManager.cpp:376-385), the
// shape check of the receive side, and the per-thread nonce generator.
#pragma once

#include <atomic>
#include <cstdint>
#include <cstring>
#include <random>
#include <span>
#include <vector>

#include <pthread.h>

#include "api_common.hpp"
#include "ephemeralnet/crypto/Batch.hpp"
#include "host_engine.hpp"

namespace enet::fq {

constexpr std::size_t kHeader = 16;  // nonce(12) || BE32(|body|), SessionManager.cpp:376-385
constexpr std::size_t kMac = 32;
constexpr std::size_t kWire = kHeader + kMac;  // |frame| - |message|

// SessionManager::send for one frame, into `f` (|m| + 48 bytes)
inline void host_wire_seal_into(const std::uint8_t key[32], const std::uint8_t nonce[12],
                                std::span<const std::uint8_t> m, std::uint8_t* f) {
    enet::host::seal_body(key, nonce, m.data(), m.size(), f + kHeader);
    std::memcpy(f, nonce, 12);
    enet::api::put_be32(f + 12, (std::uint32_t)(m.size() + kMac));
}

inline std::vector<std::uint8_t> host_wire_seal(const std::uint8_t key[32], const std::uint8_t nonce[12],
                                                std::span<const std::uint8_t> m) {
    std::vector<std::uint8_t> f(kWire + m.size());
    host_wire_seal_into(key, nonce, m, f.data());
    return f;
}

// the length checks of receive_loop (:760-796) and decode_signed (Message.cpp:315)
inline bool frame_shape_ok(std::span<const std::uint8_t> f) {
    if (f.size() < kWire) return false;
    const std::uint32_t len = (std::uint32_t)f[12] << 24 | (std::uint32_t)f[13] << 16 |
                              (std::uint32_t)f[14] << 8 | f[15];
    return (std::uint64_t)len == f.size() - kHeader &&
           len <= ephemeralnet::crypto::batch::FrameQueue::kMaxPayloadSize;
}

// receive_loop decrypt + decode_signed verify for one frame (shape already checked); the message
// goes to `m` (|f| - 48 bytes; zeroed when the MAC does not verify)
inline bool host_wire_open_into(const std::uint8_t key[32], std::span<const std::uint8_t> f, std::uint8_t* m) {
    return enet::host::open_body(key, f.data(), f.data() + kHeader, f.size() - kHeader, m);
}

// Frame nonces.  SessionManager::send draws each nonce from a fresh std::random_device
// (SessionManager.cpp:365-371); on the box that source serves ~0.4 M nonces/s for the whole
// machine however many threads ask, which capped every sender.  Each thread here keeps a
// ChaCha20 keystream generator keyed with 256 bits from std::random_device and re-keyed every
// 2^20 nonces (the arc4random construction): 12 unpredictable bytes per frame, never reused under
// one session key.  fork() copies a thread's generator into the child, so parent and child would
// hand out the same nonces; a pthread_atfork child handler bumps a generation
// counter, and a generator whose generation is stale re-keys from std::random_device before its
// next nonce.
inline std::atomic<std::uint32_t> g_fork_generation{0};
[[maybe_unused]] inline const int g_atfork_registered = pthread_atfork(nullptr, nullptr, [] {
    g_fork_generation.fetch_add(1, std::memory_order_relaxed);
});

class NonceSource {
public:
    void draw(std::uint8_t* n) {
        const std::uint32_t gen = g_fork_generation.load(std::memory_order_relaxed);
        if (gen != gen_) {  // first use, or a forked child: new key, discard buffered keystream
            gen_ = gen;
            left_ = 0;
            pos_ = sizeof(buf_);
        }
        if (pos_ + 12 > sizeof(buf_)) refill();
        std::memcpy(n, buf_ + pos_, 12);
        std::memset(buf_ + pos_, 0, 12);
        pos_ += 12;
    }

private:
    void refill() {
        if (left_ == 0) {
            std::random_device rd;
            std::uint32_t seed[11];  // key (8 words), then iv (3)
            for (auto& v : seed) v = rd();
            std::memcpy(key_, seed, 32);
            std::memcpy(iv_, seed + 8, 12);
            ctr_ = 0;
            left_ = 1u << 20;
        }
        // whole keystream blocks only: the next refill starts at the next unused block, so no
        // keystream byte (and no nonce) is ever handed out twice
        std::memset(buf_, 0, sizeof(buf_));
        enet::host::chacha20_xor(key_, iv_, ctr_, buf_, buf_, sizeof(buf_));
        ctr_ += kBlocks;
        pos_ = 0;
        left_ = left_ > kPerFill ? left_ - kPerFill : 0;
    }
    static constexpr std::uint32_t kBlocks = 16;                   // keystream blocks per fill
    static constexpr std::uint32_t kPerFill = kBlocks * 64 / 12;  // 85 nonces per fill
    std::uint8_t key_[32] = {}, iv_[12] = {};
    std::uint32_t ctr_ = 0, left_ = 0, gen_ = 0;
    std::uint8_t buf_[kBlocks * 64] = {};
    std::size_t pos_ = sizeof(buf_);
};

inline NonceSource& nonce_source() {
    thread_local NonceSource src;
    return src;
}

}  // namespace enet::fq
