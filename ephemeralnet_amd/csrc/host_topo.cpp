// host_topo.cpp -- NUMA node, CPU set / budget and node-placed pinned memory for the host-memory
// runtime (host_topo.hpp).  Linux sysfs / syscalls only (no libnuma): the node of a device from
// its PCI function's numa_node, CPU lists from /sys/devices/system/node, the cgroup quota from
// cpu.max along the process's cgroup path, page placement by mbind / get_mempolicy.
#include "host_topo.hpp"

#include <hip/hip_runtime.h>
#include <numaif.h>  // MPOL_* constants (the calls go through syscall(): no libnuma at link time)
#include <sched.h>
#include <sys/mman.h>
#include <sys/syscall.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <mutex>
#include <new>
#include <sstream>
#include <stdexcept>
#include <thread>

namespace enet::topo {

namespace {

std::string read_file(const std::string& path) {
    std::ifstream f(path);
    if (!f) return {};
    std::stringstream ss;
    ss << f.rdbuf();
    std::string s = ss.str();
    while (!s.empty() && std::isspace((unsigned char)s.back())) s.pop_back();
    return s;
}

bool parse_int(std::string_view s, long long& v) {
    if (s.empty()) return false;
    char buf[32];
    if (s.size() >= sizeof(buf)) return false;
    std::memcpy(buf, s.data(), s.size());
    buf[s.size()] = 0;
    char* end = nullptr;
    v = std::strtoll(buf, &end, 10);
    return end && *end == 0;
}

}  // namespace

std::vector<int> parse_cpulist(std::string_view s) {
    std::vector<int> out;
    size_t i = 0;
    while (i < s.size()) {
        size_t j = s.find(',', i);
        if (j == std::string_view::npos) j = s.size();
        std::string_view part = s.substr(i, j - i);
        while (!part.empty() && std::isspace((unsigned char)part.front())) part.remove_prefix(1);
        while (!part.empty() && std::isspace((unsigned char)part.back())) part.remove_suffix(1);
        const size_t dash = part.find('-');
        long long a = 0, b = 0;
        if (dash == std::string_view::npos) {
            if (parse_int(part, a) && a >= 0 && a < (1 << 20)) out.push_back((int)a);
        } else if (parse_int(part.substr(0, dash), a) && parse_int(part.substr(dash + 1), b) && a >= 0 && b >= a &&
                   b < (1 << 20)) {
            for (long long c = a; c <= b; ++c) out.push_back((int)c);
        }
        i = j + 1;
    }
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return out;
}

std::string format_cpulist(const std::vector<int>& cpus) {
    std::string s;
    for (size_t i = 0; i < cpus.size();) {
        size_t j = i;
        while (j + 1 < cpus.size() && cpus[j + 1] == cpus[j] + 1) ++j;
        if (!s.empty()) s += ',';
        s += std::to_string(cpus[i]);
        if (j > i) s += '-' + std::to_string(cpus[j]);
        i = j + 1;
    }
    return s;
}

uint32_t quota_cpus(std::string_view cpu_max) {
    const size_t sp = cpu_max.find(' ');
    if (sp == std::string_view::npos) return 0;
    std::string_view q = cpu_max.substr(0, sp), p = cpu_max.substr(sp + 1);
    while (!p.empty() && std::isspace((unsigned char)p.back())) p.remove_suffix(1);
    long long qv = 0, pv = 0;
    if (q == "max" || !parse_int(q, qv) || !parse_int(p, pv) || qv <= 0 || pv <= 0) return 0;
    return (uint32_t)std::max<long long>(1, (qv + pv - 1) / pv);
}

Plan plan(const std::vector<int>& node_cpus, const std::vector<int>& allowed, uint32_t quota, uint32_t env_cpus,
          uint32_t engines) {
    Plan p;
    const uint32_t n_allowed = std::max<uint32_t>(1, (uint32_t)allowed.size());
    uint32_t budget = n_allowed;
    if (quota) budget = std::min(budget, quota);
    if (env_cpus) budget = std::min(env_cpus, n_allowed);
    p.budget = std::max<uint32_t>(1, budget);
    // the node's CPUs this process may run on; none (unknown node, or the mask excludes it): the mask
    std::set_intersection(node_cpus.begin(), node_cpus.end(), allowed.begin(), allowed.end(),
                          std::back_inserter(p.cpus));
    if (p.cpus.empty()) p.cpus = allowed;
    // threads per engine (the caller included): the budget shared by the engines alive; at most
    // 8 workers (gather / scatter of a 32 MiB chunk saturates host memory with ~8 streaming cores)
    const uint32_t per = std::max<uint32_t>(1, p.budget / std::max<uint32_t>(1, engines));
    uint32_t w = std::min<uint32_t>(8, per - 1);
    if (!p.cpus.empty()) w = std::min<uint32_t>(w, (uint32_t)p.cpus.size() - 1);
    p.workers = w;
    p.spin = (uint64_t)std::max<uint32_t>(1, engines) * (p.workers + 1) <= p.budget;
    return p;
}

int numa_nodes() {
    const auto on = parse_cpulist(read_file("/sys/devices/system/node/online"));
    return std::max<int>(1, (int)on.size());
}

int device_numa_node(int device) {
    char bdf[64] = {};
    if (hipDeviceGetPCIBusId(bdf, sizeof(bdf), device) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    for (char* c = bdf; *c; ++c) *c = (char)std::tolower((unsigned char)*c);
    long long v = -1;
    if (!parse_int(read_file(std::string("/sys/bus/pci/devices/") + bdf + "/numa_node"), v)) return -1;
    return v >= 0 ? (int)v : -1;
}

std::vector<int> node_cpus(int node) {
    if (node < 0) return {};
    return parse_cpulist(read_file("/sys/devices/system/node/node" + std::to_string(node) + "/cpulist"));
}

// The L3 domains from sysfs: cpuN/cache/indexK with level 3 names its domain by id; the ids are
// made dense in order of first appearance
const std::vector<int>& l3_of_cpu() {
    static const std::vector<int> v = [] {
        std::vector<int> out, ids;
        const long ncpu = sysconf(_SC_NPROCESSORS_CONF);
        for (long c = 0; c < ncpu && c < 4096; ++c) {
            int dense = -1;
            for (int idx = 0; idx < 6 && dense < 0; ++idx) {
                const std::string dir =
                    "/sys/devices/system/cpu/cpu" + std::to_string(c) + "/cache/index" + std::to_string(idx);
                long long level = 0, id = -1;
                if (!parse_int(read_file(dir + "/level"), level) || level != 3) continue;
                if (!parse_int(read_file(dir + "/id"), id) || id < 0) continue;
                const auto it = std::find(ids.begin(), ids.end(), (int)id);
                dense = (int)(it - ids.begin());
                if (it == ids.end()) ids.push_back((int)id);
            }
            out.push_back(dense);
        }
        return out;
    }();
    return v;
}

std::vector<int> allowed_cpus() {
    std::vector<int> out;
    const int max_cpus = 8192;
    cpu_set_t* set = CPU_ALLOC(max_cpus);
    if (!set) return out;
    const size_t sz = CPU_ALLOC_SIZE(max_cpus);
    CPU_ZERO_S(sz, set);
    if (sched_getaffinity(0, sz, set) == 0)
        for (int c = 0; c < max_cpus; ++c)
            if (CPU_ISSET_S(c, sz, set)) out.push_back(c);
    CPU_FREE(set);
    if (out.empty()) {
        const unsigned hc = std::max(1u, std::thread::hardware_concurrency());
        for (unsigned c = 0; c < hc; ++c) out.push_back((int)c);
    }
    return out;
}

uint32_t cgroup_quota_cpus() {
    // cgroup v2: every cpu.max from the process's cgroup up to the root limits it; take the least
    uint32_t best = 0;
    auto take = [&](uint32_t q) {
        if (q && (!best || q < best)) best = q;
    };
    std::string path;
    {
        std::ifstream f("/proc/self/cgroup");
        std::string line;
        while (std::getline(f, line))
            if (line.rfind("0::", 0) == 0) path = line.substr(3);
    }
    for (std::string p = path;;) {
        take(quota_cpus(read_file("/sys/fs/cgroup" + p + "/cpu.max")));
        if (p.empty() || p == "/") break;
        const size_t s = p.rfind('/');
        p = s == std::string::npos ? std::string() : p.substr(0, s);
    }
    take(quota_cpus(read_file("/sys/fs/cgroup/cpu.max")));
    // cgroup v1
    long long q = 0, per = 0;
    for (const char* d : {"/sys/fs/cgroup/cpu", "/sys/fs/cgroup/cpu,cpuacct"})
        if (parse_int(read_file(std::string(d) + "/cpu.cfs_quota_us"), q) &&
            parse_int(read_file(std::string(d) + "/cpu.cfs_period_us"), per) && q > 0 && per > 0)
            take((uint32_t)std::max<long long>(1, (q + per - 1) / per));
    return best;
}

uint32_t env_cpus() {
    const char* e = std::getenv("ENET_HOST_CPUS");
    long long v = 0;
    return e && parse_int(e, v) && v > 0 ? (uint32_t)std::min<long long>(v, 1 << 16) : 0u;
}

int page_node(const void* p) {
    int node = -1;
    if (syscall(SYS_get_mempolicy, &node, nullptr, 0ul, const_cast<void*>(p), (unsigned long)(MPOL_F_NODE | MPOL_F_ADDR)) != 0)
        return -1;
    return node;
}

int placement_policy() {
    static const int v = [] {
        const char* e = std::getenv("ENET_HOST_NUMA");
        if (!e || !*e || std::strcmp(e, "auto") == 0) return -1;
        if (std::strcmp(e, "hip") == 0 || std::strcmp(e, "off") == 0) return -2;
        long long n = -1;
        return parse_int(e, n) && n >= 0 && n < 1024 ? (int)n : -1;
    }();
    return v;
}

int target_node(int device) {
    const int pol = placement_policy();
    if (pol == -2) return -1;
    if (pol >= 0) return pol;
    if (numa_nodes() <= 1) return -1;  // one node: nothing to place
    return device_numa_node(device);
}

namespace {

struct Block {
    size_t len;
    bool registered;  // mmap + hipHostRegister (else hipHostMalloc)
};
std::mutex g_mu;
std::map<void*, Block>* g_blocks = new std::map<void*, Block>();  // never destroyed: no HIP at exit
std::atomic<uint64_t> g_pinned{0};
// every host range this library pinned or registered, by start: length and device address
struct Range {
    uint64_t len;
    uint8_t* dev;
};
std::map<const uint8_t*, Range>* g_ranges = new std::map<const uint8_t*, Range>();

}  // namespace

void* alloc_pinned(size_t n, int node, void** dev) {
    n = std::max<size_t>(n, 1);
    void* h = nullptr;
    void* d = nullptr;
    bool registered = false;
    size_t len = n;
    if (node >= 0) {
        const size_t pg = (size_t)sysconf(_SC_PAGESIZE);
        len = (n + pg - 1) / pg * pg;
        h = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
        if (h == MAP_FAILED) throw std::bad_alloc();
        unsigned long mask[16] = {};
        if (node < 1024) mask[node / 64] = 1ul << (node % 64);
        // preferred, not bound: a full node falls back to another instead of failing the job
        (void)syscall(SYS_mbind, h, len, (unsigned long)MPOL_PREFERRED, mask, 1024ul + 1, 0ul);
        for (size_t o = 0; o < len; o += pg) static_cast<volatile uint8_t*>(h)[o] = 0;  // fault on the node
        if (hipHostRegister(h, len, hipHostRegisterMapped) != hipSuccess) {
            (void)hipGetLastError();
            munmap(h, len);
            throw std::runtime_error("enet host memory: hipHostRegister failed");
        }
        registered = true;
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipHostUnregister(h);
            munmap(h, len);
            throw std::runtime_error("enet host memory: hipHostGetDevicePointer failed");
        }
    } else {
        if (hipHostMalloc(&h, n, hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            throw std::runtime_error("enet host memory: hipHostMalloc failed");
        }
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipHostFree(h);
            throw std::runtime_error("enet host memory: hipHostGetDevicePointer failed");
        }
    }
    {
        std::lock_guard<std::mutex> lk(g_mu);
        (*g_blocks)[h] = Block{len, registered};
        (*g_ranges)[static_cast<const uint8_t*>(h)] = Range{len, static_cast<uint8_t*>(d)};
    }
    g_pinned.fetch_add(len);
    if (dev) *dev = d;
    return h;
}

void free_pinned(void* p) {
    if (!p) return;
    Block b{0, false};
    bool known = false;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_blocks->find(p);
        if (it != g_blocks->end()) {
            b = it->second;
            known = true;
            g_blocks->erase(it);
        }
        g_ranges->erase(static_cast<const uint8_t*>(p));
    }
    if (!known) {  // not ours: hipHostMalloc'ed by someone else (enet_host_free of a foreign block)
        (void)hipHostFree(p);
        return;
    }
    g_pinned.fetch_sub(b.len);
    if (b.registered) {
        (void)hipHostUnregister(p);
        munmap(p, b.len);
    } else {
        (void)hipHostFree(p);
    }
}

uint64_t pinned_bytes() { return g_pinned.load(); }

void note_range(const void* p, uint64_t n, void* dev) {
    std::lock_guard<std::mutex> lk(g_mu);
    (*g_ranges)[static_cast<const uint8_t*>(p)] = Range{n, static_cast<uint8_t*>(dev)};
}

void forget_range(const void* p) {
    std::lock_guard<std::mutex> lk(g_mu);
    g_ranges->erase(static_cast<const uint8_t*>(p));
}

uint8_t* known_device_view(const void* p, uint64_t n) {
    const auto* q = static_cast<const uint8_t*>(p);
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_ranges->upper_bound(q);
    if (it == g_ranges->begin()) return nullptr;
    --it;
    const uint64_t off = (uint64_t)(q - it->first);
    if (off >= it->second.len || n > it->second.len - off || !it->second.dev) return nullptr;
    return it->second.dev + off;
}

}  // namespace enet::topo
