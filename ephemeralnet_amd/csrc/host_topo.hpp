// host_topo.hpp -- where the host side of a device's work runs: the device's NUMA node, the CPUs
// and CPU budget its host worker threads get, and pinned host memory placed on that node.
//
// The host-resident path (SessionManager.cpp:1049-1099, Node.cpp:1414-1417: socket / relay buffers
// and chunk files in host memory) moves every byte through host DRAM twice per direction (gather
// or DMA in, DMA or scatter out).  On a two-socket node half of the GPUs sit across the socket
// link from any given buffer, and the process usually runs under a cgroup CPU quota far below the
// machine's CPU count (the GPU box: 16 of 256), so the runtime plans both explicitly:
//   * staging and enet_host_alloc blocks on the device's node (mbind + hipHostRegister);
//   * pool threads bound to that node's CPUs (intersected with the process's affinity mask);
//   * pool sizes from the effective CPU budget (affinity, cgroup quota, ENET_HOST_CPUS) divided
//     among the engines alive in the process, spinning only while every thread has a CPU.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <string_view>
#include <vector>

namespace enet::topo {

// "0-3,8,10-11" -> {0,1,2,3,8,10,11} (sorted, unique); malformed parts are skipped
std::vector<int> parse_cpulist(std::string_view s);
std::string format_cpulist(const std::vector<int>& cpus);
// cgroup v2 cpu.max ("quota period" or "max period") -> CPUs granted (ceil), 0 = unlimited
uint32_t quota_cpus(std::string_view cpu_max);

// The plan for one engine's host threads, from the facts below (pure: CPU-tested with synthetic
// topologies through enet_host_plan).
struct Plan {
    std::vector<int> cpus;  // where the engine's pool threads run (node CPUs within `allowed`)
    uint32_t budget = 1;    // CPUs this process may use
    uint32_t workers = 0;   // pool threads of this engine (the calling thread works too)
    bool spin = false;      // pool threads spin briefly between task sets (only if they fit)
};
// node_cpus: the device node's CPUs (empty = unknown); allowed: the affinity mask; quota: cgroup
// CPUs (0 = unlimited); env_cpus: ENET_HOST_CPUS (0 = unset); engines: engines sharing the budget
Plan plan(const std::vector<int>& node_cpus, const std::vector<int>& allowed, uint32_t quota, uint32_t env_cpus,
          uint32_t engines);

// facts of this machine / process
int device_numa_node(int device);   // -1 unknown (no sysfs entry, single-node machine)
std::vector<int> node_cpus(int node);
const std::vector<int>& l3_of_cpu();  // dense L3-domain (CCD) index of every CPU, -1 unknown; read once
std::vector<int> allowed_cpus();     // sched_getaffinity of the calling thread
uint32_t cgroup_quota_cpus();        // 0 = unlimited / unknown
uint32_t env_cpus();                 // ENET_HOST_CPUS, 0 = unset
int page_node(const void* p);        // NUMA node of the page at p (-1 unknown / not faulted)
int numa_nodes();                    // nodes online (1 when unknown)

// Placement policy of pinned host memory (ENET_HOST_NUMA): -1 = the device's node ("auto",
// default), -2 = leave it to hipHostMalloc ("hip"), >= 0 = that node.
int placement_policy();
// the node pinned memory for `device` goes to under the policy (-1 = hipHostMalloc decides)
int target_node(int device);

// Pinned, device-mapped host memory on `node` (anonymous mapping bound MPOL_PREFERRED to the node,
// faulted in, then hipHostRegister'ed); node < 0: hipHostMalloc(Mapped).  Returns the host
// address; *dev gets the device address.  Throws std::runtime_error / std::bad_alloc.
void* alloc_pinned(size_t n, int node, void** dev);
void free_pinned(void* p);           // either kind; nullptr is a no-op
// pinned bytes currently held through alloc_pinned (this process)
uint64_t pinned_bytes();
// Host ranges this library pinned (alloc_pinned) or registered (enet_host_register), with their
// device address.  known_device_view: the device address of [p, p + n) when the whole range lies
// in one of them, else nullptr (then ask HIP).  Consulted before HIP's range queries: C5 at its
// full size (three 7 GB enet_host_alloc arenas) was gathered through the staging with only the
// HIP queries (19.99 GiB/s, 8 workers) and runs in place with this record (21.6-21.7, none;
// profiles/r05z_side.jsonl, r05m_c5_full.jsonl).
void note_range(const void* p, uint64_t n, void* dev);
void forget_range(const void* p);
uint8_t* known_device_view(const void* p, uint64_t n);

}  // namespace enet::topo
