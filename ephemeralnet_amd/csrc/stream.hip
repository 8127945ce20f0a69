// stream.hip -- the streaming ChaCha20 / ChaCha20-Poly1305 kernel for uniform batches (gfx950).
//
// Shape: every record is L bytes with L a multiple of 128*P (P = lanes per record), records
// contiguous in both arenas (C2: 65 536 x 4 KiB, C4: 64 KiB chunks).  Lane j of record g owns
// blocks [j*B, (j+1)*B), B = L/(64 P), and moves them in stages of two blocks (128 bytes per
// lane, 8 KiB per wave).  Thread t of a workgroup of R = 512 / P records is lane t / R of record
// t mod R (stream_map.hpp): lane j of every record sits in wave group j, so what one lane of a
// record does for all of it -- the leader, j = 0: the one-time key, the AAD, the tag -- whole waves
// skip on a scalar branch, and the leader's r, the other lanes' Poly1305 sums and open's verdict
// cross through a small LDS exchange on the barriers S0(0), F1 and F2 that every wave meets anyway.
//
// One 768-thread workgroup per CU, two kinds of waves:
//   * 8 compute waves (two per SIMD, the records' 512 lanes) run the keystream in the lockstep
//     pair schedule (enet_device.hpp: both waves of a SIMD meet at s_barrier after every 24
//     ChaCha instructions, so their full-rate adds / xors pair up) and Poly1305, reading their
//     stage from an LDS input slab and writing it to an LDS output slab.  No global memory
//     instruction, no branch and no wait sits in their keystream, and no Poly1305 either: a
//     stage's Poly1305 runs behind its last keystream barrier in seal and open alike (open's is
//     held there, stream_issue below: left to the compiler most of it went into the
//     stage's first barrier intervals, and the C2 bench lost 1.2 %).
//     The two compute waves of a SIMD run at equal issue priority: raising either half, or
//     both, moved nothing.
//   * 4 memory waves (one per SIMD) move the bytes: each serves two compute waves, issuing one
//     instruction between two consecutive keystream barriers on a fixed schedule -- the 16 LDS
//     DMAs (global_load_lds_dwordx4, whole 128-byte lines) of the next stage early in the stage,
//     then the 16 whole-line non-temporal stores of the previous stage spread over it.  So every
//     CU feeds HBM a steady stream instead of bursts at stage boundaries (which, with all CUs in
//     phase, backed the memory system up and stalled the keystream: tools/stream_probe.sh,
//     tools/stall_pmc.sh), and the compute waves never wait on HBM.
// Hand-offs use the shared barriers: the stage barrier S0 (inputs landed: the memory waves wait
// for their DMAs before it; outputs of the previous stage written: the compute waves drain
// their LDS writes before it) and keystream barrier 0 (the compute waves have read their inputs,
// so the slab may be refilled).  LDS: 2 x 64 KiB, and up to 15 KiB of exchange (AEAD, P > 1).
// The LDS chunk swizzle sw(o) = ((o >> 1) & 7) ^ ((o & 1) << 2) makes the own-run ds_read_b128
// (lane groups of 16: (sw, o & 1) distinct) and ds_write_b128 (8 contiguous lanes: sw distinct)
// conflict-free (PMC SQ_LDS_BANK_CONFLICT = 0); the lane-linear DMA landing and store reads are
// contiguous.
//
// A workgroup first checks that each of its records sits at in_off[0] + g*L / out_off[0] + g*L
// (the caller's hints declared the batch uniform); if any does not, the whole workgroup runs the
// per-lane path of records_body.hpp instead (COOP 7), so a wrong hint costs speed, never bytes.
//
// Reference behaviour: ChaCha20::apply (src/crypto/ChaCha20.cpp:98-121, u32 counter wrap :110)
// for MODE_XOR; RFC 8439 AEAD (no reference implementation) for seal / open.
#include "record_route.hpp"
#include "stream_common.hpp"
#include "stream_map.hpp"

namespace enet {

static_assert(kMapLanes == kStreamLanes && kMapRun == kRun, "stream_map.hpp and the streaming kernel disagree");

// Memory-wave schedule, in keystream barrier positions (an op at position k runs between barriers
// k-1 and k; a step is ~276 shader cycles of compute, a 1 KiB DMA or store costs its memory
// wave ~100-140 cycles to issue, so no position carries more than one of them -- two pushed
// every fourth step to ~660 cycles, holding all 12 waves at the barrier: tools/stream_probe.py
// trace): DMA d (0..15) at position dA + dE d, store s (0..15) at sA + sE s.
struct StreamSched {
    int dA, dE, sA, sE;
};
// 0 (default): DMA 1 + 3d, store 2 + 3s; tuning variants (ENET_STREAM_VAR, C2 shape) 1: 1 + 2d /
// 2 + 2s, 2: 1 + 4d / 3 + 4s, 3: 1 + d / 18 + 3s; 4 / 5: keystream barriers every 2 / 4 steps
// (38 / 19 positions), DMA 1 + 2d / 1 + d, store 2 + 2s / 1 + s (same position, after the DMA).
// C2 seal kernel in the bench's alternating pattern (tools/stream_probe.py --alt), us:
// 133 / 138 / 132 / 134 / 143 / 147 -- coarser barriers lose more lockstep pairing than they
// give the memory waves.  Layout probes that did not help: rotating each wave's stage order
// (arena offsets in flight differing in their low bits) 122 vs 124 us ChaCha20-only; lane j of
// a record owning runs j, j + P, ... (P lanes read 128 P contiguous bytes per stage) 154 vs 122.
__device__ constexpr StreamSched stream_sched(int v) {
    return v == 1 ? StreamSched{1, 2, 2, 2} : v == 2 ? StreamSched{1, 4, 3, 4}
         : v == 3 ? StreamSched{1, 1, 18, 3} : v == 4 ? StreamSched{1, 2, 2, 2}
         : v == 5 ? StreamSched{1, 1, 1, 1} : StreamSched{1, 3, 2, 3};
}
__device__ constexpr int stream_barf(int v) { return v == 4 ? 2 : v == 5 ? 4 : 1; }
// Issue priority of the waves and the place of open's Poly1305.  One s_setprio per wave before its
// stage loop, never flipped inside it.  Compute waves w, w + 4 and memory wave w + 8 share a SIMD,
// 0-3 in its wave slot 0, 4-7 dispatched second, the memory waves third (tools/simd_map.py,
// profiles/stream_simd_map.json).
//   prio_old / prio_young: compute waves 0-3 / 4-7; prio_mem: the memory waves
//   poly (open only): 0 where the compiler puts it -- open's ciphertext is in registers before the
//   keystream, and 57 of a stage's 152 v_mad_u64_u32 land in the first barrier interval, 3-4 in
//   each of sixteen later ones; 1 pinned behind the last keystream barrier, as seal's is by its
//   data; 2 / 3 spread over the 76 intervals (PolySpreadHook) behind each step's rotates / behind
//   each step's barrier
// Numbers (ENET_STREAM_VAR in the tools build, C2 shape): 20 + k: priorities k & 3 = 0 young 1,
// 1 old 1, 2 both 1, 3 both 2; memory waves 3 (k < 4) or 2; 30 / 31 / 32: poly 1 / 2 / 3.
// The default kernel (every lane count; the memory schedule variants too) runs number
// ENET_STREAM_ISSUE = 30: C2 bench 948.7 -> 960.4 GiB/s against 0; no priority setting moved it
// (944-951), 31 gave 957.9, 32 929.8 (profiles/stream_issue_screen.jsonl).
// -DENET_STREAM_ISSUE=n builds a candidate library for an A/B through bench.py
// (tools/stream_issue_ab.sh); the placements are compared that way, since the tools build's
// probe branches keep the compiler from moving open's Poly1305 and 0 compiles there as 1 does.
#ifndef ENET_STREAM_ISSUE
#define ENET_STREAM_ISSUE 30
#endif
struct StreamIssue {
    int prio_old, prio_young, prio_mem, poly;
};
__device__ constexpr StreamIssue stream_issue(int v) {
    int k = -1, poly = 0;
    if (v >= 20 && v < 28) k = v - 20;
    else if (v >= 30 && v <= 32) poly = v - 29;
    if (k < 0) return StreamIssue{0, 0, 3, poly};
    const int c = k & 3;
    return StreamIssue{c == 0 ? 0 : c == 3 ? 2 : 1, c == 1 ? 0 : c == 3 ? 2 : 1, (k & 4) ? 2 : 3, poly};
}
// stores issued at or after the last DMA's position (a store shares a position only after the DMA)
__device__ constexpr int stream_stores_after(StreamSched sc) {
    int n = 0;
    for (int s = 0; s < 16; ++s) n += (sc.sA + sc.sE * s >= sc.dA + 15 * sc.dE) ? 1 : 0;
    return n;
}

// probe (dbg 32768): wave w of the workgroup writes {entry shader clock, HW_ID, w} into 16 bytes
// at 16 w of the workgroup's tag slots (12 waves = 192 of its (512 >> LOGP) * 16 >= 512 bytes)
__device__ __forceinline__ void stream_where(const RecParams& p, int logp, uint32_t wave, uint32_t lane,
                                             uint64_t t_entry) {
    if (lane != 0 || !p.tag_out) return;
    const uint32_t hw = __builtin_amdgcn_s_getreg(4 | (31 << 11));  // HW_REG_HW_ID, bits 0..31
    uint32_t* d = reinterpret_cast<uint32_t*>(p.tag_out + 16ull * ((blockIdx.x * kStreamLanes) >> logp) + 16u * wave);
    d[0] = (uint32_t)t_entry; d[1] = (uint32_t)(t_entry >> 32); d[2] = hw; d[3] = wave;
}

template <int LOGP, int MODE, int SCHED = 0>
__global__ __launch_bounds__(kStreamWG) void stream_kernel(RecParams p) {
    constexpr StreamSched SC = stream_sched(SCHED);
    constexpr int BARF = stream_barf(SCHED);       // keystream steps per barrier
    constexpr int kPos = kStreamSteps / BARF;      // barrier positions per stage
    constexpr uint32_t P = 1u << LOGP;
    constexpr bool kPoly = (MODE != MODE_XOR);
    constexpr StreamIssue ISS = stream_issue(SCHED < 20 ? ENET_STREAM_ISSUE : SCHED);
    // input slab (DMA landing, read by the compute waves) and output slab (written by the compute
    // waves, stored by the memory waves); wave w's part is 8 KiB at 8 KiB w
    __shared__ __attribute__((aligned(16))) uint8_t s_in[kStreamLanes * kRun];
    __shared__ __attribute__((aligned(16))) uint8_t s_out[kStreamLanes * kRun];
    // what the lanes of a record hand each other (AEAD, P > 1), record q of the workgroup's R:
    // its leader's clamped r for the other lanes (written before S0(0), read after it), every
    // other lane's scaled Poly1305 limbs for the leader (limb i of thread t at 512 i + t; before
    // F1, after it), the leader's verdict for the tamper zeroing (open; before F2, after it)
    constexpr uint32_t kRecs = kStreamLanes >> LOGP;  // R
    constexpr bool kXch = kPoly && P > 1;
    __shared__ uint4 s_r[kXch ? kRecs : 1];
    __shared__ uint32_t s_limb[kXch ? 5 * kStreamLanes : 1];
    __shared__ uint32_t s_bad[kXch && MODE == MODE_OPEN ? kRecs : 1];

    const uint32_t L = (uint32_t)p.uniform_len;
    const bool compute = threadIdx.x < kStreamLanes;
    // the launch covers records [0, n), n = whole workgroups; lane j of every record sits in wave
    // group j (stream_map.hpp), j == 0 is the record's leader
    const StreamLane me = stream_lane(LOGP, blockIdx.x, compute ? threadIdx.x : 0u);
    const uint32_t rec = me.rec;
    // probe (dbg 16384, tools/stage_probe.py): compute wave 0 stamps the 100 MHz clock and the
    // shader clock at entry, the shader clock at the body start, after every stage barrier S0 and
    // after F1, and both clocks at exit, into the workgroup's tag slots
#ifdef ENET_TOOLS_BUILD
    const int dbg = p.dbg;
#else
    // the shipping build compiles the probes out: a runtime probe branch around the keystream made
    // the compiler route the state through PHI copies (~50 extra v_mov per stage)
    constexpr int dbg = 0;
#endif
    const bool stamp = (dbg & 16384) && threadIdx.x == 0 && p.tag_out;
    // probe (dbg 32768, tools/simd_map.py): every wave notes the shader clock at entry and its
    // HW_ID (wave slot, SIMD, CU) and writes both into the workgroup's tag slots at exit
    uint64_t t_entry = 0;
    if (__builtin_expect(dbg & 32768, 0)) t_entry = __builtin_amdgcn_s_memtime();
    uint64_t* stamps = reinterpret_cast<uint64_t*>(p.tag_out + 16ull * rec);
    if (__builtin_expect(stamp, 0)) {
        stamps[0] = __builtin_amdgcn_s_memrealtime();
        stamps[1] = __builtin_amdgcn_s_memtime();
    }
    const uint64_t i0 = p.in_off[0], o0 = p.out_off[0];
    {
        const bool mine = !compute || (p.in_off[rec] == i0 + (uint64_t)rec * L &&
                                       p.in_off[rec + 1] == i0 + (uint64_t)(rec + 1) * L &&
                                       p.out_off[rec] == o0 + (uint64_t)rec * L &&
                                       p.out_off[rec + 1] == o0 + (uint64_t)(rec + 1) * L);
        if (!__syncthreads_and(mine ? 1 : 0)) {
            if (compute) records_body<LOGP, MODE, FR_NONE, 7>(p);
            return;
        }
    }

    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the record-lane, taken from the wave's first thread where a wave holds one value of it
    // (P <= 8): a scalar, so whole waves branch around what only some lane of a record does
    const uint32_t j = P == 1 ? 0u : LOGP <= 3 ? stream_lane(LOGP, blockIdx.x, 64u * wave).j : me.j;
    const uint32_t B = L >> (6 + LOGP);  // blocks per lane (the host launches L % (128 P) == 0)
    const uint32_t S = B >> 1;           // stages
    const bool mem = !(dbg & 1);

    if (!compute) {
        // ================================================================ memory waves
        // Memory wave m serves compute waves 2m and 2m+1.  Instruction i of compute wave c moves
        // 16-byte chunk kk ^ sw(o) of its owner o = 8i + lane/8, thread 64c + o of the workgroup.
        // 32-bit offsets from the arena bases: the host launches this kernel only for arenas
        // < 4 GiB.
        const uint32_t m = wave - 8u;
        const uint32_t kk = lane & 7u;
        // the memory waves win issue arbitration: their one instruction per keystream barrier
        // interval then never waits behind the compute waves' VALU stream (C2: +1-2 %,
        // tools/prio_ab.sh 876/879/889 -> 893/896/899 GiB/s on one box)
        if (!(dbg & 4096)) __builtin_amdgcn_s_setprio(ISS.prio_mem);
        // every slot's lane offset precomputed (16 VGPRs): a memory wave shares its SIMD with two
        // compute waves that keep the VALU saturated, so each VALU instruction it issues waits for
        // a slot -- the address arithmetic of a store (~10 VALU) held it ~300 cycles past the
        // next barrier (tools/stream_probe.py trace).  Slots are SALU + VMEM / LDS only.
        // The owner's record and record-lane come from the map the compute waves use
        // (stream_map.hpp; consecutive owners are consecutive records, L bytes apart).
        uint32_t offs[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const uint32_t t = stream_mem_owner(m, s, lane);
            offs[s] = stream_lane_offset(LOGP, L, stream_lane(LOGP, blockIdx.x, t)) + 16u * (kk ^ slab_sw(t & 63u));
        }
        // the arena bases are SGPR operands of the DMA / store asm: keep them provably uniform
        auto uni = [](const void* q) {
            const uint64_t v = reinterpret_cast<uintptr_t>(q);
            // (readfirstlane returns int: zero-extend, a sign-extended low half corrupts the address)
            return (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)v) |
                   ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32);
        };
        const uint8_t* ibase = reinterpret_cast<const uint8_t*>(uni(p.in + i0));
        uint8_t* obase = reinterpret_cast<uint8_t*>(uni(p.out + o0));
        // this wave's parts of the slabs: compute waves 2m and 2m+1, adjacent
        const uint32_t in_part = (uint32_t)reinterpret_cast<uintptr_t>(s_in) + 2u * m * (64u * kRun);
        const uint8_t* out_part = s_out + 2u * m * (64u * kRun) + 16u * lane;
        // op s (0..15) = instruction s & 7 of compute wave 2m + (s >> 3): 1 KiB group 1024 s of
        // the part.  The DMA is issued from inline asm (M0 saved and restored in the statement):
        // the compiler then sees no LDS DMA and puts no vmcnt wait in front of the LDS reads it
        // cannot prove disjoint from the landing slab; the landing is awaited explicitly before
        // the stage barrier.
        auto dma = [&](const uint8_t* base, int s) {
            const uint32_t m0 = in_part + 1024u * (uint32_t)s;
            uint32_t keep;
            // non-temporal: every input line is read exactly once (C2: +1.2 %, three interleaved
            // pairs, tools/stagger_ab.sh "0 14"; SCHED 14 = plain loads for the A/B)
            if constexpr (SCHED == 14)
                asm volatile("s_mov_b32 %0, m0\n s_mov_b32 m0, %2\n s_nop 0\n global_load_lds_dwordx4 %1, %3\n s_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(offs[s]), "s"(m0), "s"(base) : "memory");
            else
                asm volatile("s_mov_b32 %0, m0\n s_mov_b32 m0, %2\n s_nop 0\n global_load_lds_dwordx4 %1, %3 nt\n s_mov_b32 m0, %0"
                             : "=&s"(keep) : "v"(offs[s]), "s"(m0), "s"(base) : "memory");
        };
        auto ldsread = [&](int s) {
            return *reinterpret_cast<const uint4*>(out_part + 1024u * (uint32_t)s);
        };
        // whole non-temporal lines, SGPR base + VGPR offset: no VALU in the slot (a 64-bit address
        // add waited for a VALU issue slot behind the compute waves).  From inline asm, so the
        // store is absent from the compiler's vmcnt bookkeeping: the stage-end waits count it.
        auto store = [&](uint8_t* base, int s, uint4 v) {
            enet_u32x4 d = {v.x, v.y, v.z, v.w};
            asm volatile("global_store_dwordx4 %0, %1, %2 nt\n s_nop 1"
                         :: "v"(offs[s]), "v"(d), "s"(base) : "memory");
        };
        uint64_t wait_cyc = 0;
        if (mem) {
#pragma unroll
            for (int s = 0; s < 16; ++s) dma(ibase, s);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        for (uint32_t st = 0; st < S; ++st) {
            stream_barrier();  // S0(st): stage st landed; stage st-1's outputs in the output slab
            const bool more = mem && st + 1 < S && !(dbg & 128), prev = mem && st > 0 && !(dbg & 64);
            const uint8_t* inext = ibase + (size_t)kRun * (st + 1);
            uint8_t* oprev = obase + (size_t)kRun * (st - 1);
            uint4 v = make_uint4(0, 0, 0, 0);
            if (__builtin_expect(prev, 1)) v = ldsread(0);
#pragma unroll
            for (int k = 0; k < kPos; ++k) {
                if (k >= SC.dA && (k - SC.dA) % SC.dE == 0 && (k - SC.dA) / SC.dE < 16) {
                    // the compute waves read their runs before barrier 0
                    if (__builtin_expect(more, 1)) dma(inext, (k - SC.dA) / SC.dE);
                }
                if (k >= SC.sA && (k - SC.sA) % SC.sE == 0 && (k - SC.sA) / SC.sE < 16) {
                    const int sl = (k - SC.sA) / SC.sE;
                    if (__builtin_expect(prev, 1)) {
                        store(oprev, sl, v);  // (waits for its LDS read)
                        if (sl < 15) v = ldsread(sl + 1);
                    }
                }
                stream_barrier();
            }
            // the next stage has landed: the stores issued after the last DMA may still be in
            // flight (vmcnt retires in issue order)
            constexpr int kStoresAfter = stream_stores_after(SC);
            uint64_t tw0 = 0;
            if (__builtin_expect(dbg & 2048, 0)) tw0 = __builtin_amdgcn_s_memtime();
            if (__builtin_expect(prev, 1)) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(kStoresAfter) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (__builtin_expect(dbg & 2048, 0)) wait_cyc += __builtin_amdgcn_s_memtime() - tw0;
        }
        if (__builtin_expect(dbg & 2048, 0) && lane == 0 && p.tag_out)  // probe: stage-end DMA waits
            reinterpret_cast<uint64_t*>(p.tag_out)[blockIdx.x * 4u + m] = wait_cyc;
        stream_barrier();  // F1: the last stage's outputs are in slab (S-1) & 1
        if (S > 0 && mem) {
            uint8_t* olast = obase + (size_t)kRun * (S - 1);
#pragma unroll
            for (int s = 0; s < 16; ++s) store(olast, s, ldsread(s));
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every store done (tamper zeroing)
        stream_barrier();  // F2
        if (__builtin_expect(dbg & 32768, 0)) stream_where(p, LOGP, wave, lane, t_entry);
        return;
    }

    // ==================================================================== compute waves
    const uint32_t msw = slab_sw(lane);
    if (__builtin_expect(stamp, 0)) stamps[2] = __builtin_amdgcn_s_memtime();

    // ---- per-record ChaCha20 constants
    uint32_t kw[8], nw[3];
    {
        const uint32_t* kp = reinterpret_cast<const uint32_t*>(p.keys + (size_t)p.key_stride * rec);
#pragma unroll
        for (int i = 0; i < 8; ++i) kw[i] = kp[i];
        const uint32_t* np = reinterpret_cast<const uint32_t*>(p.nonces + 12ull * rec);
#pragma unroll
        for (int i = 0; i < 3; ++i) nw[i] = np[i];
    }
    ChachaRecord R;
    chacha_record_init(R, kw, nw);
    uint32_t ctr = 1u;  // RFC 8439 data counter
    if (MODE == MODE_XOR)  // reference ChaCha20::apply start counter (0 when not given)
        ctr = p.counters ? p.counters[(size_t)rec * (p.counter_stride ? p.counter_stride : 1u)] : 0u;
    ctr += j * B;  // this lane's first block (u32 wrap, ChaCha20.cpp:110)

    uint64_t clk0 = 0, rt0 = 0;
    if (dbg & 256) {  // clock probe: shader cycles and 100 MHz ticks around the whole body
        clk0 = __builtin_amdgcn_s_memtime();
        rt0 = __builtin_amdgcn_s_memrealtime();
    }

    // ---- Poly1305: the record's leader makes the one-time key from block 0 (while stage 0 lands),
    // hands r to the record's other lanes and absorbs the AAD; waves without a leader go straight
    // to the stage barrier
    uint32_t h[5] = {0, 0, 0, 0, 0};
    PolyR32 PR{};
    uint32_t pad[4] = {0, 0, 0, 0};
    uint32_t na = 0, aad_len = 0;
    const uint32_t q = threadIdx.x & (kRecs - 1u);  // the record's place in the workgroup
    if (kPoly) {
        uint64_t aoff = 0;
        if (p.aad) {
            aoff = p.aad_off[rec];
            aad_len = (uint32_t)(p.aad_off[rec + 1] - aoff);
        }
        na = (aad_len + 15) >> 4;
        if (j == 0) {
            uint32_t otk[16];
            chacha_block(R, 0u, otk);
            PR = polyr32_make(otk[0], otk[1], otk[2], otk[3]);
            pad[0] = otk[4]; pad[1] = otk[5]; pad[2] = otk[6]; pad[3] = otk[7];
            if (kXch) s_r[q] = make_uint4(PR.r0, PR.r1, PR.r2, PR.r3);
            for (uint32_t s = 0; s < na; ++s) {
                const uint8_t* ap = p.aad + aoff + 16ull * s;
                const uint32_t cnt = min(16u, aad_len - 16u * s);
                uint32_t w[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    uint32_t v = 0;
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if ((uint32_t)(4 * i + b) < cnt) v |= (uint32_t)ap[4 * i + b] << (8 * b);
                    w[i] = v;
                }
                poly32_block(h, PR, w[0], w[1], w[2], w[3], 1u);
            }
        }
    }

    const uint32_t ff[16] = {kSigma0, kSigma1, kSigma2, kSigma3, R.k[0], R.k[1], R.k[2], R.k[3],
                             R.k[4], R.k[5], R.k[6], R.k[7], 0u, R.n[0], R.n[1], R.n[2]};
    if constexpr (ISS.prio_old == ISS.prio_young) {
        if constexpr (ISS.prio_old != 0) __builtin_amdgcn_s_setprio(ISS.prio_old);
    } else if (wave >= 4u) {
        if constexpr (ISS.prio_young != 0) __builtin_amdgcn_s_setprio(ISS.prio_young);
    } else {
        if constexpr (ISS.prio_old != 0) __builtin_amdgcn_s_setprio(ISS.prio_old);
    }
    // S0(0): the memory waves saw stage 0 land; the leaders' r is in the exchange
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    stream_barrier();
    if (__builtin_expect(stamp, 0)) stamps[3] = __builtin_amdgcn_s_memtime();
    if (kXch && j != 0) {
        const uint4 r = s_r[q];
        PR = polyr32_make(r.x, r.y, r.z, r.w);
    }
    for (uint32_t st = 0;;) {  // (S >= 1: the host launches L >= 128 P)
        uint8_t* myrun = s_in + threadIdx.x * kRun;
        // the run is read now and consumed after the keystream, so its LDS latency is hidden
        uint32_t w[32];
        if (__builtin_expect(dbg & 32, 0)) {  // probe: no LDS traffic in the compute waves
#pragma unroll
            for (int k = 0; k < 32; ++k) w[k] = k * lane + st;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint4 v = *reinterpret_cast<const uint4*>(myrun + 16u * (k ^ msw));
                w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
            }
        }
        const uint32_t c0 = ctr + 2u * st;
        uint32_t x[32];
        {
            uint32_t a0 = kSigma0, a4 = R.k[0], a8 = R.k[4], a12 = c0;
            uint32_t b0 = kSigma0, b4 = R.k[0], b8 = R.k[4], b12 = c0 + 1u;
            ENET_QR(a0, a4, a8, a12);
            ENET_QR(b0, b4, b8, b12);
            x[0] = a0; x[4] = a4; x[8] = a8; x[12] = a12;
            x[16] = b0; x[20] = b4; x[24] = b8; x[28] = b12;
#pragma unroll
            for (int c = 1; c < 4; ++c) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    x[c + 4 * r] = R.pre[4 * (c - 1) + r];
                    x[16 + c + 4 * r] = R.pre[4 * (c - 1) + r];
                }
            }
        }
        // the input run is in registers before keystream barrier 0: the slab may be refilled
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (__builtin_expect(dbg & 2, 0)) {  // probe: no keystream, the barriers only
#pragma unroll
            for (int k = 0; k < kPos; ++k) stream_barrier();
        } else if constexpr (MODE == MODE_OPEN && ISS.poly >= 2) {
            // the hook of poly 2 issues the step's barrier itself, behind its piece
            using Hook = PolySpreadHook<ISS.poly == 2>;
            constexpr int HB = ISS.poly == 2 ? 0 : 1;
            Hook hook(h, PR, w);
            chacha_half_lockstep2<true, Hook&, HB, 0>(x, hook);
            [&]<int... DR>(std::integer_sequence<int, DR...>) {  // double rounds 1..9, steps 4..75
                ((chacha_half_lockstep2<false, Hook&, HB, 8 * DR + 4>(x, hook),
                  chacha_half_lockstep2<true, Hook&, HB, 8 * DR + 8>(x, hook)), ...);
            }(std::make_integer_sequence<int, 9>{});
        } else {
            chacha_half_lockstep2<true, NoStepHook, BARF>(x);
#pragma unroll
            for (int dr = 1; dr < 10; ++dr) {
                chacha_half_lockstep2<false, NoStepHook, BARF>(x);
                chacha_half_lockstep2<true, NoStepHook, BARF>(x);
            }
        }
        if constexpr (MODE == MODE_OPEN && ISS.poly == 1) {
            // the ciphertext is held behind the last keystream barrier: Poly1305 runs after it
#pragma unroll
            for (int i = 0; i < 32; ++i) ENET_PIN(w[i]);
        }
        if (MODE == MODE_OPEN && ISS.poly < 2 && !(dbg & 4)) {
            poly_block64(h, PR, w);
            poly_block64(h, PR, w + 16);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            w[i] ^= x[i] + (i == 12 ? c0 : ff[i]);
            w[16 + i] ^= x[16 + i] + (i == 12 ? c0 + 1u : ff[i]);
        }
        if (MODE == MODE_SEAL && !(dbg & 4)) {
            poly_block64(h, PR, w);
            poly_block64(h, PR, w + 16);
        }
        // outputs into the own run of the output slab (the memory waves have read its previous
        // contents out by now)
        uint8_t* myout = s_out + threadIdx.x * kRun;
        if (__builtin_expect(dbg & 32, 0)) {
            uint32_t acc = 0;
#pragma unroll
            for (int k = 0; k < 32; ++k) acc ^= w[k];
            if (acc == 0x9e3779b9u) myout[0] = 1;
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                *reinterpret_cast<uint4*>(myout + 16u * (k ^ msw)) =
                    make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
        }
        if (kPoly) {
            // the stage's Poly1305 stays in front of the stage barrier (with the loop's exit in its
            // middle the compiler moved seal's behind it, between S0 and keystream barrier 0)
#pragma unroll
            for (int i = 0; i < 5; ++i) ENET_PIN(h[i]);
        }
        if (++st == S) break;
        // S0(st): the memory waves saw stage st land; this wave's output writes are done
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        stream_barrier();
        if (__builtin_expect(stamp, 0)) stamps[3 + st] = __builtin_amdgcn_s_memtime();
    }
    // ---- Poly1305 tail, the part of every lane: the length block LE64(|aad|) || LE64(|ct|) in the
    // record's last lane; every other lane scales its sum by r^e, e = N-1-s_last (the last wave
    // group skips the power), and hands the leader its limbs
    uint32_t l[5] = {0, 0, 0, 0, 0};
    if (kPoly) {
        const uint32_t nct = L >> 4;
        const uint32_t N = na + nct + 1;
        if (j == P - 1) poly32_block(h, PR, aad_len, 0u, L, 0u, 1u);
        h32_to_limbs(h, l);
        if (j != P - 1) {
            const uint32_t e = N - 1 - (na + 4 * (j + 1) * B - 1);  // >= 4 B + 1
            uint32_t r26[5], xx[5];
            plimbs(r26, PR.r0, PR.r1, PR.r2, PR.r3);
            ppow(r26, e, xx);
            pmul(l, pmul_make(xx));
        }
        if (kXch && j != 0) {
#pragma unroll
            for (int i = 0; i < 5; ++i) s_limb[kStreamLanes * i + threadIdx.x] = l[i];
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    stream_barrier();  // F1
    if (__builtin_expect(stamp, 0)) stamps[3 + S] = __builtin_amdgcn_s_memtime();

    if (dbg & (256 | 2048 | 16384 | 32768)) {  // 4 words at the workgroup's first tag slot: clk0, rt0, clk1, rt1
        const uint64_t clk1 = __builtin_amdgcn_s_memtime(), rt1 = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0 && p.tag_out && !(dbg & (2048 | 16384 | 32768))) {
            uint64_t* d = reinterpret_cast<uint64_t*>(p.tag_out + 16ull * rec);
            d[0] = clk0; d[1] = rt0; d[2] = clk1; d[3] = rt1;
        }
        stream_barrier();  // F2
        if (__builtin_expect(stamp, 0)) {
            stamps[4 + S] = __builtin_amdgcn_s_memtime();
            stamps[5 + S] = __builtin_amdgcn_s_memrealtime();
        }
        if (dbg & 32768) stream_where(p, LOGP, wave, lane, t_entry);
        return;
    }
    uint32_t diff = 0;
    if (kPoly) {
        // the leader's part: the sum of the record's lanes, the tag, and for open the verdict,
        // handed to the record's other lanes across F2
        if (j == 0) {
            if (kXch) {
#pragma unroll
                for (uint32_t jj = 1; jj < P; ++jj) {
#pragma unroll
                    for (int i = 0; i < 5; ++i) l[i] += s_limb[kStreamLanes * i + stream_thread(LOGP, q, jj)];
                }
            }
            uint32_t tag[4];
            pfinish(l, pad, tag);
            if (MODE == MODE_SEAL) {
                uint32_t* tp = reinterpret_cast<uint32_t*>(p.tag_out + 16ull * rec);
                tp[0] = tag[0]; tp[1] = tag[1]; tp[2] = tag[2]; tp[3] = tag[3];
            } else {
                const uint32_t* tp = reinterpret_cast<const uint32_t*>(p.tag_in + 16ull * rec);
                diff = (tag[0] ^ tp[0]) | (tag[1] ^ tp[1]) | (tag[2] ^ tp[2]) | (tag[3] ^ tp[3]);
                p.ok[rec] = diff == 0 ? 1 : 0;
                if (kXch) s_bad[q] = diff;
            }
        }
        if (kXch && MODE == MODE_OPEN) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
    stream_barrier();  // F2: the memory waves' stores of this workgroup are complete
    if (kXch && MODE == MODE_OPEN && j != 0) diff = s_bad[q];
    if (MODE == MODE_OPEN && diff != 0) {
        // authentication failed: do not release plaintext
        uint8_t* seg = p.out + o0 + (uint64_t)rec * L + ((uint64_t)j * B << 6);
        for (uint32_t c = 0; c < 4 * B; ++c)
            *reinterpret_cast<uint4*>(seg + 16ull * c) = make_uint4(0, 0, 0, 0);
    }
}

// seal and xor have no placement variants
template <int MODE>
constexpr int stream_issue_var(int v) {
    return (MODE == MODE_OPEN || v < 30) ? v : 0;
}

template <int MODE>
static hipError_t launch_stream_mode(const RecParams& p, uint32_t lanes, uint32_t blocks, hipStream_t s) {
    switch (lanes) {
        case 1: hipLaunchKernelGGL((stream_kernel<0, MODE>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
        case 2:
#ifdef ENET_TOOLS_BUILD
            // memory schedule variants of the C2 shape (ENET_STREAM_VAR, tools build)
            switch (p.var) {
                case 1: hipLaunchKernelGGL((stream_kernel<1, MODE, 1>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
                case 2: hipLaunchKernelGGL((stream_kernel<1, MODE, 2>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
                case 3: hipLaunchKernelGGL((stream_kernel<1, MODE, 3>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
                case 4: hipLaunchKernelGGL((stream_kernel<1, MODE, 4>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
                case 5: hipLaunchKernelGGL((stream_kernel<1, MODE, 5>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
                case 14: hipLaunchKernelGGL((stream_kernel<1, MODE, 14>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
#define ENET_VAR(V) case V: hipLaunchKernelGGL((stream_kernel<1, MODE, stream_issue_var<MODE>(V)>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
                ENET_VAR(20) ENET_VAR(21) ENET_VAR(22) ENET_VAR(23) ENET_VAR(24) ENET_VAR(25) ENET_VAR(26) ENET_VAR(27)
                ENET_VAR(30) ENET_VAR(31) ENET_VAR(32)
#undef ENET_VAR
                default: hipLaunchKernelGGL((stream_kernel<1, MODE>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
            }
#else
            hipLaunchKernelGGL((stream_kernel<1, MODE>), dim3(blocks), dim3(kStreamWG), 0, s, p);
#endif
            break;
        case 4: hipLaunchKernelGGL((stream_kernel<2, MODE>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
        case 8: hipLaunchKernelGGL((stream_kernel<3, MODE>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
        case 16: hipLaunchKernelGGL((stream_kernel<4, MODE>), dim3(blocks), dim3(kStreamWG), 0, s, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// which batches come here: record_route.hpp choose_record_route (RecordKind::Stream)
static_assert(kRouteWideWG == kStreamLanes, "record_route.hpp and the streaming kernel disagree on the workgroup");

hipError_t launch_stream(int mode, const RecParams& p, uint32_t lanes, uint32_t blocks, hipStream_t s) {
    switch (mode) {
        case MODE_XOR: return launch_stream_mode<MODE_XOR>(p, lanes, blocks, s);
        case MODE_SEAL: return launch_stream_mode<MODE_SEAL>(p, lanes, blocks, s);
        case MODE_OPEN: return launch_stream_mode<MODE_OPEN>(p, lanes, blocks, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace enet
