"""Rebuild profiles/README.md: one row per evidence file that the docs cite (DESIGN.md,
INTEGRATION.md, README.md, DESIGN_HISTORY.md, bench.py), with the citing documents; descriptions
kept from the previous README where it had one, else from DESC below.  Files no document cites
move to profiles/archive/ (git mv).  usage: python tools/profiles_index.py [--move]"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = os.path.join(ROOT, "profiles")
DOCS = ["DESIGN.md", "INTEGRATION.md", "README.md", "DESIGN_HISTORY.md", "bench.py"]
# source files whose comments cite evidence (file:line of the measurement behind a choice)
CODE_DIRS = ["ephemeralnet_amd", "include", "tests", "tools", "oracle"]
CODE_EXT = (".cpp", ".hpp", ".h", ".hip", ".py", ".c", ".sh")

DESC = {
    "r05_seal_variants.jsonl": "host engine frame seal / open, stitched vs two-pass, by size (tools/seal_variants, EPYC 9575F)",
    "r05_seal_bench.jsonl": "enet_host_seal_body vs HMAC then ChaCha20 over the C ABI (tools/seal_bench)",
    "r05_seal_cpu.txt": "the box's CPU model for the seal measurements",
    "r05_seal_host_queue.jsonl": "queue bench, host engine rows (blocking 1 / 16 threads, 16 x 256 views) with the stitched seal / open",
    "r05_seal_queue_bench.jsonl": "queue bench, every form, with the stitched host engine (two rounds)",
    "r05_seal_auto_routing.jsonl": "AUTO vs host vs device by in-flight count, stitched host engine, backlog threshold 192",
    "r05_seal_auto_routing_320.jsonl": "the same with the threshold at 320",
    "r05_seal_auto_long_legs.jsonl": "AUTO vs device at 16 x 1 024, 0.8 s and 3 s legs (AUTO's gap is the device path's cold start)",
    "r05_hmac_regs_ab.jsonl": "seal_variants, register-resident HMAC vs the streaming-state HMAC, two runs each",
    "r05_hmac_scalar_latency_auto.jsonl": "scalar-signature latency, policy auto, register-resident HMAC",
    "r05_queue_inflight.jsonl": "device queue by device passes in flight (4 / 8 / 16) x 128 / 256 / 1 024 frames in flight, two rounds",
    "r05_queue_inflight_hwq16.jsonl": "the same at 256 / 1 024 with GPU_MAX_HW_QUEUES=16",
    "r05_queue_stage_ab.jsonl": "device queue passes staged in device memory vs zero-copy, forced (tools build), 16 x 128 / 256 / 1 024, two rounds",
    "r05_queue_stage_stress.txt": "byte-checked window stress run with every pass staged",
    "r05_queue_stage_queue_bench.jsonl": "queue bench, every form, with passes of >= 768 frames staged (two rounds)",
    "r05_queue_stage_pytest.log": "pytest -m gpu of the queue tests with the staged passes",
    "r05_queue_stage_crossover.jsonl": "device queue with staged large passes, 16 threads x 256-768 in flight, two rounds",
    "r05_queue_w8_pytest.log": "pytest -m gpu of the queue and C++ API tests with 8 device passes in flight",
    "r05_queue_w8_queue_bench.jsonl": "queue bench, every form, staged large passes and 8 passes in flight (two rounds)",
    "r05_queue_w8_auto_routing.jsonl": "AUTO vs host vs device by in-flight count with staged passes and 8 in flight",
    "r05_queue_stage_inflight.jsonl": "staged queue by device passes in flight (4 / 8 / 16) x 512 / 1 024 in flight",
    "r05_b3_bench.json": "default bench line with the queue leg's device_1024 key (staged passes, 8 in flight)",
    "r05_v2_pytest_gpu.log": "pytest -m gpu, full suite, staged queue passes and 8 in flight",
    "r05_v2_smoke.log": "smoke() on the same tree",
    "r05_v2_bench.json": "default bench line on the same tree",
    "r05_queue_stage_ab_w8.jsonl": "staged vs zero-copy forced at 8 passes in flight, 16 x 256 / 384 / 512, two rounds",
    "r05_queue_thr_queue_bench.jsonl": "queue bench, every form, staging from 640 frames sealing / 512 opening, 8 passes in flight",
    "r05_queue_thr_crossover.jsonl": "device queue at 256 / 384 / 512 in flight with that rule, two rounds",
    "r05_queue_thr_auto_routing.jsonl": "AUTO vs host vs device with that rule",
    "r05_v3_pytest_gpu.log": "pytest -m gpu, full suite, final tree (per-direction staging rule)",
    "r05_v3_smoke.log": "smoke() on the final tree",
    "r05_v3_bench.json": "default bench line on the final tree",
    "r05_queue_stage_out_ab.jsonl": "staged passes with results staged in device memory and copied back (1) vs written into the pinned pass (0), 512 / 1 024 in flight, two rounds",
    "r05_queue_auto_warm.jsonl": "AUTO vs host vs device by in-flight count after an untimed warm-up leg each way (steady state)",
    "r05_b4_bench.json": "default bench line, queue side leg with its warm-up legs",
    "r05_v4_pytest_gpu.log": "pytest -m gpu, full suite, final tree",
    "r05_v4_smoke.log": "smoke() on the final tree",
    "r05_v4_bench.json": "default bench line on the final tree",
    "r05_seal_crossover_hi.jsonl": "device vs stitched host engine, 16 threads x 256-768 in flight, two rounds",
    "r05_seal_pytest_queue.log": "pytest -m gpu of the queue and C++ API tests with the 320 threshold",
    "r05_seal_scalar_latency_auto.jsonl": "scalar-signature latency, policy auto, after the stitched seal and explicit_bzero wipes",
    "r05_seal_verify_pytest_gpu.log": "pytest -m gpu, full suite, stitched host engine tree",
    "r05_seal_verify_bench.json": "default bench line on the same tree",
    "r05_seal_verify_smoke.log": "smoke() on the same tree",
    "r05_c3_persistent_ab.jsonl": "C3 persistent-workgroup kernel (2 WG/CU) vs the per-batch grid, three interleaved pairs",
    "r05_c3_persistent_1wg_ab.jsonl": "the same at 1 workgroup per CU (265-270 VGPRs)",
    "r05_numa_ab.jsonl": "C2 e2e and C5 share with staging on the GPU's node / the other node / where HIP puts it",
    "r05_numa_topology.txt": "the box's NUMA / CPU / cgroup facts behind the placement plan",
    "r05a_bench.json": "bench line, first round-5 box run",
    "r05a_batch_bench_c2.jsonl": "crypto::batch C2 from std::vector records: packed, fresh vectors, pinned",
    "r05a_batch_bench_c2_trace.txt": "ENET_HOST_TRACE of the fresh-vector C2 calls (gather / scatter bound)",
    "r05b_queue_bench_cas.jsonl": "frame queue with one shared reservation word: failed CAS per frame",
    "r05c_batch_bench.jsonl": "crypto::batch C2 / C3 wire: packed, fresh, reused vectors, pinned",
    "r05c_batch_bench_trace.txt": "ENET_HOST_TRACE of the reused-vector calls",
    "r05c_probe_trace_summary.txt": "rocprofv3 kernel + copy trace of the host pipeline on both HIP runtimes (blit-kernel D2H on torch's)",
    "r05c_queue_bench.jsonl": "frame queue, blocking-sync vs polling worker waits",
    "r05d_bench.json": "bench line with the copy-timing probe on both runtimes",
    "r05d_probe.jsonl": "copy-timing probe: D2H, H2D, both at once, D2H beside a busy kernel, both runtimes",
    "r05d_e2e_torch_modes.jsonl": "C2 e2e in a torch process per host mode (3 vs 4)",
    "r05d_queue_bench.jsonl": "frame queue, first round-5 design (slot records, polling)",
    "r05d_n2_rehearsal.json": "N = 2 torchrun rehearsal (gloo, one GPU): per-rank placement and C5 host share",
    "r05d_pytest_gpu.log": "pytest -m gpu",
    "r05e_probe_pipeline64.jsonl": "64 MiB pinned pipeline A/B per mode on both runtimes (no difference)",
    "r05e_queue_prof.jsonl": "queue bench under the per-phase profile (tools build)",
    "r05e_queue_prof.txt": "per-phase TSC profile of the first queue design",
    "r05f_mode_diag.jsonl": "C2 per host-buffer variant, modes 3 / 4, torch's runtime (tools/mode_diag.py)",
    "r05f_trace_torch_mode3.txt": "ENET_HOST_TRACE, torch's runtime, mode 3 (launch calls block)",
    "r05f_trace_torch_mode4.txt": "the same in mode 4",
    "r05f_queue_bench.jsonl": "queue with get(out) and the incremental release scan",
    "r05f_queue_prof.jsonl": "queue profile by shard placement (first A/B)",
    "r05f_queue_prof.txt": "per-phase profile: lock waits and reopen cost of the reference-counted design",
    "r05g_queue_bench.jsonl": "queue with generation-tagged slots and ticket-owned states",
    "r05g_queue_prof.txt": "per-phase profile of that design",
    "r05g_pytest_gpu.log": "pytest -m gpu",
    "r05h_bench.json": "bench line with the auto host mode on both runtimes",
    "r05h_queue_bench.jsonl": "queue with the per-thread state cache and streamed fills",
    "r05h_session_log.txt": "session log incl. the streamed vs plain fill profile",
    "r05i_queue_shards.jsonl": "queue shard placement A/B: 4 / 8 shards by thread order or L3 domain",
    "r05i_queue_shards_prof.txt": "per-phase profile of each shard placement",
    "r05j_bench.json": "bench line after the queue work (auto mode decisions and rates)",
    "r05j_queue_bench.jsonl": "final round-5 queue table (DESIGN §6)",
    "r05j_pytest_gpu.log": "pytest -m gpu",
    "r05k_queue_prof_release_split.txt": "per-phase profile with the release split, streamed vs plain fills",
    "r05l_queue_prof_prefetch.txt": "per-phase profile with result prefetch (dropped)",
    "r05l_queue_bench_prefetch.jsonl": "queue bench with result prefetch (dropped)",
    "r05m_c5_full.jsonl": "C5 host-resident at its full BASELINE size, arenas in place (block record first)",
    "r05m_pytest_host_topology.log": "host-topology GPU tests incl. the block past 4 GiB",
    "r05z_bench.json": "final round-5 default bench line (roofline, cpu_baseline, host_resident, power)",
    "r05z_bench_torchrun_n1.json": "the same through torch.distributed.run --nproc-per-node 1",
    "r05z_side.jsonl": "final round-5 side configs: C3, C4, xor, wire, store, PoW, e2e, C5 host / device",
    "r05z_pytest_gpu.log": "final round-5 pytest -m gpu",
    "r05z_smoke.log": "__graft_entry__.smoke() on the box",
    "r05z_c5_probe.json": "C5 device-resident chain probe (tools/c5_overlap_probe.py)",
    "r05z_scalar_latency_auto.jsonl": "scalar-signature latency, policy auto",
    "r05z_scalar_latency_device.jsonl": "scalar-signature latency, policy device",
    "r05z_scalar_latency_ref.jsonl": "the reference's own scalar calls (oracle/_ref)",
    "r05p_queue_bench_view.jsonl": "queue with zero-copy FrameTicket::view() vs get(out) vs the host engine",
    "r05p_pytest_queue.log": "frame-queue GPU tests with views",
    "r05o_pytest_gpu.log": "pytest -m gpu on the final tree (457 passed)",
    "r05o_pytest_queue.log": "frame-queue GPU tests, verbose: pass sizes, evictions, queue-bench test",
    "r05o_bench.json": "bench line on the final tree",
    "r05o_n2_rehearsal.json": "N = 2 torchrun rehearsal on the final tree",
    "r05q_queue_bench.jsonl": "queue with the worker's first sleep from its recent kernel time",
    "r05q_queue_kernel_stats.csv": "rocprofv3 --kernel-trace --stats of the queue bench (wire kernel per pass)",
    "r05q_queue_under_rocprof.json": "the queue bench line printed under that rocprofv3 run",
    "r05x_pytest_gpu.log": "pytest -m gpu on the final tree (457 passed)",
    "r05x_bench.json": "bench line on the final tree",
    "r05u_bench.json": "bench line on the final tree",
    "r05r_bench.json": "bench line on the final tree",
    "r05s_crossover.jsonl": "device queue vs host engine by threads x frames in flight (the AUTO crossover)",
    "r05t_auto_routing.jsonl": "AUTO routing by backlog vs device vs host, 16 threads x 16-1 024 in flight",
    "r05t_pytest_queue.log": "frame-queue GPU tests with backlog routing",
    "r05w_queue_bench_host_tail.jsonl": "frame queue host engine vs device after the host ChaCha20 tail went vector",
    "r05w_scalar_latency_auto.jsonl": "scalar-signature latency (policy auto) with the vector ChaCha20 tail",
    "frame_queue_split_ab.jsonl": "tools/queue_bench against the library before and after the frame_queue.cpp split, alternately, six pairs per case (device reuse 16 x 1 024, device view 16 x 256, host view 16 x 256, host sync 16)",
    "r05w_bench.json": "bench line incl. the frame_queue side leg",
    "r05y_bench_repeat_one_box.jsonl": "the default bench line five times on one box (value, kernel ms, power)",
    "r05z2_queue_bench_hmac_cache.jsonl": "frame queue host engine vs device with the HMAC pad cache",
    "r05z2_scalar_latency_auto.jsonl": "scalar-signature latency (policy auto) with both host-engine changes",
    "r05z2_pytest_gpu.log": "pytest -m gpu on the final tree (457 passed)",
    "r05z2_bench.json": "bench line incl. the frame_queue side leg (final tree)",
    "r05_final_pytest_gpu.log": "pytest -m gpu on the final tree (457 passed; tools/gpu_session.sh verify)",
    "r05_final_bench.json": "bench line on the final tree",
    "r05_final_queue_bench.jsonl": "every queue submission form vs the host engine on the final tree (gpu_session.sh queue)",
    "r05z_kernel_stats.csv": "rocprofv3 --kernel-trace --stats of the default bench (C2 stream_kernel seal / open)",
    "r05z_bench_under_rocprof.json": "the bench line printed by that rocprofv3 run",
    "r05z_kernel_stats_c3.csv": "rocprofv3 stats, C3 AEAD (records_kernel, line staging)",
    "r05z_kernel_stats_c3_wire.csv": "rocprofv3 stats, C3 wire frames (duplex_kernel)",
    "r05z_kernel_stats_fused_store.csv": "rocprofv3 stats, chunk store / fetch at C2 shape (duplex_kernel)",
    "r05z_kernel_stats_c5_device.csv": "rocprofv3 stats, C5 device-resident (duplex_split_kernel)",
    "r05z_kernel_stats_store_64k.csv": "rocprofv3 stats, 64 KiB chunk store / fetch (duplex_split_kernel)",
    "pmc_r05z.json": "PMC of the C2 bench kernels: HBM bytes per launch (bench.py roofline.traffic), VALU counts",
    "pmc_c3_r05z.json": "PMC, C3 AEAD",
    "pmc_c3w_r05z.json": "PMC, C3 wire frames",
    "pmc_st_r05z.json": "PMC, chunk store / fetch",
    "pmc_c5_r05z.json": "PMC, C5 device-resident",
    "r03_c5_chain_probe_split4.json": "C5 device chain probe with the four-wave split kernel",
    "r04_batch_bench_p13.jsonl": "crypto::batch C2 / C3 wire from vectors (round 4)",
    "r04_c2_copy_trace_summary.jsonl": "C2 host pipeline copy trace: small D2H behind every chunk copy",
    "r04_e2e_probe_hip_runtime.jsonl": "C2 host pipeline on the system vs torch's HIP runtime (round 4)",
    "r04_queue_bench_engine_modes.jsonl": "round-4 frame queue by engine mode",
    "r04f_e2e.json": "host-resident C2 e2e (round 4)",
    "r04f_rehearsal_c2_n2_gloo_one_gpu.json": "N = 2 gloo rehearsal of the C2 bench on one GPU (round 4)",
    "r04g_c5_share.jsonl": "C5 per-GPU share host-resident (round 4)",
    "r04g_e2e.jsonl": "host-resident C2 e2e sweep (round 4)",
    "r04r_host_legs.txt": "host legs of the round-4 bench, traced",
    "r04z_c5_probe.json": "C5 device-resident chain probe (round 4 final)",
}


def generic(f: str) -> str:
    if f.startswith("pmc"):
        return "PMC counter passes (tools/pmc.py): HBM bytes per launch, instruction counts, VALU busy"
    if "kernel_stats" in f:
        return "rocprofv3 --kernel-trace --stats summary"
    if f.endswith("pytest_gpu.log"):
        return "pytest -m gpu on the box"
    if "bench_under_rocprof" in f:
        return "the bench line printed by the rocprofv3 run (HIP-event vs rocprof kernel times)"
    if "torchrun" in f:
        return "bench.py through torch.distributed.run --nproc-per-node 1"
    if f.endswith("_bench.json"):
        return "default bench.py line"
    if "side" in f:
        return "bench.py side configs and modes"
    if "scalar_latency" in f:
        return "per-call latency of the reference-signature scalar calls"
    return ""


def main():
    move = "--move" in sys.argv
    txt = {d: open(os.path.join(ROOT, d)).read() for d in DOCS if os.path.exists(os.path.join(ROOT, d))}
    code = []
    for top in CODE_DIRS:
        for dp, dn, fs in os.walk(os.path.join(ROOT, top)):
            dn[:] = [x for x in dn if x not in ("build", "build_tools", "__pycache__", "_ref")]
            for f in fs:
                if f.endswith(CODE_EXT) and f != "profiles_index.py":
                    try:
                        code.append(open(os.path.join(dp, f), errors="replace").read())
                    except OSError:
                        pass
    txt["source comments"] = "\n".join(code)
    old = open(os.path.join(P, "README.md")).read() if os.path.exists(os.path.join(P, "README.md")) else ""
    olddesc = {}
    for line in old.splitlines():
        cells = [c.strip() for c in line.split("|")]
        if len(cells) < 4 or "`" not in cells[1]:
            continue
        for f in re.findall(r"`([^`]+)`", cells[1]):
            olddesc.setdefault(f, cells[2])
    files = sorted(f for f in os.listdir(P) if os.path.isfile(os.path.join(P, f)) and f != "README.md")
    rows, uncited = [], []
    for f in files:
        by = [d for d, t in txt.items() if f in t]
        if not by:
            uncited.append(f)
            continue
        rows.append((f, DESC.get(f) or olddesc.get(f) or generic(f), by))
    if move and uncited:
        os.makedirs(os.path.join(P, "archive"), exist_ok=True)
        for f in uncited:
            subprocess.run(["git", "mv", "-k", os.path.join("profiles", f), os.path.join("profiles", "archive", f)],
                           cwd=ROOT, check=True)
    out = ["# profiles/ -- evidence cited by the documents", "",
           "Every file here is cited by at least one of DESIGN.md, INTEGRATION.md, README.md,",
           "DESIGN_HISTORY.md, bench.py or a source comment (column 3).  Evidence no document cites any more (superseded",
           "runs of rounds 1-5) is kept, unindexed, under `archive/`.  Produced on one MI355X box per",
           "run (`tools/gpu_round.sh`; the round-5 recipes in `tools/gpu_session.sh`); the driver's own round-end lines are",
           "`BENCH_rNN.json` / `SCALE_rNN.json` at the repository root.  Regenerate with",
           "`python tools/profiles_index.py`.", "",
           "| file | what | cited by |", "|---|---|---|"]
    for f, d, by in rows:
        out.append(f"| `{f}` | {d} | {', '.join(by)} |")
    open(os.path.join(P, "README.md"), "w").write("\n".join(out) + "\n")
    print(f"{len(rows)} cited, {len(uncited)} uncited" + (" (moved to archive/)" if move else ""))


if __name__ == "__main__":
    main()
