"""Cross-session frame queues (crypto::batch::FrameQueue / FrameReceiveQueue; SURVEY.md 8f row 1;
VERDICT r02 item 5): 16 session threads seal through one shared send queue and open through one
shared receive queue at the same time (tests/cpp/queue_stress.cpp).  Checked: every thread gets
back exactly its own messages, tampered frames (nonce, length field, body, MAC) and frames opened
under another session's key are rejected for that caller only, oversized payloads are refused
like SessionManager::send, flushes batch many frames, and sampled frames are bit-exact with the
oracle's restatement of SessionManager::send + encode_signed (SessionManager.cpp:362-387,
Message.cpp:305-311).  CPU: the host engine serves the flushes (policy host, and policy device
with no usable device -- every flush a counted device failure finished on the host).  GPU: the
flushes run on the MI355X."""
import os
import re
import subprocess

import pytest

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "queue_stress.cpp")


def compile_against(lib, src, out):
    """Build a test program from `src` against the library file `lib`."""
    name = os.path.basename(lib)[len("lib"):-len(".so")]
    subprocess.run(["g++", "-std=c++20", "-O2", "-pthread", "-I", os.path.join(ROOT, "include"), src, "-o", out,
                    "-L", os.path.dirname(lib), "-l" + name, "-Wl,-rpath," + os.path.dirname(lib)], check=True)
    return out


@pytest.fixture(scope="module")
def stress_bin(tmp_path_factory):
    from ephemeralnet_amd import build as B
    return compile_against(B.build(verbose=False), SRC, str(tmp_path_factory.mktemp("q") / "queue_stress"))


@pytest.fixture(scope="module")
def tools_stress_bin(tmp_path_factory):
    """queue_stress over the tools build (stand-in device, stall hook, A/B knobs); skips when that
    build is missing or stale."""
    from ephemeralnet_amd import build as B
    stamp = B.read_stamp(B.LIB_TOOLS)
    if not os.path.exists(B.LIB_TOOLS) or not stamp or stamp.get("sources_sha256") != B.source_digest(tools=True):
        pytest.skip("tools build (ephemeralnet_amd/libenet_crypto_tools.so) missing or stale")
    return compile_against(B.LIB_TOOLS, SRC, str(tmp_path_factory.mktemp("qt") / "queue_stress_tools"))


def summary(r):
    """The k=v pairs of a queue_stress run's summary line."""
    summ = [ln for ln in r.stdout.splitlines() if ln.startswith("summary")]
    assert summ, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return {k: int(v) for k, v in (kv.split("=") for kv in summ[0].split()[1:])}


def run(stress_bin, policy, threads=16, frames=150, seed=1):
    r = subprocess.run([stress_bin, policy, str(threads), str(frames), str(seed)], capture_output=True,
                       text=True, timeout=600)
    s = summary(r)
    sample = [ln.split()[1:] for ln in r.stdout.splitlines() if ln.startswith("frame ")]
    return r.returncode, s, sample, r.stderr


def check_common(rc, s, sample, threads, frames):
    # every sealed frame equals the host engine's bytes for its key, message and nonce
    assert rc == 0 and s["bad"] == 0 and s["wrong"] == 0 and s["mismatch"] == 0, s
    assert s["oversize_refused"] == threads
    # every sealed frame reaches the send queue (the oversized ones are refused before it); every
    # opened frame reaches the receive queue except those whose length field was tampered, which
    # fail receive_loop's shape check first (SessionManager.cpp:770-796) and are never queued
    assert s["tx_frames"] == threads * frames, s
    length_tampered = sum(1 for t in range(threads) for i in range(frames) if i % 7 == 3 and (i // 7) % 4 == 1)
    assert s["rx_frames"] == s["opened"] + s["rejected"] - length_tampered, s
    assert s["tx_flushes"] >= 1 and s["rx_flushes"] >= 1 and s["tx_flushes"] <= s["tx_frames"]
    tampered = sum(1 for t in range(threads) for i in range(frames) if i % 7 == 3)
    foreign = sum(1 for t in range(threads) for i in range(frames) if i % 7 != 3 and i % 11 == 4)
    assert s["rejected"] == tampered + foreign
    assert s["opened"] == threads * frames - tampered - foreign
    assert len(sample) == 3 * threads
    for key, m, frame in sample:
        key, frame = bytes.fromhex(key), bytes.fromhex(frame)
        m = b"" if m == "-" else bytes.fromhex(m)
        nonce = frame[:12]
        assert int.from_bytes(frame[12:16], "big") == len(m) + 32
        assert frame[16:] == oracle.frame_seal(key, nonce, m)
    assert len({bytes.fromhex(f)[:12] for _, _, f in sample}) == len(sample)  # fresh nonces


@pytest.mark.parametrize("policy", ["host", "device"])
def test_frame_nonces_never_repeat(stress_bin, policy):
    """8 threads x 30 000 frames under ONE session key: every nonce distinct (each thread's
    ChaCha20 nonce generator hands out whole keystream blocks once; refills and re-keys included).
    CPU: host engine (device policy finishes its flushes on the host with no device)."""
    if policy == "device" and os.path.exists("/dev/kfd"):
        pytest.skip("device flushes are covered by the -m gpu queue tests")
    r = subprocess.run([stress_bin, "nonces", policy, "8", "30000"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-500:])
    assert "total=240000 distinct=240000" in r.stdout


def test_queues_16_threads_host_engine(stress_bin):
    """Host policy: no queue -- every session thread seals / opens its own frame on the host
    engine (one 'flush' per frame), bit-exact and isolated as through the queue."""
    rc, s, sample, _ = run(stress_bin, "host")
    check_common(rc, s, sample, 16, 150)
    assert s["tx_host_flushes"] == s["tx_flushes"] == s["tx_frames"] and s["device_failures"] == 0


def test_queues_16_threads_device_failure_on_cpu(stress_bin):
    """No usable device here: each flush's device pass fails and is finished on the host
    engine; callers never see an exception or a wrong frame."""
    rc, s, sample, err = run(stress_bin, "device", frames=60)
    check_common(rc, s, sample, 16, 60)
    assert s["tx_flushes"] < s["tx_frames"]  # batched: many frames per flush
    if s["device_failures"] == 0 and s["tx_host_flushes"] == 0:
        pytest.skip("a usable device served every flush (GPU box): covered by the -m gpu tests")
    assert s["device_failures"] >= s["tx_flushes"] > 0
    assert "finished on the host engine" in err


@pytest.mark.gpu
def test_queues_16_threads_on_gpu(stress_bin):
    """Policy device: every flush is one MI355X pass over the frames queued by 16 session
    threads (batched, no host flush, no device failure), bit-exact and isolated per caller."""
    rc, s, sample, err = run(stress_bin, "device")
    check_common(rc, s, sample, 16, 150)
    assert s["tx_flushes"] < s["tx_frames"]  # batched: many frames per flush
    assert s["tx_host_flushes"] == 0 and s["rx_host_flushes"] == 0 and s["device_failures"] == 0, err


@pytest.mark.gpu
def test_queues_16_threads_auto_policy_on_gpu(stress_bin):
    """Policy auto with a working GPU: the queues route MTU-sized frames to each session thread's
    host engine (measured faster than a device pass): one host pass per frame,
    no device failure, same bytes."""
    rc, s, sample, err = run(stress_bin, "auto")
    check_common(rc, s, sample, 16, 150)
    assert s["tx_host_flushes"] == s["tx_flushes"] == s["tx_frames"] and s["device_failures"] == 0, err


@pytest.mark.gpu
@pytest.mark.parametrize("policy", ["auto", "device"])
def test_queues_512_blocking_session_threads_on_gpu(stress_bin, policy):
    """The reference's own session threading (SessionManager.cpp:331-332 one reader thread per
    session; send() seals synchronously, :337-388; receive_loop opens one frame at a time, :822):
    512 session threads, each with ONE blocking frame in flight, 20 frames each (a 64 KiB one and
    the 1 MiB maximum payload among them), every 7th opened frame tampered, every 11th opened under
    another session's key.  Every sealed frame is checked byte for byte against the host engine
    (and 1 536 of them against the oracle).  Routing: AUTO serves every blocking frame on the
    calling thread's host engine (profiles/r06_sessions_blocking.jsonl: 64-4 096 blocked threads
    move 7-10 M frames/s there against 0.2-2.4 M through device passes); DEVICE batches the
    blocked threads' frames into shared passes, no host flush."""
    rc, s, sample, err = run(stress_bin, policy, threads=512, frames=20)
    check_common(rc, s, sample, 512, 20)
    assert s["device_failures"] == 0, err
    if policy == "auto":
        assert s["tx_host_flushes"] == s["tx_flushes"] == s["tx_frames"], s
        assert s["rx_host_flushes"] == s["rx_flushes"] == s["rx_frames"], s
    else:
        assert s["tx_host_flushes"] == 0 and s["rx_host_flushes"] == 0, s
        assert s["tx_flushes"] < s["tx_frames"] and s["rx_flushes"] < s["rx_frames"], s  # shared passes


def run_async(stress_bin, policy, threads=8, frames=400):
    r = subprocess.run([stress_bin, "async", policy, str(threads), str(frames)], capture_output=True, text=True,
                       timeout=600)
    return r.returncode, summary(r), r.stderr


def check_async(rc, s, threads, frames):
    # every frame is >= 48 bytes, so byte 20 (in the body) of every 5th one is flipped
    tampered = threads * sum(1 for i in range(frames) if i % 5 == 2)
    assert rc == 0 and s["bad"] == 0 and s["mismatch"] == 0, s
    assert s["opened"] + s["rejected"] == threads * frames
    assert s["tx_frames"] == threads * frames and s["rx_frames"] == threads * frames, s
    assert s["rejected"] == tampered


@pytest.mark.parametrize("policy", ["host", "device"])
def test_queues_async_cpu(stress_bin, policy):
    """seal_async / open_async (non-blocking submission): 8 threads each put 400 frames in flight
    before waiting; every result comes back to its own future, tampered frames are rejected.  CPU:
    the host engine serves them (device policy: each pass fails over to the host engine)."""
    if policy == "device" and os.path.exists("/dev/kfd"):
        pytest.skip("device passes are covered by the -m gpu queue tests")
    rc, s, err = run_async(stress_bin, policy)
    check_async(rc, s, 8, 400)


@pytest.mark.gpu
def test_queues_async_on_gpu(stress_bin):
    """Device policy, async submission: passes carry many frames (several in flight at once), no
    host pass, no device failure, every frame bit-exact back to its own caller."""
    rc, s, err = run_async(stress_bin, "device")
    check_async(rc, s, 8, 400)
    assert s["tx_host_flushes"] == 0 and s["rx_host_flushes"] == 0, err
    # every thread submits all 400 before collecting any: passes carry many threads' frames
    assert s["tx_frames"] / s["tx_flushes"] >= 64 and s["rx_frames"] / s["rx_flushes"] >= 64, s


def run_window(stress_bin, policy, threads=16, window=256, frames=4000):
    r = subprocess.run([stress_bin, "window", policy, str(threads), str(window), str(frames)], capture_output=True,
                       text=True, timeout=600)
    return r.returncode, summary(r), r.stderr


def check_window(rc, s, threads, frames):
    # every sealed frame equals the host engine's bytes (mismatch), and decrypts / verifies (bad)
    assert rc == 0 and s["bad"] == 0 and s["mismatch"] == 0, s
    tampered = sum(1 for i in range(frames) if i % 9 == 4)
    foreign = sum(1 for i in range(frames) if i % 9 != 4 and i % 13 == 6) if threads > 1 else 0
    assert s["rejected"] == threads * (tampered + foreign), s
    assert s["opened"] == threads * (frames - tampered - foreign), s
    assert s["tx_frames"] == threads * frames and s["rx_frames"] == threads * frames, s


def test_queues_window_cpu(stress_bin):
    """submit() / FrameTicket with a window of frames in flight per thread, host policy (CPU): every
    sealed frame verified independently, tampered / foreign-key frames rejected per caller."""
    rc, s, err = run_window(stress_bin, "host", threads=8, window=64, frames=600)
    check_window(rc, s, 8, 600)


@pytest.mark.gpu
def test_queues_window_on_gpu(stress_bin):
    """16 threads x 256 frames in flight through the device queue, every pass on
    the MI355X, every frame verified.  Batching is checked loosely here (each thread also verifies
    every frame on the host, which throttles its arrivals); test_queue_bench_passes_and_rate_on_gpu
    checks the >= 1 000-frame passes at the queue's own load."""
    rc, s, err = run_window(stress_bin, "device")
    check_window(rc, s, 16, 4000)
    assert s["tx_host_flushes"] == 0 and s["rx_host_flushes"] == 0 and s["device_failures"] == 0, err
    tx_pass, rx_pass = s["tx_frames"] / s["tx_flushes"], s["rx_frames"] / s["rx_flushes"]
    print("frames per pass", tx_pass, rx_pass, s)
    # every thread here also verifies each sealed frame on the host engine (~3-7 us a frame) and
    # waits for its oldest ticket, so its arrival rate, not the queue, sets the pass size (passes
    # close on a 30 us arrival gap); tools/queue_bench, a consumer that only collects, fills passes
    # of 530-900 frames at this load and 1 023 at 1 024 in flight.
    assert tx_pass >= 48 and rx_pass >= 48, s


@pytest.mark.gpu
def test_queues_window_evictions_on_gpu(stress_bin):
    """16 threads x 4 096 frames in flight reference more passes than a queue keeps (48), so
    finished passes are evicted into their uncollected tickets while the device keeps running the
    others (generation-tagged slots): evictions happen, every pass runs on the
    MI355X, and every frame is still verified byte for byte."""
    rc, s, err = run_window(stress_bin, "device", threads=16, window=4096, frames=5000)
    check_window(rc, s, 16, 5000)
    print(s)
    assert s["tx_host_flushes"] == 0 and s["rx_host_flushes"] == 0 and s["device_failures"] == 0, err
    assert s["evicted"] > 0, s


@pytest.mark.gpu
def test_queues_window_auto_policy_on_gpu(stress_bin):
    """Policy auto routes a non-blocking submission by its thread's backlog (frames submitted and
    not yet collected): with 512 in flight per thread the device queue takes over once a thread
    holds 320 (where it overtakes the host engine, profiles/r05_seal_crossover_hi.jsonl) -- only
    each thread's first frames run on the host engine -- and with 16 in flight every frame stays on
    the host engine (the device queue would be ~13x slower there)."""
    rc, s, err = run_window(stress_bin, "auto", window=512, frames=1500)
    check_window(rc, s, 16, 1500)
    print("auto, 512 in flight:", s)
    assert s["device_failures"] == 0, err
    assert s["tx_host_flushes"] <= 16 * 330 and s["rx_host_flushes"] <= 16 * 330, s
    assert s["tx_flushes"] > s["tx_host_flushes"] and s["rx_flushes"] > s["rx_host_flushes"], s
    rc, s, err = run_window(stress_bin, "auto", window=16, frames=600)
    check_window(rc, s, 16, 600)
    print("auto, 16 in flight:", s)
    assert s["tx_host_flushes"] == s["tx_flushes"] == s["tx_frames"], s


BENCH_SRC = os.path.join(ROOT, "tools", "queue_bench.cpp")


@pytest.mark.gpu
def test_queue_bench_passes_and_rate_on_gpu(tmp_path):
    """VERDICT r04 item 2 at the queue's own load (tools/queue_bench: 16 session threads each
    keeping 1 024 MTU frames in flight and collecting into a reused buffer, nothing else per
    frame): every pass runs on the MI355X, all sizes right.  With 4 device passes in flight a pass
    holds ~1 000 frames on average (992-1 016 measured; >= 950 asserted -- the mean moves with
    the host threads' scheduling); with the default 8 (1.3x the frames at this load) the
    workers take passes a little earlier (910-1 016 frames measured) and the rate must stay
    >= 8 M frames/s each way.  Rates and CPU per frame are printed."""
    from ephemeralnet_amd import build as B
    out = compile_against(B.build(verbose=False), BENCH_SRC, str(tmp_path / "queue_bench"))
    import json
    for inflight in ("4", None):
        args = [out, "device", "reuse", "16", "1024", "1.0"] + (["1500", inflight] if inflight else [])
        r = subprocess.run(args, capture_output=True, text=True, timeout=120)
        d = json.loads(r.stdout.strip().splitlines()[-1])
        print(d)
        assert r.returncode == 0 and d["ok"] == 1, (r.stdout[-2000:], r.stderr[-2000:])
        assert d["tx_host_passes"] == 0 and d["rx_host_passes"] == 0 and d["device_failures"] == 0, d
        if inflight:
            assert d["tx_frames_per_pass"] >= 950 and d["rx_frames_per_pass"] >= 950, d
        else:
            assert d["tx_frames_per_pass"] >= 800 and d["rx_frames_per_pass"] >= 800, d
            assert d["seal_frames_per_s"] >= 8e6 and d["open_frames_per_s"] >= 8e6, d


def test_device_style_passes_and_evictions_on_cpu(tools_stress_bin):
    """The queue's device path on a CPU-only host: the tools build's stand-in device
    (ENET_QUEUE_FAKE_US: a pass takes 100 us; ENET_QUEUE_FAKE_COMPUTE: the worker computes it on
    the host engine first) runs every pass as a device pass.  16 threads x 4 096 frames in flight
    reference more passes than the queue keeps, so finished passes are evicted into their tickets
    while other threads collect, drop and reuse slots (generation-tagged slot words); every frame
    is still checked byte for byte and every tamper rejected."""
    env = dict(os.environ, ENET_QUEUE_FAKE_US="100", ENET_QUEUE_FAKE_COMPUTE="1")
    r = subprocess.run([tools_stress_bin, "window", "device", "16", "4096", "5000"], capture_output=True, text=True,
                       timeout=600, env=env)
    s = summary(r)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(s)
    assert s["bad"] == 0 and s["tx_frames"] == 16 * 5000 and s["rx_frames"] == 16 * 5000
    assert s["tx_host_flushes"] == 0 and s["rx_host_flushes"] == 0 and s["device_failures"] == 0
    assert s["evicted"] > 0


@pytest.mark.gpu
def test_queues_staged_passes_on_gpu(tools_stress_bin):
    """Device passes with their input side staged in device memory (one SDMA copy, the kernel
    reading HBM, the results written straight into the pinned pass -- the default for passes of
    640+ frames sealing, 512+ opening): forced on every pass through the tools build
    (ENET_QUEUE_STAGE=1), the window stress run checks every frame byte for byte and every tamper rejected, with no host
    flush and no device failure."""
    env = dict(os.environ, ENET_QUEUE_STAGE="1")
    r = subprocess.run([tools_stress_bin, "window", "device", "16", "256", "1500"], capture_output=True, text=True,
                       timeout=300, env=env)
    s = summary(r)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(s)
    check_window(r.returncode, s, 16, 1500)
    assert s["tx_host_flushes"] == 0 and s["rx_host_flushes"] == 0 and s["device_failures"] == 0, s


def test_stalled_overflow_submitter_on_cpu(tools_stress_bin):
    """a submitter whose reservation found its pass full and that is then
    preempted must not close the pass's NEXT generation (reopened meanwhile, possibly for another
    shard): that left the new owner's open pointer on a closed pass.  The fix ties close_full to
    the generation read before the reservation and clears every shard that holds the pass.  This
    run exercises that path hard on the CPU: the tools build's stand-in device runs device-style
    passes, passes of 16 frames (QUEUE_STRESS_MAX_FRAMES=64) overflow constantly, 2 shards by
    thread order, and ENET_QUEUE_STALL_OVERFLOW_US holds every overflowing submitter 300 us before
    its close while passes are evicted and reopened; every frame is checked byte for byte.  (The
    stale close did not hang here before the fix either: eviction churn soon reopens the pass for
    some shard, which re-validates the dangling pointer -- the fix is by construction.)"""
    env = dict(os.environ, ENET_QUEUE_FAKE_US="20", ENET_QUEUE_FAKE_COMPUTE="1", ENET_QUEUE_STALL_OVERFLOW_US="300",
               ENET_QUEUE_SHARDS="2", ENET_QUEUE_SHARD_BY="thread", QUEUE_STRESS_MAX_FRAMES="64")
    r = subprocess.run([tools_stress_bin, "window", "device", "16", "128", "3000"], capture_output=True, text=True,
                       timeout=120, env=env)
    s = summary(r)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(s)
    check_window(r.returncode, s, 16, 3000)
    assert s["overflows"] > 1000 and s["evicted"] > 0, s


def test_split_submitter_collector_auto_stays_on_host_on_cpu(tools_stress_bin):
    """one reader thread submits, one writer thread collects, at most 8 frames
    between them, policy auto with a (stand-in) device.  The frames are counted against the
    submitting thread only until collected -- on the other thread -- so the trickle never reaches
    AUTO's device threshold (320): every frame on the host engine, every byte checked."""
    env = dict(os.environ, ENET_QUEUE_FAKE_US="60", ENET_QUEUE_FAKE_COMPUTE="1")
    r = subprocess.run([tools_stress_bin, "split", "auto", "3000", "8"], capture_output=True, text=True, timeout=300, env=env)
    s = summary(r)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    print(s)
    assert s["bad"] == 0 and s["mismatch"] == 0
    assert s["tx_frames"] == 3000 and s["tx_host_flushes"] == s["tx_flushes"] == 3000, s


def test_split_submitter_collector_device_on_cpu(tools_stress_bin):
    """The same split under the device policy (stand-in device): the frames go through passes and
    come back byte for byte to the collecting thread."""
    env = dict(os.environ, ENET_QUEUE_FAKE_US="60", ENET_QUEUE_FAKE_COMPUTE="1")
    r = subprocess.run([tools_stress_bin, "split", "device", "2000", "64"], capture_output=True, text=True, timeout=300, env=env)
    s = summary(r)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert s["bad"] == 0 and s["mismatch"] == 0 and s["tx_frames"] == 2000 and s["tx_host_flushes"] == 0, s


def run_tickets(binary, policy, threads, frames, **env):
    r = subprocess.run([binary, "tickets", policy, str(threads), str(frames)], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, **env))
    return r.returncode, summary(r), r.stderr


def check_tickets(rc, s, threads, frames):
    """queue_stress tickets: per thread every third item is dropped (destructor, release() after
    ready(), move-assignment), the others are collected after ready() or through view() + get();
    the collected frames are opened the same way (every 5th tampered); then 2 000 frames all
    dropped, 16 collected, and 200 each way through queues destroyed before their tickets."""
    assert rc == 0 and s["bad"] == 0 and s["mismatch"] == 0, s
    dropped = lambda n: sum(1 for k in range(n) if k % 3 == 1)
    sealed = frames - dropped(frames)  # frames collected from the send queue = frames opened
    assert s["tx_submitted"] == threads * (frames + 2000 + 16) and s["rx_submitted"] == threads * sealed, s
    # every submitted frame is served, collected or not
    assert s["tx_frames"] == s["tx_submitted"] and s["rx_frames"] == s["rx_submitted"], s
    assert s["dropped"] == threads * (dropped(frames) + dropped(sealed) + 2000), s
    assert s["collected"] == threads * (sealed + sealed - dropped(sealed) + 16), s
    rejected = sum(1 for j in range(sealed) if j % 3 != 1 and j % 5 == 2) + sum(1 for i in range(200) if i % 5 == 2)
    assert s["rejected"] == threads * rejected, s
    assert s["opened"] == threads * (sealed - dropped(sealed) + 200 - rejected), s


def test_tickets_host_engine(stress_bin):
    """FrameTicket::ready(), dropped tickets, view() twice + get(), tickets outliving their queue
    and the empty ticket under the host policy: every ticket is born with its result."""
    rc, s, _ = run_tickets(stress_bin, "host", 8, 600)
    check_tickets(rc, s, 8, 600)
    assert s["tx_host_flushes"] == s["tx_flushes"] == s["tx_frames"] and s["device_failures"] == 0, s
    assert s["burst_host"] == 8 * 2000 and s["after_drop_host"] == 8 * 16, s


@pytest.mark.parametrize("policy", ["device", "auto"])
def test_tickets_device_style_passes_on_cpu(tools_stress_bin, policy):
    """The same through device-style passes (the tools build's stand-in device computing on the
    host engine), passes of 16 slots so that dropped and half-collected passes must be reused and
    evicted for the run to finish.  auto: each thread's burst reaches the device queue once it
    holds 320 uncollected frames, and after dropping all of them its next 16 frames are served by
    the host engine again -- exactly 16 host flushes per thread: the dropped tickets left AUTO's
    backlog."""
    rc, s, _ = run_tickets(tools_stress_bin, policy, 8, 600, ENET_QUEUE_FAKE_US="60", ENET_QUEUE_FAKE_COMPUTE="1",
                           QUEUE_STRESS_MAX_FRAMES="64")
    print(s)
    check_tickets(rc, s, 8, 600)
    assert s["device_failures"] == 0 and s["evicted"] > 0, s
    if policy == "device":
        assert s["tx_host_flushes"] == 0 and s["rx_host_flushes"] == 0 and s["after_drop_host"] == 0, s
    else:
        assert s["after_drop_host"] == 8 * 16, s
        assert s["burst_host"] <= 8 * 320 and s["tx_flushes"] > s["tx_host_flushes"], s


@pytest.mark.gpu
def test_tickets_on_gpu(stress_bin):
    """4 threads x 64 in flight x 500 frames, policy device: several passes per shard and slots
    reused across generations on the MI355X; no host flush, no device failure."""
    rc, s, err = run_tickets(stress_bin, "device", 4, 500)
    print(s)
    check_tickets(rc, s, 4, 500)
    assert s["tx_host_flushes"] == 0 and s["rx_host_flushes"] == 0 and s["device_failures"] == 0, err
    assert s["tx_flushes"] < s["tx_frames"], s


def test_tools_build_compiles_every_unit_behind_the_knobs_header():
    """The tools-build hooks live in csrc/queue_knobs.hpp: every unit that includes it, directly or
    through another header, is among the units compiled with -DENET_TOOLS_BUILD (a unit left out
    would link the product's empty inlines into the tools library) and no kernel is; and the tools
    library's stamp records each of those units as built with that flag, naming nothing else as
    recompiled."""
    from ephemeralnet_amd import build as B
    tus = B.tools_tus()
    assert {"frame_queue.cpp", "queue_core.cpp", "capi.cpp", "host_batch.cpp"} <= set(tus), tus
    assert not [f for f in tus if f.endswith(".hip")], tus
    for f in B.SOURCES:  # the selection is the text search of every unit's include closure
        text = open(os.path.join(B.CSRC, f)).read()
        if f.endswith(".cpp") and ("ENET_TOOLS_BUILD" in text or '#include "queue_core.hpp"' in text):
            assert f in tus, f
    stamp = B.read_stamp(B.LIB_TOOLS)
    if not os.path.exists(B.LIB_TOOLS) or not stamp or stamp.get("sources_sha256") != B.source_digest(tools=True):
        pytest.skip("tools build (ephemeralnet_amd/libenet_crypto_tools.so) missing or stale")
    for f in tus:
        assert stamp["tu_sha256"][f] == B.tu_digest(f, tools=True), f  # flags + source + headers
        assert stamp["tu_sha256"][f] != B.tu_digest(f, tools=False), f
    assert set(stamp["recompiled"]) <= set(tus), stamp["recompiled"]
