"""The lane map of the streaming kernel (csrc/stream_map.hpp: which record and record-lane each
thread of a workgroup serves, and which thread's run each memory-wave op moves) against the rule
written out again in tests/cpp/stream_map_table.cpp.  CPU only: the header is plain C++; the
program is a stand-alone executable built with the address and undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_map_table(tmp_path):
    out = str(tmp_path / "stream_map_table")
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "ephemeralnet_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "stream_map_table.cpp"), "-o", out], check=True)
    res = subprocess.run([out], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert " 0 mismatches" in res.stdout, res.stdout[-2000:]
