"""The routing rule for long records (csrc/long_route.hpp choose_long_route: record engine,
one-launch uniform XOR / AEAD, or plan + tiles) and the plan + tiles scratch layout (seg_layout: one
claim byte per position of the launch, partials 256-aligned behind them; seg_claim_slot: the byte a
record owns, whatever index a caller's order gives it) against hand-made tables,
tests/cpp/route_table.cpp.  CPU only: the header is plain C++ and is compiled with g++ alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_long_route_table(tmp_path):
    out = str(tmp_path / "route_table")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "ephemeralnet_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "route_table.cpp"), "-o", out], check=True)
    res = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
