"""The routing rule of the record engine (csrc/record_route.hpp choose_record_route: which of the
per-lane, run-staged, line-staged, lockstep and streaming kernels a launch runs on, over how many
whole workgroups, with how many records left per lane) against a hand-made table,
tests/cpp/record_route_table.cpp.  CPU only: the header is plain C++ and is compiled with g++
alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_record_route_table(tmp_path):
    out = str(tmp_path / "record_route_table")
    subprocess.run(["g++", "-std=c++20", "-O1", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "ephemeralnet_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "record_route_table.cpp"), "-o", out], check=True)
    res = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stdout + res.stderr
    assert " 0 mismatches" in res.stdout, res.stdout[-2000:]


def test_record_route_counts_api():
    """enet_record_route_counts through the Python view, without a GPU: five cumulative counters
    named in the order of the header's RecordKind, and a NULL destination is ignored."""
    import re

    from ephemeralnet_amd import build as B
    B.build(verbose=False)
    import ephemeralnet_amd as E
    src = open(os.path.join(ROOT, "ephemeralnet_amd", "csrc", "record_route.hpp")).read()
    body = re.search(r"enum class RecordKind : int \{(.*?)\};", src, re.S).group(1)
    kinds = [(name, int(val)) for name, val in re.findall(r"^\s*(\w+) = (\d+),", body, re.M)]
    assert kinds == [(k, i) for i, k in enumerate(E.ROUTE_KINDS)] and len(kinds) == 5
    first = E.record_route_counts()
    assert tuple(first) == E.ROUTE_KINDS and all(isinstance(v, int) and v >= 0 for v in first.values())
    E.lib().enet_record_route_counts(None)
    second = E.record_route_counts()
    assert all(second[k] >= first[k] for k in E.ROUTE_KINDS)
