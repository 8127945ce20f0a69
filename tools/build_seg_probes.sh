#!/bin/bash
# Hand-built probe library: segments.hip recompiled with -DENET_SEG_PROBE_<SWITCH>, linked with the
# product's other objects into ephemeralnet_amd/libenet_probe_<SWITCH>.so.  TRACE is the one switch
# segments.hip still reads (per-workgroup phase stamps; correct bytes): tools/seg_trace.py reads
# the stamps, tools/seg_ab.sh times the library beside the shipping one.
#   bash tools/build_seg_probes.sh TRACE
# Run after `python -m ephemeralnet_amd.build`.
set -euo pipefail
cd "$(dirname "$0")/.."
B=ephemeralnet_amd/build
for v in "$@"; do
  o=/tmp/seg_probe_$v.o
  defs=""; for d in ${v//+/ }; do defs="$defs -DENET_SEG_PROBE_$d"; done
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++20 -fPIC -fvisibility=hidden -Wall -Wno-unused-function \
    -Iinclude $defs -c ephemeralnet_amd/csrc/segments.hip -o $o
  objs=$(ls $B/*.o | grep -v '/segments.o$')
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -fPIC -shared $objs $o -o ephemeralnet_amd/libenet_probe_$v.so
  echo built ephemeralnet_amd/libenet_probe_$v.so
done
