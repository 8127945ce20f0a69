# A/B of the stream kernel's issue settings (stream.hip stream_issue: wave priorities, the place of
# open's Poly1305) through bench.py, in the shipping flavour of the kernel.
#
#   bash tools/stream_issue_ab.sh build N [N ...]
#       candidate libraries: stream.hip compiled with -DENET_STREAM_ISSUE=N (the default kernel runs
#       with the settings of number N), linked with the product's other objects (build.py first)
#       -> ephemeralnet_amd/cand/libenet_issue_N.so
#   [BASE=lib.so] [ROUNDS=5] [OUT=file.jsonl] bash tools/stream_issue_ab.sh run N [N ...]
#       ROUNDS alternating rounds of plain `python bench.py` (400 steps, 50 warm-up): BASE (default:
#       the in-tree product library), then every candidate (a number, or the path of a library);
#       each run under its own time limit, the first failure ends the script.  One line per run in
#       OUT: {"lib", "round", "value", ...}.
set -euo pipefail
cd "$(dirname "$0")/.."
P=ephemeralnet_amd
cmd=$1; shift
case $cmd in
build)
  mkdir -p $P/cand
  FLAGS="--offload-arch=gfx950 -O3 -std=c++20 -fPIC -fvisibility=hidden -Wall -Wno-unused-function -Iinclude"
  for n in "$@"; do
    ( ${HIPCC:-/opt/rocm/bin/hipcc} $FLAGS -DENET_STREAM_ISSUE=$n -c $P/csrc/stream.hip -o $P/cand/stream_$n.o ) &
    while [ "$(jobs -r | wc -l)" -ge "${JOBS:-8}" ]; do wait -n; done
  done
  wait
  for n in "$@"; do
    objs=$(ls $P/build/*.o | grep -v '/stream\.o$')
    ${HIPCC:-/opt/rocm/bin/hipcc} --offload-arch=gfx950 -fPIC -shared $objs $P/cand/stream_$n.o -o $P/cand/libenet_issue_$n.so
    rm -f $P/cand/stream_$n.o
  done
  ;;
run)
  OUT=${OUT:-bench_out/stream_issue_ab.jsonl}; mkdir -p "$(dirname "$OUT")"; : > "$OUT"
  BASE=${BASE:-$P/libenet_crypto.so}
  for r in $(seq 1 "${ROUNDS:-5}"); do
    for lib in "$BASE" $(for n in "$@"; do if [ -f "$n" ]; then echo "$n"; else echo $P/cand/libenet_issue_$n.so; fi; done); do
      ENET_LIB_PATH=$lib timeout -k 10 "${LIMIT:-120}" python bench.py > /tmp/stream_issue_ab.$$ || { echo "bench.py failed with $lib" >&2; exit 1; }
      tail -n 1 /tmp/stream_issue_ab.$$ | python -c "
import json, sys
d = json.loads(sys.stdin.read())
print(json.dumps({'lib': '$lib', 'round': $r, 'value': d['value'], 'unit': d.get('unit'), 'ms_per_step': d.get('ms_per_step')}))" | tee -a "$OUT"
    done
  done
  rm -f /tmp/stream_issue_ab.$$
  ;;
*) echo "usage: stream_issue_ab.sh build|run N [N ...]" >&2; exit 2 ;;
esac
