#!/bin/bash
# One gpurun call: GPU parity tests, smoke, bench, rocprof summary.  A step that is killed or
# times out (rc 124/137) stops the script: no further GPU step runs after a hang.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
# every log, the bench line and the profiler output go under $OUT (default run_out/ in the repository root)
OUT=${OUT:-run_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
stage() {  # name timeout cmd...
  local name=$1 to=$2; shift 2
  echo "=== $name ===" | tee -a "$OUT/run.log"
  timeout -k 10 "$to" "$@" > "$OUT/$name.log" 2>&1
  local rc=$?
  echo "$name rc=$rc" | tee -a "$OUT/run.log"
  tail -n 25 "$OUT/$name.log"
  if [ $rc -eq 124 ] || [ $rc -eq 137 ]; then echo "ABORT: $name hung/killed" | tee -a "$OUT/run.log"; exit $rc; fi
  return $rc
}
: > "$OUT/run.log"
WHAT=${1:-all}
if [ "$WHAT" = all ] || [ "$WHAT" = test ]; then
  stage pytest_gpu 900 python -m pytest tests -m gpu -q --no-header -p no:cacheprovider ${PYTEST_ARGS--x}
fi
if [ "$WHAT" = all ] || [ "$WHAT" = bench ]; then
  stage smoke 300 python __graft_entry__.py smoke
  stage bench 600 python bench.py --steps ${STEPS:-10} --warmup 3 --full
  grep -E '^\{' "$OUT/bench.log" | tail -n 1 > "$OUT/bench.json"
fi
if [ "$WHAT" = all ] || [ "$WHAT" = prof ]; then
  rm -rf "$OUT/prof"
  stage rocprof 600 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o bench -- python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline --no-extras
  find "$OUT/prof" -name '*kernel_stats*' | head -n 3 | tee -a "$OUT/run.log"
fi
echo DONE | tee -a "$OUT/run.log"
