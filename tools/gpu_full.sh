#!/bin/bash
# Full -m gpu suite, then the C2 bench and the bf16 (C3-shape) bench.
#   gpurun -- bash tools/gpu_full.sh <tag>
set -o pipefail
OUT=gpurun_out/${1:-full}
mkdir -p "$OUT"
export TMPDIR=/tmp
step() {
  local t=$1 log=$2; shift 2
  echo "== $(date +%T) $*" | tee -a "$OUT/steps.log"
  timeout -k 10 "$t" "$@" > "$OUT/$log" 2>&1
  local rc=$?
  echo "   rc=$rc" | tee -a "$OUT/steps.log"
  tail -2 "$OUT/$log"
  return $rc
}
step 900 pytest_gpu.log python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread || exit 1
step 300 bench.json python bench.py --full || exit 1
step 300 bench_bf16.json python bench.py --full --dtype bf16 --no-cpu-baseline || exit 1
echo "all steps ok"
