#!/bin/bash
# One GPU-box session: build, parity tests, smoke, short bench, kernel profile.
# Every GPU step has its own time limit; steps are chained so the first
# failure ends the session.
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT:-out/gpu_check}; mkdir -p $OUT
export TMPDIR=/tmp
STEP=${1:-all}
timeout -k 10 600 python -c "import __graft_entry__ as g; g.build()" > $OUT/build.log 2>&1 || { echo "build failed"; tail -30 $OUT/build.log; exit 1; }
if [ "$STEP" = "all" ] || [ "$STEP" = "test" ]; then
  timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1; rc=$?
  tail -25 $OUT/pytest_gpu.log
  [ $rc -eq 0 ] || exit $rc
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 || { cat $OUT/smoke.log; exit 1; }
  cat $OUT/smoke.log
fi
if [ "$STEP" = "all" ] || [ "$STEP" = "bench" ]; then
  timeout -k 10 600 python bench.py --full > $OUT/bench.log 2>&1 || { tail -30 $OUT/bench.log; exit 1; }
  tail -3 $OUT/bench.log
fi
if [ "$STEP" = "all" ] || [ "$STEP" = "prof" ]; then
  rm -rf $OUT/prof
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python3 bench.py --full --steps 5 --warmup 1 --no-cpu-baseline > $OUT/prof.log 2>&1 || { tail -30 $OUT/prof.log; exit 1; }
  find $OUT/prof -name "*kernel_stats.csv" | head -1 | xargs -I{} sh -c 'head -20 {}'
fi
