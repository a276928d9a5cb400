#!/bin/bash
# round 6 final check on the final tree: GPU tests, smoke, a short bench
set -o pipefail
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}   # output folder, relative to the repository root
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/gpu_tests.log 2>&1
rc=$?; echo "tests rc=$rc"; tail -2 $OUT/gpu_tests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -1 $OUT/smoke.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 900 python bench.py --full --steps 5 --warmup 1 > $OUT/bench_final.log 2>&1
rc=$?; echo "bench rc=$rc"; grep "^{" $OUT/bench_final.log | cut -c1-200; [ $rc -eq 0 ] || exit $rc
