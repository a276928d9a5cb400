#!/bin/bash
# codec parity on the GPU (incl. lz4 / blosclz), then a bench run with the lz4 leg
set -o pipefail
OUT=${OUT:-bench_out}   # output folder, relative to the repository root
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests/test_gpu_codec.py -m gpu -x -v --timeout 300 --timeout-method thread \
  > $OUT/lz_tests.log 2>&1
rc=$?; echo "tests rc=$rc"; grep -E "passed|failed|Error|assert" $OUT/lz_tests.log | tail -8
[ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python bench.py --full --steps 5 --warmup 1 --cpu-seconds 3 --e2e 0 --cfg3 0 --cfg5 0 > $OUT/lz_bench.log 2>&1
rc=$?; echo "bench rc=$rc"; grep -v amdgpu.ids $OUT/lz_bench.log | tail -2
exit $rc
