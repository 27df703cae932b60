#!/bin/bash
# GPU-box check: parity tests, then (only if the tests ran to completion without a
# crash/timeout) one full bench line.  Outputs under $OUT (LLFE_OUT, default bench_out/).
set -u
OUT=${LLFE_OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread -p no:cacheprovider > $OUT/gpu_tests.log 2>&1
rc=$?
tail -30 $OUT/gpu_tests.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest exit $rc: stopping"; exit $rc; fi
timeout -k 10 600 python bench.py --full "$@" > $OUT/bench.json 2> $OUT/bench.err
brc=$?
cat $OUT/bench.json
tail -5 $OUT/bench.err
[ $brc -ne 0 ] && exit $brc
exit $rc
