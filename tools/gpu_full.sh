#!/bin/bash
# GPU box: GPU test suite, one default bench line (CPU baseline included), then the
# rocprofv3 kernel-trace + PMC traffic profile (tools/profile.sh TAG).
# Outputs under $OUT (LLFE_OUT, default bench_out/).
set -u -o pipefail
TAG=${1:-run}
OUT=${LLFE_OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread -p no:cacheprovider > $OUT/gpu_tests.log 2>&1
rc=$?
tail -15 $OUT/gpu_tests.log
if [ $rc -ne 0 ]; then echo "pytest exit $rc: stopping"; exit $rc; fi
timeout -k 10 600 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
brc=$?
head -c 3000 $OUT/bench_$TAG.json; echo
tail -3 $OUT/bench_$TAG.err
if [ $brc -ne 0 ]; then echo "bench exit $brc: stopping"; exit $brc; fi
bash tools/profile.sh $TAG
