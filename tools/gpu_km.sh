#!/bin/bash
# GPU box: k-means checks (incremental vs full sweeps, oracle parity, pipeline), the
# per-attempt k-means timeline, then one full bench line without the CPU baseline.
# Outputs under $OUT (LLFE_OUT, default bench_out/).
set -u -o pipefail
OUT=${LLFE_OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 400 python -u -m pytest tests/test_gpu_kmeans_inc.py tests/test_gpu_parity.py tests/test_gpu_pipeline.py -m gpu -x -v --timeout 120 --timeout-method thread -p no:cacheprovider > $OUT/gpu_km_tests.log 2>&1
rc=$?
tail -12 $OUT/gpu_km_tests.log
if [ $rc -ne 0 ]; then echo "pytest exit $rc: stopping"; exit $rc; fi
bash tools/km_trace.sh || exit 1
timeout -k 10 300 python bench.py --full --cpu-baseline off > $OUT/bench_km.json 2> $OUT/bench_km.err || exit 1
python3 - $OUT/bench_km.json <<'PY'
import json, sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], {k: (v['avg_ms'], v.get('isolated_ms')) for k, v in d['kernels'].items()})
PY
