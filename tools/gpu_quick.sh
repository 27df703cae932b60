#!/bin/bash
# GPU box: selected GPU tests (-k expression in $1), then a bench line with extra args
# Outputs under $OUT (LLFE_OUT, default bench_out/).
set -u -o pipefail
OUT=${LLFE_OUT:-bench_out}
mkdir -p $OUT
K=${1:-""}; shift || true
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread -p no:cacheprovider ${K:+-k "$K"} > $OUT/gpu_quick.log 2>&1
rc=$?
tail -25 $OUT/gpu_quick.log
if [ $rc -ne 0 ]; then echo "pytest exit $rc: stopping"; exit $rc; fi
timeout -k 10 600 python bench.py --full --cpu-baseline off --e2e-png-steps 0 --e2e-jpeg-steps 0 --per-class-steps 0 "$@" > $OUT/bench_quick.json 2> $OUT/bench_quick.err
brc=$?
python3 - $OUT/bench_quick.json <<'PY'
import json, sys
try:
    d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
except Exception as e:
    print("no bench json", e); raise SystemExit(0)
print("value", d["value"], "ms/step", d["ms_per_step"])
for k, v in d["kernels"].items():
    print(f'{k:22s} avg {v["avg_ms"]:8.3f} iso {v.get("isolated_ms")}')
print("stencil roofline", d.get("roofline_stencil"))
PY
tail -3 $OUT/bench_quick.err
exit $brc
