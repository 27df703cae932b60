set -u -o pipefail
OUT=${LLFE_OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 600 python bench.py --full > $OUT/full.json 2> $OUT/full.err || { tail -5 $OUT/full.err; exit 1; }
python3 - $OUT/full.json <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"])
print("png", d["e2e_png"])
print("jpeg", d["e2e_jpeg"])
print("host", d["e2e_host"]["value"], "cpu", d["cpu_baseline"]["value"], d["cpu_baseline"]["cores"])
print(d["per_class"])
PY
