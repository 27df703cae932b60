#!/bin/bash
# Device assembly of kmeans.hip (narrow and wide build) and unique.hip with _build.py's flags, comment
# lines stripped, for comparing two trees:
#   profiles/km_variants_retired/asm.sh <tree> <outdir>
# writes <outdir>/{kmeans,kmeans_wide,unique}.s and .remarks (kernel-resource-usage).
set -eu -o pipefail
tree=$1 out=$2
mkdir -p "$out"
common="-O3 -fPIC -std=c++17 -ffp-contract=off -I$tree/include -Wall -Wno-unused-function -Wno-unused-variable -x hip --offload-arch=gfx950"
ilp="-mllvm -amdgpu-sched-strategy=iterative-ilp"
csrc=$tree/low_level_feature_extraction_amd/csrc
one() {  # stem, source, extra flags
    local stem=$1 src=$2
    shift 2
    hipcc $common "$@" --cuda-device-only -S -Rpass-analysis=kernel-resource-usage "$csrc/$src" -o "$out/$stem.raw.s" 2> "$out/$stem.remarks"
    # (__hip_cuid_<hash> is a one-byte object named by a hash of the source text: no device code)
    grep -v '^[[:space:]]*;' "$out/$stem.raw.s" | sed -e 's/__hip_cuid_[0-9a-f]*/__hip_cuid/g' > "$out/$stem.s"
}
one kmeans kmeans.hip $ilp & a=$!
one kmeans_wide kmeans.hip $ilp -DLLFE_KM_WIDE=1 -DLLFE_KM_THREADS=512 -DLLFE_KM_UNROLL=4 & b=$!
one unique unique.hip & c=$!
wait $a && wait $b && wait $c
