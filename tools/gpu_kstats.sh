#!/bin/bash
# Kernel-trace stats per library build: tools/gpu_kstats.sh <lib.so|default>...
# -> $OUT/ks_<name>/ (rocprofv3 --stats) and $OUT/kstats.txt
set -o pipefail
OUT=${OUT:-bench_out}
export TMPDIR=/tmp
mkdir -p $OUT; rm -f $OUT/kstats.txt
for lib in "$@"; do
  name=$(basename $lib .so); name=${name#libcip_hip_}
  if [ "$lib" = default ]; then unset CIP_HIP_LIB; else export CIP_HIP_LIB=$PWD/$lib; fi
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $PWD/$OUT/ks_$name -o ks --output-format csv \
    -- python3 bench.py --full --steps ${STEPS:-5} --warmup 3 --no-cpu-baseline ${BENCH_ARGS:---sync} > $OUT/ks_$name.json 2> $OUT/ks_$name.err || exit 1
  python3 tools/kstats.py $name $OUT/ks_$name >> $OUT/kstats.txt || exit 1
done
