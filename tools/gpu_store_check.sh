#!/bin/bash
# GPU suite (incl. the forced-store parity test), C4 shard bench with max|err| (stores on at 16384^2), strong C4
set -o pipefail
OUT=${OUT:-bench_out}
mkdir -p $OUT
timeout -k 10 500 python -u -m pytest tests -m gpu -x -q --timeout 200 --timeout-method thread > $OUT/store_pytest.log 2>&1 && echo "pytest ok" &&
timeout -k 10 400 python bench.py --full --config c4 --no-cpu-baseline > $OUT/store_c4.json 2> $OUT/store_c4.err && echo "c4 ok" &&
timeout -k 10 400 python bench.py --full --strong --no-cpu-baseline > $OUT/store_strong.json 2> $OUT/store_strong.err && echo "strong ok"
