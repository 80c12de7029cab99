#!/bin/bash
# One GPU session: parity tests, smoke, bench, kernel-trace profile (summary
# over the bench's 10 profiled, synchronous calls after its timed region).
# Every GPU step has its own time limit; steps are chained with && so the
# first failure (fault, abort, timeout) ends the session.
set -o pipefail
OUT=gpurun_out
mkdir -p $OUT
export TMPDIR=/tmp
ROUND=${ROUND:-r01}
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 && echo "pytest ok" &&
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 && echo "smoke ok" &&
timeout -k 10 600 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err && echo "bench ok" &&
timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $PWD/$OUT/prof -o $ROUND --output-format csv -- \
    python3 bench.py --full --no-cpu-baseline > $OUT/bench_prof.json 2> $OUT/bench_prof.err && echo "prof ok" &&
python3 tools/trace_summary.py $OUT/prof/${ROUND}_kernel_trace.csv 10 $OUT/${ROUND}_kernel_summary.md > /dev/null
