#!/bin/bash
# One GPU round: parity tests, smoke, bench, rocprofv3 kernel-trace stats.  Every GPU step has its own
# time limit and the steps are chained with && (the first failure ends the call).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-/root/repo}"
export TMPDIR=/tmp
OUT=${OUT:-build/bench}  # where the logs and JSON lines go
mkdir -p $OUT
STEPS=${STEPS:-5}
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 &&
echo "pytest ok" &&
timeout -k 10 180 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1 &&
echo "smoke ok" &&
timeout -k 10 400 python -u bench.py --full --steps $STEPS --warmup 2 > $OUT/bench.json 2> $OUT/bench.err &&
echo "bench ok" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python3 bench.py --full --depth 1 --steps 3 --warmup 1 --no-cpu-baseline --no-configs > $OUT/bench_prof.json 2> $OUT/bench_prof.err &&
echo "rocprof ok"
