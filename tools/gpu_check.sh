#!/bin/bash
# GPU-box check: smoke, GPU parity tests, short bench, kernel-trace profile.
# Every GPU step has its own time limit; a fault/abort/timeout ends the script.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
ok() { [ "$1" -eq 0 ] || [ "$1" -eq 1 ]; }
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; ok $rc || exit $rc
timeout -k 10 600 python -m pytest tests -m gpu -q -rf > $OUT/pytest_gpu.log 2>&1
rc=$?; echo "pytest rc=$rc"; ok $rc || exit $rc
timeout -k 10 400 python bench.py --full ${BENCH_ARGS:-} > $OUT/bench.log 2>&1
rc=$?; echo "bench rc=$rc"; [ $rc -eq 0 ] || exit $rc
if [ -n "${PROFILE:-}" ]; then
  bash tools/profile.sh; exit $?
fi
