#!/bin/bash
# One GPU session: parity tests, smoke, bench.  Stops at the first crash /
# timeout (exit codes other than 0/1 from pytest), never retries.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT=${OUT:-bench_out}  # where this script writes its logs
mkdir -p $OUT
STEPS=${STEPS:-30}
timeout -k 10 900 python -m pytest tests -m gpu -q -p no:cacheprovider --timeout 300 "$@" \
    > $OUT/pytest_gpu.log 2>&1
rc=$?
tail -5 $OUT/pytest_gpu.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest crashed rc=$rc"; exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1
src=$?
tail -3 $OUT/smoke.log
if [ $src -ne 0 ]; then echo "smoke failed rc=$src"; exit $src; fi
timeout -k 10 600 python bench.py --full --steps $STEPS --warmup 10 > $OUT/bench.log 2>&1
brc=$?
tail -2 $OUT/bench.log
exit $(( rc > brc ? rc : brc ))
