#!/bin/bash
# rocprofv3 kernel-trace summary of a short bench run (separate from PMC passes).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT=${OUT:-bench_out}  # where this script writes its logs
mkdir -p $OUT/prof
export TMPDIR=/tmp
STEPS=${STEPS:-20}
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run \
    -- python bench.py --full --steps $STEPS --warmup 5 --no-cpu-baseline --no-kernel-timing \
    > $OUT/prof/bench_prof.log 2>&1
rc=$?
tail -2 $OUT/prof/bench_prof.log
find $OUT/prof -name "*stats*" | head
exit $rc
