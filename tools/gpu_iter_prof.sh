#!/bin/bash
# Iteration loop: the given GPU test files, then a rocprofv3 kernel-trace of a
# short bench run, summarised to $OUT/prof/top.txt.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT=${OUT:-bench_out}  # where this script writes its logs
mkdir -p $OUT/prof
export TMPDIR=/tmp
TESTS=${TESTS:-tests}
timeout -k 10 400 python -u -m pytest $TESTS -x -q -p no:cacheprovider -m gpu --timeout 120 --timeout-method thread > $OUT/pt_iter.log 2>&1
rc=$?
tail -5 $OUT/pt_iter.log
if [ $rc -ne 0 ]; then echo "pytest rc=$rc"; exit $rc; fi
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -o run \
    -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-kernel-timing ${BENCH_ARGS:-} \
    > $OUT/prof/bench_prof.log 2>&1 || { echo "prof failed"; tail -20 $OUT/prof/bench_prof.log; exit 3; }
grep '^{' $OUT/prof/bench_prof.log | python -c "import json,sys; d=json.loads(sys.stdin.read()); print('ms/step', d['ms_per_step'], 'infer ms', d.get('inference',{}).get('ms_per_frame'))"
python tools/prof_top.py $OUT/prof/run_kernel_stats.csv 25 > $OUT/prof/top.txt
cat $OUT/prof/top.txt
