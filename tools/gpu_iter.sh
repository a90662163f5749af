#!/bin/bash
# Iteration session: given pytest files ($TESTS), then a graph bench line and a
# rocprofv3 kernel-stats pass.  Stops at the first crash / timeout.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT=${OUT:-bench_out}  # where this script writes its logs
mkdir -p $OUT
TESTS=${TESTS:-tests}
timeout -k 10 500 python -m pytest $TESTS -q -x -p no:cacheprovider -m gpu > $OUT/pt_iter.log 2>&1
rc=$?
tail -12 $OUT/pt_iter.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest crashed rc=$rc"; exit $rc; fi
timeout -k 10 300 python bench.py --full --steps 30 --warmup 10 --no-cpu-baseline > $OUT/bench_graph.log 2>&1 || { echo "bench failed"; tail -20 $OUT/bench_graph.log; exit 3; }
tail -1 $OUT/bench_graph.log | cut -c1-700
bash tools/gpu_prof.sh > /dev/null 2>&1 || { echo "prof failed"; exit 4; }
python3 tools/prof_top.py $OUT/prof/run_kernel_stats.csv 14
exit $rc
