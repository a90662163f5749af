#!/bin/bash
# Graph-step session: new graph tests + network tests, then eager and graph bench lines.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT=${OUT:-bench_out}  # where this script writes its logs
mkdir -p $OUT
timeout -k 10 600 python -m pytest tests/test_gpu_graph.py tests/test_gpu_network.py tests/test_gpu_raymarching.py -q -p no:cacheprovider --timeout 300 -x \
    > $OUT/pytest_graph.log 2>&1
rc=$?
tail -15 $OUT/pytest_graph.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest crashed rc=$rc"; exit $rc; fi
timeout -k 10 300 python bench.py --full --steps 30 --warmup 10 --no-cpu-baseline > $OUT/bench_graph.log 2>&1 || { echo "graph bench failed"; tail -30 $OUT/bench_graph.log; exit 3; }
tail -1 $OUT/bench_graph.log
timeout -k 10 300 python bench.py --full --steps 30 --warmup 10 --no-cpu-baseline --eager > $OUT/bench_eager.log 2>&1 || { echo "eager bench failed"; tail -30 $OUT/bench_eager.log; exit 3; }
tail -1 $OUT/bench_eager.log
exit $rc
