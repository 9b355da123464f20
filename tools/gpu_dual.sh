#!/bin/bash
# Dual-kite (config 3) GPU session: parity tests, then a short bench with only the dual block.
# Every GPU step has its own time limit; exit codes other than 0/1 end the script.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT="${AWE_OUT:-out}"   # the folder this script writes to
mkdir -p $OUT
export TMPDIR=/tmp
run() {
    local limit=$1 log=$2; shift 2
    echo "=== $* (limit ${limit}s)" | tee -a $OUT/steps.log
    timeout -k 10 "$limit" "$@" > "$OUT/$log" 2>&1
    local rc=$?
    echo "=== rc=$rc" | tee -a $OUT/steps.log
    tail -5 "$OUT/$log"
    if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "stopping after rc=$rc"; exit $rc; fi
    return 0
}
STAGES=${STAGES:-"test bench"}
for s in $STAGES; do
  case $s in
    test)  run 600 dual_tests.log python -u -m pytest tests/test_dual_gpu.py -x -v --timeout 300 --timeout-method thread ;;
    bench) run 300 dual_bench.log python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-hessian --mpc-batch 0 --sweep-points 0 ${BENCH_ARGS} ;;
    prof)  run 300 dual_rocprof.log rocprofv3 --kernel-trace --stats -d $OUT/dprof -o run --output-format csv -- python bench.py --full --steps 5 --warmup 1 --no-cpu-baseline --no-hessian --mpc-batch 0 --sweep-points 0 ${BENCH_ARGS} && \
           find $OUT/dprof -name '*_trace.csv' -size +4M -delete ;;
  esac
done
echo ALL_DONE
