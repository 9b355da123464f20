#!/bin/bash
# Round-end check on the final sources in one call: GPU suite, smoke, default bench, rocprof stats of
# the bench's AP2 block alone and of its AP2 sweep block alone.  A failure ends the script.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT="${AWE_OUT:-out}"   # the folder this script writes to
mkdir -p $OUT
export TMPDIR=/tmp
step() {  # step <limit> <log> <cmd...>
    local limit=$1 log=$2; shift 2
    timeout -k 10 "$limit" "$@" > "$OUT/$log" 2>&1
    local rc=$?
    echo "=== $log rc=$rc"; tail -2 "$OUT/$log" | cut -c1-300
    if [ $rc -ne 0 ]; then exit $rc; fi
}
step 600 pytest_gpu.log python -u -m pytest tests -m gpu -x -v --timeout 400 --timeout-method thread --durations=15
step 120 smoke.log python -c "import __graft_entry__ as g; g.smoke()"
step 260 bench.log python bench.py --full
step 80 rocprof_ap2.log rocprofv3 --kernel-trace --stats -d $OUT/prof_ap2 -o run --output-format csv -- python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --dual-batch 0 --mpc-batch 0 --sweep-points 0 --dual-sweep-points 0 --no-hessian --no-latency
find $OUT/prof_ap2 -name '*_trace.csv' -size +4M -delete
step 90 rocprof_sweep.log rocprofv3 --kernel-trace --stats -d $OUT/prof_sweep -o run --output-format csv -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --dual-batch 0 --mpc-batch 0 --pmpc-loops 0 --dual-sweep-points 0 --no-hessian
find $OUT/prof_sweep -name '*_trace.csv' -size +4M -delete
echo FINAL_DONE
