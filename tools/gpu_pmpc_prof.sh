#!/bin/bash
# kernel-trace statistics of the bench's converged-MPC block alone (64 loops)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
export OUT="${AWE_OUT:-out}"   # the folder this script writes to
mkdir -p $OUT
export TMPDIR=/tmp
timeout -s KILL 400 rocprofv3 --kernel-trace --stats -d $OUT/pmpc_prof -o run --output-format csv -- python -u bench.py --full --steps 1 --warmup 0 --batch 8 --no-cpu-baseline --no-hessian --no-latency --dual-batch 0 --mpc-batch 64 --pmpc-loops 64 --sweep-points 0 --dual-sweep-points 0 > $OUT/pmpc_prof.log 2>&1 || exit 1
find $OUT/pmpc_prof -name '*_trace.csv' -size +4M -delete
tail -c 400 $OUT/pmpc_prof.log
