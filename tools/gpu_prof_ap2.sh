#!/bin/bash
# rocprof kernel-trace stats of the bench's AP2 block alone (no sweep, no batch-1 latency launches)
cd "${GRAFT_REPO_ROOT:-.}"
export OUT="${AWE_OUT:-out}"   # the folder this script writes to
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_ap2b -o run --output-format csv -- python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --dual-batch 0 --mpc-batch 0 --pmpc-loops 0 --sweep-points 0 --dual-sweep-points 0 --no-hessian --no-latency > $OUT/rocprof_ap2b.log 2>&1 || exit $?
find $OUT/prof_ap2b -name '*_trace.csv' -size +4M -delete
echo PROF_DONE
# the config-4 dual sweep block alone (8 points, fan mode) under the kernel tracer
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_dualsweep -o run --output-format csv -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --dual-batch 0 --mpc-batch 0 --pmpc-loops 0 --sweep-points 0 --no-hessian --no-latency > $OUT/rocprof_dualsweep.log 2>&1 || exit $?
find $OUT/prof_dualsweep -name '*_trace.csv' -size +4M -delete
echo DUAL_PROF_DONE
