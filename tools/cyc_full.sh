#!/bin/bash
# Full measurement cycle: parity, bench --full (with the CPU baseline leg), rocprofv3 stats.
# Tag = $1; results go to $SGN_OUT (default: bench_out).
set -u
T=${1:-x}
O=${SGN_OUT:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 400 python -u -m pytest tests/test_gpu_parity.py -x -q -m gpu --timeout 120 --timeout-method thread > $O/t_$T.log 2>&1
rc=$?; echo "PYTEST $rc"; tail -2 $O/t_$T.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python -u bench.py --full > $O/bench_$T.json 2> $O/bench_$T.err
rc=$?; echo "BENCH $rc"; cat $O/bench_$T.json; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_$T -o run --output-format csv -- python -u bench.py > $O/prof_$T.log 2>&1
rc=$?; echo "PROF $rc"; cat $O/prof_$T/run_kernel_stats.csv | cut -c1-150; exit $rc
