#!/bin/bash
# Closing rehearsal on the GPU box: all -m gpu tests, smoke(), bench --full (with its CPU
# leg), rocprofv3 kernel stats of the plain bench, then PMC traffic. Tag = $1; results go to
# $SGN_OUT (default: bench_out).
# Every GPU step has its own time limit; the script stops at the first failure.
set -u
T=${1:-x}
O=${SGN_OUT:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 500 python -u -m pytest tests -x -v -m gpu --timeout 120 --timeout-method thread > $O/t_$T.log 2>&1
rc=$?; echo "PYTEST $rc"; tail -3 $O/t_$T.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$T.log 2>&1
rc=$?; echo "SMOKE $rc"; tail -3 $O/smoke_$T.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python -u bench.py --full > $O/bench_$T.json 2> $O/bench_$T.err
rc=$?; echo "BENCH $rc"; cat $O/bench_$T.json; tail -3 $O/bench_$T.err; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof_$T -o run --output-format csv -- python -u bench.py > $O/prof_$T.log 2>&1
rc=$?; echo "PROF $rc"; [ $rc -eq 0 ] || exit $rc
bash tools/pmc_traffic.sh $T
