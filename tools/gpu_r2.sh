#!/bin/bash
# GPU cycle: all -m gpu tests, smoke, bench --full (CPU leg + parity). Tag = $1; results go
# to $SGN_OUT (default: bench_out).
set -u
T=${1:-x}
O=${SGN_OUT:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 600 python -u -m pytest tests -x -v -m gpu --timeout 300 --timeout-method thread > $O/t_$T.log 2>&1
rc=$?; echo "PYTEST $rc"; tail -4 $O/t_$T.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 200 python -u -c "import __graft_entry__ as g; g.smoke()" > $O/smoke_$T.log 2>&1
rc=$?; echo "SMOKE $rc"; tail -2 $O/smoke_$T.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 400 python -u bench.py --full > $O/bench_$T.json 2> $O/bench_$T.err
rc=$?; echo "BENCH $rc"; cat $O/bench_$T.json; tail -3 $O/bench_$T.err; exit $rc
