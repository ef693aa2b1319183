#!/bin/bash
# Configs B and D through bench.py --full: with the CPU baselines.
# Tag = $1; results go to $SGN_OUT (default: bench_out).
set -u
T=${1:-x}
O=${SGN_OUT:-bench_out}
mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 400 python -u bench.py --full --workload B > $O/benchB_$T.json 2> $O/benchB_$T.err
rc=$?; echo "BENCH_B $rc"; cat $O/benchB_$T.json | cut -c1-400; [ $rc -eq 0 ] || exit $rc
timeout -k 10 600 python -u bench.py --full --workload D --steps 5 --warmup 2 --cpu-budget-s 8 > $O/benchD_$T.json 2> $O/benchD_$T.err
rc=$?; echo "BENCH_D $rc"; cat $O/benchD_$T.json | cut -c1-400; tail -3 $O/benchD_$T.err; exit $rc
