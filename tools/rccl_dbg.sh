#!/bin/bash
# Debug run of the 2-rank one-GPU RCCL rehearsal (bench --full) with the sgn_run batch trace.
# Tag = $1, then env assignments for the ranks (e.g. SGN_GRAPH=0 SGN_XSZ_INIT=16); results go
# to $SGN_OUT (default: bench_out).
set -u
T=${1:-x}; shift
O=${SGN_OUT:-bench_out}
mkdir -p $O
export TMPDIR=/tmp NCCL_DEBUG=WARN SGN_DEBUG_RUN=1 "$@"
timeout -k 10 100 python -u -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 \
  --master-port 29551 bench.py --gpus 2 --steps 2 --warmup 1 --one-gpu --hosts 20000 --rounds-per-step 70 --full \
  > $O/dbg_$T.json 2> $O/dbg_$T.err
rc=$?; echo "DBG $rc"; grep "\[sgn" $O/dbg_$T.err | tail -30; cat $O/dbg_$T.json | cut -c1-300; exit $rc
