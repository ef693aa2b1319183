"""Run-control for sharded simulations, the ranks form (-m gpu): two fresh processes, each one
shard with an RCCL communicator on device 0 (bench.py --one-gpu's environment: RCCL's socket
transport), make the collective calls with n = 1 — sgn_shards_run_until, save, run to the end,
restore, run to the end (tests/shard_ranks_runner.py) — in both exchange modes: per-round launches
with the RCCL send/recv and k_import (mode 1), and k_rounds_x with the peer's inbox mapped
(mode 2, SGN_XPEER_SHARED=1). Both passes are compared, bit for bit, with the oracle's once-stepped
run of test_gpu_snapshot.until_ref("periodic"): its mid-run mark and its end.

A rank's run time is RCCL's start-up: measured on an MI355X box, a rank has its communicator
2.0 s after its start (6.3 s in the first pair of processes on a box) and is done 0.06 s later —
the simulation and the five collective calls take 60 ms of a rank's 2.1 to 6.4 s. Each process
gets RANK_TIMEOUT_S = 90 s, fourteen times the slowest start seen; when one rank fails or runs out
of time the other is killed and nothing more is started."""
import pathlib
import subprocess
import sys
import time

import numpy as np
import pytest

from test_gpu_snapshot import S0, assert_state, state, until_ref  # noqa: F401
from test_gpu_xpersist import ADD, DIGESTS

pytestmark = pytest.mark.gpu
HERE = pathlib.Path(__file__).resolve().parent
RANK_TIMEOUT_S = 90.0
EINVAL = -22


def run_ranks(tmp_path, targets, shared):
    """One process per target (rank order); returns their result files."""
    import os
    env = dict(os.environ, NCCL_DEBUG="WARN", TMPDIR="/tmp", SGN_GRAPH="0")
    env.pop("SGN_XPEER_SHARED", None)
    env.pop("SGN_LOCAL_PERSIST", None)
    if shared:
        env["SGN_XPEER_SHARED"] = "1"
    world = len(targets)
    procs, logs = [], []
    for r, t in enumerate(targets):
        log = open(tmp_path / f"rank{r}.log", "w")
        logs.append(log)
        procs.append(subprocess.Popen([sys.executable, "-u", str(HERE / "shard_ranks_runner.py"), str(r), str(world),
                                       str(tmp_path), str(t)], env=env, stdout=log, stderr=subprocess.STDOUT))
    deadline = time.monotonic() + RANK_TIMEOUT_S  # (all start together: each rank's own limit)
    failed = None
    left = set(range(world))
    while left and failed is None:
        for r in sorted(left):
            try:
                rc = procs[r].wait(timeout=0.1)
            except subprocess.TimeoutExpired:
                if time.monotonic() > deadline:
                    failed = (r, "timeout")
                    break
                continue
            left.discard(r)
            if rc != 0:
                failed = (r, rc)
                break
    for p in procs:  # a failed or late rank: the others are stopped, nothing more is started
        if p.poll() is None:
            p.kill()
            p.wait()
    for log in logs:
        log.close()
    if failed is not None:
        text = "\n".join(f"--- rank {r}\n" + (tmp_path / f"rank{r}.log").read_text()[-3000:] for r in range(world))
        pytest.fail(f"rank {failed[0]}: {failed[1]}\n{text}")
    return [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]


def merged(res, tag):
    wins = [tuple(int(v) for v in r[tag + "_window"]) for r in res]
    assert all(w == wins[0] for w in wins), wins
    sts = [r[tag + "_stats"] for r in res]
    assert all(int(s[0]) == int(sts[0][0]) for s in sts)
    st = {"rounds": int(sts[0][0])}
    for i, key in enumerate(ADD):
        st[key] = sum(int(s[1 + i]) for s in sts)
    assert [int(r["lo"]) for r in res[1:]] == [int(r["hi"]) for r in res[:-1]]
    w = wins[0]
    return (w[0], w[1], bool(w[2])), st, {f: np.concatenate([r[tag + "_" + f] for r in res]) for f in DIGESTS}


def assert_merged(got, ref, what):
    assert_state(got, (ref[0], {k: ref[1][k] for k in got[1]}, ref[2]), what)


@pytest.mark.parametrize("shared", [False, True])
def test_two_ranks_console_sequence(oracle, tmp_path, shared):
    args, o, marks = until_ref(oracle, "periodic")
    n = args[2].n
    t_mid, r_mid, at_mid = marks[1]
    res = run_ranks(tmp_path, [t_mid, t_mid], shared)
    print("communicator start-up per rank (s):", [float(r["t_comm"]) for r in res], "whole rank:",
          [float(r["t_total"]) for r in res])
    assert all(int(r["rc"]) == 0 for r in res)
    assert all(int(r["done_mid"]) == r_mid and int(r["snap_rounds"]) == r_mid for r in res)
    end = state(o, n)
    assert_merged(merged(res, "mid"), at_mid, "paused")
    assert_merged(merged(res, "end1"), end, "first pass")
    assert_merged(merged(res, "back"), at_mid, "restored")
    assert_merged(merged(res, "end2"), end, "second pass")
    if shared:  # k_rounds_x across the two processes: its pause compare and the inbox reset ran
        assert all(int(r["exchange_mode"]) == 2 and int(r["persistent_x_launches"]) > 0 for r in res)
    else:
        assert all(int(r["exchange_mode"]) == 1 for r in res)


def test_two_ranks_different_targets_are_refused(oracle, tmp_path):
    args, o, marks = until_ref(oracle, "periodic")
    t_mid = marks[1][0]
    res = run_ranks(tmp_path, [t_mid, t_mid + 1], False)
    assert all(int(r["rc"]) == EINVAL for r in res), [int(r["rc"]) for r in res]
