"""The premises of the run-control sweep (tests/test_gpu_runctl_fuzz.py), checked on the CPU against
the oracle alone: that the drawn programs really save in mid-run and rewind over real work, pause
inside the run, cover every knob and operation; that the trace-cursor model reproduces the documented
scenario of test_take_rewind; that the comparers fail when they should; and that the train-merge
cases save at an edge where the server holds a cached packet. These are conditions on the draw
(tests/runctl_model.py): a draw that misses one is changed, never the condition.

"Save and rewind" is read per case: every default case has at least one save at a round whose window
is still active that a later restore rewinds to over at least 10 rounds and 200 popped packet events
(the closing pair of every program is built to be one).

SGN_RUNCTL_COVERAGE=<file> writes the coverage table there (profiles/runctl/coverage.txt is that
file for the default counts); it is printed either way.
"""
import os

import numpy as np
import pytest

import sgn
from runctl_model import (KINDS, S0, TraceLedger, assert_state, cached_edges, cached_round, check_take, draw_case,
                          only, oracle_rounds, resolve, same_records, srt)
from test_gpu_parity import scenario
from test_gpu_train_merge import CASES, world

N_SINGLE = int(os.environ.get("SGN_RUNCTL_CASES", "32"))
N_SHARD = int(os.environ.get("SGN_RUNCTL_SHARD_CASES", "12"))
SET6 = [3, 63, 64, 65, 127, 199]


def case_args(case):
    args = scenario(**case["kw"])
    args[3].event_capacity = 1 << 23
    return args


def rewinds(steps, ref):
    """The (save round, rounds rewound, packet events popped over them) of every restore that took
    effect and went back to a save made while the window was active."""
    R = len(ref["windows"]) - 1
    popped = [s[1]["packet_events_popped"] for s in ref["states"]]
    saved, out, at = {}, [], 0
    for st in steps:
        op = st["op"]
        if op[0] == "save":
            saved[op[1]] = st["round"]
        elif op[0] == "restore" and not st["refused"] and saved[op[1]] < R and at > saved[op[1]]:
            out.append((saved[op[1]], at - saved[op[1]], popped[at] - popped[saved[op[1]]]))
        at = st["round"]
    return out


@pytest.fixture(scope="module")
def single(oracle):
    """Every default case of test_program_single: the case, the oracle's rounds, the resolved steps."""
    out = []
    for i in range(N_SINGLE):
        case = draw_case(i)
        ref = oracle_rounds(oracle, case_args(case), case["trace"])
        ledger = TraceLedger(ref["trace"], ref["lens"], case["hosts"]) if case["trace"] else None
        out.append((case, ref, resolve(case["program"], ref["windows"], ref["stop"], ledger)))
    return out


@pytest.fixture(scope="module")
def sharded(oracle):
    out = []
    for i in range(N_SHARD):
        case = draw_case(i, trace=False)
        ref = oracle_rounds(oracle, case_args(case), False)
        out.append((case, ref, resolve(case["program"], ref["windows"], ref["stop"])))
    return out


def test_draw_follows_the_fuzz_and_is_stable():
    from test_gpu_fuzz import draw
    for i in (0, 7, 31):
        kw, env, trace = draw(i)
        case = draw_case(i)
        assert case["env"] == env and case["trace"] == trace and case["kw"]["seed"] == kw["seed"]
        again = draw_case(i)
        assert again["program"] == case["program"] and again["hosts"] == case["hosts"]
        prog = case["program"]
        assert 6 <= len(prog) - (2 if trace else 1) <= 12, prog
        assert prog[-1] == ("take",) if trace else prog[-1] == ("run", None)
        assert all(op[0] not in ("take", "take_small") for op in draw_case(i, trace=False)["program"])
        if trace:
            assert all(op[0] != "fresh" for op in prog)
        if case["hosts"] is not None:
            n = kw["n"]
            assert 0 in case["hosts"] and n - 1 in case["hosts"] and 2 <= len(case["hosts"]) <= 8
            assert len(set(case["hosts"])) == len(case["hosts"]) and max(case["hosts"]) < n


@pytest.mark.parametrize("which", ["single", "sharded"])
def test_save_rewind_and_pause_in_every_case(single, sharded, which):
    for i, (case, ref, steps) in enumerate(single if which == "single" else sharded):
        R = len(ref["windows"]) - 1
        assert steps[-1 - bool(case["trace"])]["round"] == R, i
        good = [x for x in rewinds(steps, ref) if x[1] >= 10 and x[2] >= 200]
        assert good, (which, i, rewinds(steps, ref), R)
        pauses = [st for st in steps if st["op"][0] == "run_until" and st["ret"] > 0 and st["round"] < R]
        assert pauses, (which, i, R)
        for st in steps:  # run_until: never a multiple of 1 ms; a target at or below the window runs nothing
            if st["op"][0] == "run_until":
                assert (st["t"] - S0) % 1_000_000 != 0 or st["t"] == S0, st
                if st["op"][2]:
                    assert st["ret"] == 0, st


def _features(case):
    kw, env = case["kw"], case["env"]
    f = {"SGN_PERSISTENT=" + env["SGN_PERSISTENT"], "SGN_HOSTS_PER_WAVE=" + env["SGN_HOSTS_PER_WAVE"],
         "TGEN" if kw["kind"] == sgn.TRAFFIC_TGEN else "PERIODIC", "fifo=%d" % kw["fifo"], "codel=%d" % kw["codel"]}
    for k in ("SGN_SLAB_CAP", "SGN_HOST_ORDER", "SGN_PEER64"):
        if k in env:
            f.add(k + "=" + env[k])
    if kw["qdisc"] == sgn.QDISC_ROUND_ROBIN:
        f.add("round-robin qdisc")
    if kw["dynamic"]:
        f.add("dynamic=True")
    if kw["bootstrap_ns"] > 0:
        f.add("bootstrap_ns>0")
    if case["trace"]:
        f.add("traced, host set" if case["hosts"] is not None else "traced, all hosts")
    return f


ROWS = ("SGN_PERSISTENT=0", "SGN_PERSISTENT=1", "SGN_SLAB_CAP=16", "SGN_HOST_ORDER=id", "SGN_PEER64=1",
        "SGN_HOSTS_PER_WAVE=16", "round-robin qdisc", "dynamic=True", "bootstrap_ns>0", "fifo=2", "codel=160",
        "TGEN", "PERIODIC", "traced, host set", "traced, all hosts")


def test_coverage_over_the_default_cases(single, sharded):
    hits = {row: [] for row in ROWS}
    kinds = {k: 0 for k in KINDS}
    refused = forward = 0
    for i, (case, ref, steps) in enumerate(single):
        if any(x[1] >= 10 and x[2] >= 200 for x in rewinds(steps, ref)):
            for row in _features(case) & set(ROWS):
                hits[row].append(i)
        at = 0
        for st in steps:
            kinds[st["op"][0]] += 1
            refused += st["refused"]
            forward += st["op"][0] == "restore" and not st["refused"] and st["round"] > at
            at = st["round"]
    lines = ["run-control sweep: coverage of the default cases (%d single, %d sharded)" % (N_SINGLE, N_SHARD),
             "knob, with a save / rewind pair over >= 10 rounds and >= 200 popped events: cases"]
    lines += ["  %-22s %2d  %s" % (row, len(hits[row]), " ".join(map(str, hits[row]))) for row in ROWS]
    lines += ["operations over the single cases:"] + ["  %-22s %3d" % (k, kinds[k]) for k in KINDS]
    lines.append("  restores forward      %3d   traced restores / exports refused (records no longer held) %d" % (forward, refused))
    sk = {k: sum(st["op"][0] == k for _, _, steps in sharded for st in steps) for k in KINDS[:6]}
    lines += ["operations over the sharded cases:"] + ["  %-22s %3d" % (k, sk[k]) for k in sk]
    lines.append("rounds per case (single): " + " ".join(str(len(ref["windows"]) - 1) for _, ref, _ in single))
    text = "\n".join(lines) + "\n"
    print("\n" + text)
    if os.environ.get("SGN_RUNCTL_COVERAGE"):
        with open(os.environ["SGN_RUNCTL_COVERAGE"], "w") as f:
            f.write(text)
    if N_SINGLE >= 32:
        assert all(hits[row] for row in ROWS), {row: hits[row] for row in ROWS if not hits[row]}
        assert all(v >= 5 for v in kinds.values()), kinds
    if N_SHARD >= 12:
        assert all(v >= 5 for v in sk.values()), sk


def test_ledger_on_the_documented_scenario(oracle):
    """test_take_rewind's sequence on its scenario: save@150, run 100, take, restore, run 100, take,
    run 50, save, run 60, restore, run, take."""
    ref = oracle_rounds(oracle, scenario(), True, every_state=False)
    t = only(srt(ref["trace"]), SET6)
    program = [("run", 150), ("save", "a"), ("run", 100), ("take",), ("restore", "a"), ("run", 100), ("take",),
               ("run", 50), ("save", "b"), ("run", 60), ("restore", "b"), ("run", None), ("take",)]
    L = TraceLedger(ref["trace"], ref["lens"], SET6)
    steps = resolve(program, ref["windows"], ref["stop"], L)
    assert [s["round"] for s in steps[:11]] == [150, 150, 250, 250, 150, 250, 250, 300, 300, 360, 300]
    assert not any(s["refused"] for s in steps)
    first, second, last = steps[3]["take"], steps[6]["take"], steps[12]["take"]
    pre = len(L.produced(150))
    assert pre > 0 and steps[1]["pending"] == pre and len(first) == steps[2]["pending"] > pre
    assert steps[4]["pending"] == 0  # the take had passed the save: the cursor went back with it
    assert len(second) == len(first) - pre > 0
    same_records(srt(np.concatenate([L.produced(150), second])), first, "the second take is the first from round 150 on")
    assert steps[10]["pending"] == steps[8]["pending"] > 0 and steps[9]["pending"] > steps[8]["pending"]
    same_records(srt(np.concatenate([first, last])), t, "first + last")
    for take in (first, second, last):
        hs, cnt = np.unique(take["host"], return_counts=True)
        spans = np.zeros(len(hs), sgn.SPAN_DTYPE)
        spans["host"], spans["count"] = hs, cnt
        spans["first"] = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        check_take(take, spans, SET6)


def test_ledger_refuses_what_the_buffer_no_longer_holds(oracle):
    """A snapshot ahead of the position whose records left the buffer: after a rewind and a take the
    later save can be neither restored nor exported; after running past it again it can."""
    ref = oracle_rounds(oracle, scenario(n=60, V=10, stop_ns=60_000_000), True, every_state=False)
    program = [("run", 20), ("save", "a"), ("run", 20), ("save", "b"), ("restore", "a"), ("restore", "b"),
               ("restore", "a"), ("take",), ("restore", "b"), ("export_import", "b"), ("run", 30),
               ("export_import", "b"), ("restore", "b"), ("run", None), ("take",)]
    L = TraceLedger(ref["trace"], ref["lens"])
    steps = resolve(program, ref["windows"], ref["stop"], L)
    assert [s["refused"] for s in steps] == [False] * 8 + [True, True] + [False] * 5
    assert [s["round"] for s in steps[:13]] == [20, 20, 40, 40, 20, 40, 20, 20, 20, 20, 50, 50, 40]
    same_records(srt(np.concatenate([steps[7]["take"], steps[14]["take"]])), srt(ref["trace"]), "every record once")


def test_comparers_fail_when_they_should(oracle):
    ref = oracle_rounds(oracle, scenario(n=60, V=10, stop_ns=30_000_000), True, every_state=False)
    good = ref["states"][-1]
    assert_state(good, good, "same")
    dig = good[2].copy()
    dig["rng"][17, 2] ^= 1 << 40
    with pytest.raises(AssertionError):
        assert_state((good[0], good[1], dig), good, "one digest word of one host")
    st = dict(good[1])
    st["delivered"] += 1
    with pytest.raises(AssertionError):
        assert_state((good[0], st, good[2]), good, "one counter")
    with pytest.raises(AssertionError):
        assert_state(((good[0][0] + 1,) + good[0][1:], good[1], good[2]), good, "the window")
    t = srt(ref["trace"])
    same_records(t, t)
    k = int(np.nonzero(t["host"] == 5)[0][3])
    assert t["host"][k + 1] == 5
    bad = t.copy()
    bad[[k, k + 1]] = bad[[k + 1, k]]
    with pytest.raises(AssertionError):
        same_records(bad, t, "two records of one host swapped")
    hs, cnt = np.unique(t["host"], return_counts=True)
    spans = np.zeros(len(hs), sgn.SPAN_DTYPE)
    spans["host"], spans["count"], spans["first"] = hs, cnt, np.concatenate([[0], np.cumsum(cnt)[:-1]])
    check_take(t, spans)
    with pytest.raises(AssertionError):
        check_take(bad, spans)


@pytest.mark.parametrize("name", ["plain_100M", "cached_last_then_other_train"])
def test_train_merge_save_round_holds_a_cached_packet(oracle, name):
    from test_gpu_train_merge import MSS, server_sends
    ref = oracle_rounds(oracle, world(**CASES[name]), True, every_state=False)
    t, w = srt(ref["trace"]), ref["windows"]
    r = cached_round(name, t, w)
    assert 0 < r and r + 5 < len(w) - 1
    tp, ts, _, pay, _ = server_sends(t)
    held = np.nonzero((tp <= w[r]) & (ts > w[r]))[0]
    assert len(held) >= 1, (name, r)
    assert (r, int(pay[held[0]])) in cached_edges(t, w)
    if name == "cached_last_then_other_train":
        assert int(pay[held[0]]) == CASES[name]["file_bytes"] % MSS  # the train's short last packet
    assert ref["states"][-1][1]["packet_events_popped"] > 0
