"""Randomised run-control sweep (-m gpu): seeded programs of pauses (sgn_run_until), saves, rewinds,
snapshot-file round trips, moves into a fresh context and trace takes (tests/runctl_model.py) over
the scenarios of test_gpu_fuzz.draw — every traffic kind, runahead mode, queue size, qdisc and layout
knob the fuzz mixes, which the fixed scenarios of the run-control tests never save.

The engine is bit-deterministic and the oracle is never paused: it is stepped once, a round at a
time, and whatever a program does, after EVERY operation the context must stand exactly on the
oracle's state at the round edge the model resolves (window, counters, all nine digest fields), the
running calls must report the resolved round counts, every take must be the model's records field
by field, and the end must be the oracle's end. The model's premises — that the programs save in
mid-run, rewind over real work and cover every knob — are checked on the CPU in
tests/test_runctl_model.py. A failing case names its number: the plain fuzz case of that number is
the same scenario run straight through.
"""
import os

import numpy as np
import pytest

import sgn
from runctl_model import (TraceLedger, assert_state, cached_round, check_take, draw_case, only, oracle_rounds,
                          resolve, same_records, srt, state)
from test_gpu_parity import assert_same_run, scenario
from test_gpu_shard_control import assert_merged, check_mode, group, merged, run_group, set_persist
from test_gpu_train_merge import CASES as TRAIN_CASES
from test_gpu_train_merge import world

pytestmark = pytest.mark.gpu

ESTATE = -71
CASES = int(os.environ.get("SGN_RUNCTL_CASES", "32"))
SHARD_CASES = int(os.environ.get("SGN_RUNCTL_SHARD_CASES", "12"))


def make_ctx(args, trace=False, hosts=None, cap=1 << 22):
    g, used, hst, cfg, tr = args
    c = sgn.Context()
    c.routes_build(g, used)
    c.hosts_set(hst)
    if trace:
        c.trace_enable(cap)
        if hosts is not None:
            c.trace_hosts(hosts)
    c.sim_init(cfg, tr)
    return c


def refused(call):
    with pytest.raises(sgn.SgnError, match="trace") as e:
        call()
    assert e.value.rc == ESTATE, str(e.value)


def drive_single(args, ref, steps, tmp_path, trace, hosts, tag):
    """One context through the resolved program; returns it and the takes."""
    n = ref["n"]
    c = make_ctx(args, trace, hosts)
    slots, takes = {}, []
    for k, st in enumerate(steps):
        op, what = st["op"], (tag, k, st["op"])
        before = state(c, n) if op[0] in ("save", "export_import") or st["refused"] else None
        if op[0] == "run":
            assert (c.run() if op[1] is None else c.run(op[1])) == st["ret"], what
        elif op[0] == "run_until":
            assert c.run_until(st["t"]) == st["ret"], what
        elif op[0] == "save":
            if op[1] in slots:
                c.snapshot_free(slots[op[1]])
            slots[op[1]] = c.snapshot_save()
            assert c.snapshot_info(slots[op[1]])["rounds"] == st["round"], what
        elif op[0] == "restore":
            if st["refused"]:
                refused(lambda: c.snapshot_restore(slots[op[1]]))
            else:
                c.snapshot_restore(slots[op[1]])
        elif op[0] == "export_import":
            path = tmp_path / f"{tag}-{k}.snap"
            if st["refused"]:
                refused(lambda: c.snapshot_export(slots[op[1]], path))
                assert not path.exists()
            else:
                c.snapshot_export(slots[op[1]], path)
                new = c.snapshot_import(path)
                c.snapshot_free(slots[op[1]])
                slots[op[1]] = new
        elif op[0] == "fresh":
            path = tmp_path / f"{tag}-{k}.snap"
            c.snapshot_export(slots[op[1]], path)
            c.close()
            c = make_ctx(args)
            slots = {op[1]: c.snapshot_import(path)}
            c.snapshot_restore(slots[op[1]])
        elif op[0] == "take":
            recs, spans = c.trace_take()
            if len(st["take"]) == 0:  # (check_take is written for takes with records)
                assert len(recs) == 0 and len(spans) == 0, what
            else:
                check_take(recs, spans, hosts)
            same_records(recs, st["take"], what)
            takes.append(recs)
        elif op[0] == "take_small":
            pend, nsp = st["needed"]
            if pend == 0:
                recs, spans = c.trace_take()
                assert len(recs) == 0 and len(spans) == 0, what
            else:
                small = dict(cap=pend - 1, span_cap=nsp) if st["small"] == "records" else dict(cap=pend, span_cap=nsp - 1)
                with pytest.raises(sgn.SgnError) as e:
                    c.trace_take(**small)
                assert e.value.rc == sgn.ERANGE and e.value.needed == (pend, nsp), (what, e.value.needed)
        got = state(c, n)
        assert got[1]["rounds"] == st["round"], (what, got[1]["rounds"], st["round"])
        assert_state(got, ref["states"][st["round"]], what)
        if before is not None:
            assert_state(got, before, (what, "nothing moved"))
        if trace:
            assert c.trace_pending() == st["pending"], (what, c.trace_pending(), st["pending"])
    for s in slots.values():
        c.snapshot_free(s)
    return c, takes


@pytest.mark.parametrize("case", range(CASES))
def test_program_single(oracle, monkeypatch, tmp_path, case):
    d = draw_case(case)
    for k, v in d["env"].items():
        monkeypatch.setenv(k, v)
    args = scenario(**d["kw"])
    args[3].event_capacity = 1 << 23  # (as the fuzz: bootstrapping bursts fill the calendar's slabs faster)
    trace, hosts = d["trace"], d["hosts"]
    ref = oracle_rounds(oracle, args, trace)
    ledger = TraceLedger(ref["trace"], ref["lens"], hosts) if trace else None
    steps = resolve(d["program"], ref["windows"], ref["stop"], ledger)
    print(case, d["env"], "trace", trace, hosts, "rounds", len(ref["windows"]) - 1,
          [(s["op"], s["round"]) for s in steps])
    c, takes = drive_single(args, ref, steps, tmp_path, trace, hosts, f"case{case}")
    o, n = ref["o"], ref["n"]
    assert c.stats()["rounds"] == len(ref["windows"]) - 1 > 0
    info = c.engine_info()
    assert info["codel_pages_free"] + info["codel_pages_chained"] == info["codel_pages"], (case, info)
    assert_same_run(o, c, n, trace=False)
    if trace:
        # the takes of the final timeline: a record taken again after a rewind replaces the earlier one
        allr = np.concatenate(takes)
        allr = allr[np.lexsort((np.arange(len(allr)), allr["seq"], allr["host"]))]
        last = np.ones(len(allr), bool)
        last[:-1] = (allr["host"][1:] != allr["host"][:-1]) | (allr["seq"][1:] != allr["seq"][:-1])
        got = allr[last]
        want = srt(ref["trace"])
        same_records(got, want if hosts is None else only(want, hosts), (case, "the takes, reassembled"))
        assert c.trace_pending() == 0
    c.close()


def _shard_files(shards, snaps, tmp_path, tag):
    paths = [tmp_path / f"{tag}-shard{r}.snap" for r in range(len(shards))]
    for c, s, p in zip(shards, snaps, paths):
        c.snapshot_export(s, p)
    return paths


@pytest.mark.parametrize("case", range(SHARD_CASES))
def test_program_sharded(oracle, monkeypatch, tmp_path, case):
    d = draw_case(case, trace=False)
    r = np.random.default_rng(6000 + case)
    k = int(r.choice([2, 3]))
    persist = None if r.random() < 0.5 else "0"
    for key, v in d["env"].items():
        if key != "SGN_PERSISTENT":
            monkeypatch.setenv(key, v)
    monkeypatch.delenv("SGN_PERSISTENT", raising=False)
    set_persist(monkeypatch, persist)
    args = scenario(**d["kw"])
    args[3].event_capacity = 1 << 23
    ref = oracle_rounds(oracle, args, False)
    steps = resolve(d["program"], ref["windows"], ref["stop"])
    n = ref["n"]
    print(case, "k", k, "persist", persist, d["env"], "rounds", len(ref["windows"]) - 1,
          [(s["op"], s["round"]) for s in steps])
    shards, arr = group(args, k)
    slots, ran, modes = {}, 0, 0

    def free(snaps):
        for c, s in zip(shards, snaps):
            c.snapshot_free(s)

    for i, st in enumerate(steps):
        op, what = st["op"], (case, i, st["op"])
        before = merged(shards, n) if op[0] in ("save", "export_import") else None
        if op[0] == "run":
            got = run_group(shards, arr) if op[1] is None else run_group(shards, arr, op[1])
            assert got == st["ret"], what
            ran += got
        elif op[0] == "run_until":
            got = sgn.shards_run_until(shards, st["t"])
            assert got == st["ret"], what
            ran += got
        elif op[0] == "save":
            if op[1] in slots:
                free(slots[op[1]])
            slots[op[1]] = sgn.shards_snapshot_save(shards)
        elif op[0] == "restore":
            sgn.shards_snapshot_restore(shards, slots[op[1]])
        elif op[0] == "export_import":
            paths = _shard_files(shards, slots[op[1]], tmp_path, f"s{case}-{i}")
            new = [c.snapshot_import(p) for c, p in zip(shards, paths)]
            free(slots[op[1]])
            slots[op[1]] = new
        elif op[0] == "fresh":
            paths = _shard_files(shards, slots[op[1]], tmp_path, f"s{case}-{i}")
            if ran:
                check_mode(shards, persist)
                modes += 1
            for c in shards:
                c.close()
            shards, arr = group(args, k)
            ran = 0
            slots = {op[1]: [c.snapshot_import(p) for c, p in zip(shards, paths)]}
            sgn.shards_snapshot_restore(shards, slots[op[1]])
        got = merged(shards, n)
        assert got[1]["rounds"] == st["round"], (what, got[1]["rounds"], st["round"])
        assert_merged(got, ref["states"][st["round"]], what)
        if before is not None:
            assert_merged(got, before, (what, "nothing moved"))
    if ran:
        check_mode(shards, persist)  # which round edge ran: k_rounds_x's, or the per-round launches with k_import
        modes += 1
    assert modes > 0
    assert not shards[0].window()[2]
    assert_merged(merged(shards, n), state(ref["o"], n), (case, "end"))
    for snaps in slots.values():
        free(snaps)
    for c in shards:
        c.close()


_TRAIN = {}


def train_ref(oracle, name):
    if name not in _TRAIN:
        args = world(**TRAIN_CASES[name])
        ref = oracle_rounds(oracle, args, True)
        _TRAIN[name] = (args, ref, cached_round(name, srt(ref["trace"]), ref["windows"]))
    return _TRAIN[name]


@pytest.mark.parametrize("trace", [False, True], ids=["untraced", "traced"])
@pytest.mark.parametrize("name", ["plain_100M", "cached_last_then_other_train"])
def test_program_train_merge(oracle, tmp_path, name, trace):
    """A save at a round edge where the server holds a cached packet (Relay::next_packet: refused by
    the token bucket, sent with the next refill), through a file and back."""
    args, ref, r = train_ref(oracle, name)
    n, R = ref["n"], len(ref["windows"]) - 1
    program = [("run", r), ("save", "a"), ("run", 5), ("export_import", "a"), ("restore", "a"), ("run", None)]
    if trace:
        program.append(("take",))
    ledger = TraceLedger(ref["trace"], ref["lens"]) if trace else None
    steps = resolve(program, ref["windows"], ref["stop"], ledger)
    assert [s["round"] for s in steps[:6]] == [r, r, r + 5, r + 5, r, R] and not any(s["refused"] for s in steps)
    c, takes = drive_single(args, ref, steps, tmp_path, trace, None, name)
    assert_same_run(ref["o"], c, n, trace=False)
    if trace:
        assert len(takes) == 1
        same_records(takes[0], srt(ref["trace"]), (name, "one final take"))
        assert np.count_nonzero(takes[0]["kind"] == sgn.TRACE_IF_POP) == np.count_nonzero(takes[0]["kind"] == sgn.TRACE_SEND)
    c.close()
