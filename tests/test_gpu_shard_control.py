"""Run-control for sharded simulations (-m gpu): sgn_shards_run_until, sgn_shards_snapshot_save and
sgn_shards_snapshot_restore on local shard groups, through both multi-shard round edges — the
persistent launches (k_rounds_x, exchange mode 2) and the per-round launches with k_import
(SGN_LOCAL_PERSIST=0, exchange mode 1).

Every comparison is bit for bit against the oracle's ONE uninterrupted (or once-stepped) run of
the scenario, or — for the inbox-growth scenario, as in test_gpu_xpersist — against one unsharded
run. A sharded state is the shards' common window and round count, the additive counters summed
and every host's digests, concatenated in shard order.
"""
import ctypes as C

import numpy as np
import pytest

import sgn
from test_gpu_parity import scenario
from test_gpu_pools import _codel_args, _pages_ok
from test_gpu_snapshot import S0, _until_args, assert_state, ref_run, state, until_ref  # noqa: F401
from test_gpu_xpersist import ADD, DIGESTS, compare, local_group, unsharded

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -22, -71
_MARKS = {}


def group(args, k, **kw):
    """k shards of the scenario as one local group, initialised, no round run."""
    shards, arr, done = local_group(args, k, rounds=0, **kw)
    assert done == 0
    return shards, arr


def run_group(shards, arr, rounds=1 << 40):
    done = C.c_uint64()
    shards[0].check(shards[0].L.sgn_run_local_group(arr, len(shards), rounds, C.byref(done)))
    return done.value


def merged(shards, n):
    wins = [c.window() for c in shards]
    assert all(w == wins[0] for w in wins), wins
    sts = [c.stats() for c in shards]
    assert all(s["rounds"] == sts[0]["rounds"] for s in sts), [s["rounds"] for s in sts]
    st = {"rounds": sts[0]["rounds"]}
    for key in ADD:
        st[key] = sum(s[key] for s in sts)
    digs = []
    for r, c in enumerate(shards):
        lo, hi = C.c_uint32(), C.c_uint32()
        c.L.sgn_shard_range(n, r, len(shards), C.byref(lo), C.byref(hi))
        digs.append(c.digests(lo.value, hi.value))
    return wins[0], st, {f: np.concatenate([d[f] for d in digs]) for f in DIGESTS}


def assert_merged(got, ref, what):
    """got: merged(); ref: merged(), or state() of the oracle (its counters cut to the merged ones)."""
    assert_state(got, (ref[0], {k: ref[1][k] for k in got[1]}, ref[2]), what)


def marks_400(oracle):
    """until_ref's three marks for the 400-host TGEN scenario of test_xpersist_shards_match_single
    (the oracle stepped once, a round at a time)."""
    if "tgen400" in _MARKS:
        return _MARKS["tgen400"]
    n, stop = 400, 600_000_000
    bw = np.where(np.arange(n) % 10 == 0, 100_000_000, 4_000_000).astype(np.uint64)
    args = scenario(n=n, V=30, kind=sgn.TRAFFIC_TGEN, stop_ns=stop, bw=bw, tor=True, tgen_think=100_000_000)
    g, used, hosts, cfg, tr = args
    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr)
    t_mid, t_past = S0 + stop // 2 + 12_345, S0 + stop + 1_000_000_000
    marks, rounds = [], 0
    while o.window()[2]:
        o.round()
        rounds += 1
        ws = o.window()[0]
        if rounds == 30:
            assert ws < t_mid
            marks.append((ws, rounds, state(o, n)))
        if len(marks) == 1 and ws >= t_mid and o.window()[2]:
            assert ws != t_mid
            marks.append((t_mid, rounds, state(o, n)))
    assert len(marks) == 2 and rounds > marks[1][1] > 30
    marks.append((t_past, rounds, state(o, n)))
    _MARKS["tgen400"] = (args, o, marks)
    return _MARKS["tgen400"]


def set_persist(monkeypatch, persist):
    if persist is None:
        monkeypatch.delenv("SGN_LOCAL_PERSIST", raising=False)
    else:
        monkeypatch.setenv("SGN_LOCAL_PERSIST", persist)


def check_mode(shards, persist):
    info = shards[0].engine_info()
    if persist is None and info["calendar_buckets"] <= 256:
        assert info["exchange_mode"] == 2 and info["persistent_x_launches"] > 0, info  # k_rounds_x's compare ran
    elif persist == "0":
        assert info["exchange_mode"] == 1 and info["persistent_x_launches"] == 0, info  # k_import's
    return info


# ---- 1. run-until ----
def _run_until_case(monkeypatch, ref, k, kind, persist):
    set_persist(monkeypatch, persist)
    args, o, marks = ref
    n = args[2].n
    shards, arr = group(args, k)
    assert sgn.shards_run_until(shards, S0) == 0 and sgn.shards_run_until(shards, 0) == 0
    assert all(c.stats()["rounds"] == 0 for c in shards)
    done = 0
    for t, rounds, at in marks[:2]:
        done += sgn.shards_run_until(shards, t)
        assert done == rounds, (kind, t - S0, done, rounds)
        got = merged(shards, n)
        assert got[0][0] >= t and got[0][2], got[0]
        assert_merged(got, at, (kind, t - S0))
        # a target at or below the current window start runs nothing and changes nothing
        for t2 in (t, S0, got[0][0]):
            assert sgn.shards_run_until(shards, t2) == 0
        assert_merged(merged(shards, n), at, (kind, "no-op"))
    info = check_mode(shards, persist)
    assert all(c.engine_info()["rounds_held"] == 0 for c in shards) or kind == "tgen", info  # a pause is no held round
    run_group(shards, arr)  # a plain run after a pause finishes bit-exact
    assert_merged(merged(shards, n), state(o, n), (kind, "end"))
    # a target past the stop time: to the end, in one call
    t, rounds, at = marks[2]
    shards, arr = group(args, k)
    assert sgn.shards_run_until(shards, t) == rounds
    assert_merged(merged(shards, n), at, (kind, "past the end"))
    assert sgn.shards_run_until(shards, t) == 0
    check_mode(shards, persist)


@pytest.mark.parametrize("persist", [None, "0"])
@pytest.mark.parametrize("kind", ["periodic", "tgen", "dynamic"])
@pytest.mark.parametrize("k", [2, 3])
def test_run_until(oracle, monkeypatch, k, kind, persist):
    _run_until_case(monkeypatch, until_ref(oracle, kind), k, kind, persist)


def test_run_until_eight_shards(oracle, monkeypatch):
    _run_until_case(monkeypatch, marks_400(oracle), 8, "tgen", None)


# ---- 2. rewind ----
@pytest.mark.parametrize("persist", [None, "0"])
def test_rewind(oracle, monkeypatch, persist):
    set_persist(monkeypatch, persist)
    args = scenario()
    n, k = args[2].n, 3
    o = ref_run(oracle, "periodic", args, trace=True)  # (test_gpu_snapshot's reference, as it makes it)
    shards, arr = group(args, k)
    assert run_group(shards, arr, 150) == 150
    at = merged(shards, n)
    snaps = sgn.shards_snapshot_save(shards)
    for c, s in zip(shards, snaps):
        info = c.snapshot_info(s)
        assert info["rounds"] == 150 and (info["window_start"], info["window_end"]) == at[0][:2], info
    assert_merged(merged(shards, n), at, "after save")
    run_group(shards, arr)
    end = merged(shards, n)
    assert_merged(end, state(o, n), "first pass")  # the save did not disturb the run
    sgn.shards_snapshot_restore(shards, snaps)
    assert_merged(merged(shards, n), at, "after restore")
    run_group(shards, arr)
    assert_merged(merged(shards, n), end, "second pass")
    assert_merged(merged(shards, n), state(o, n), "second pass, oracle")
    check_mode(shards, persist)
    for c, s in zip(shards, snaps):
        c.snapshot_free(s)


# ---- 3. rewind across an inbox overflow and growth ----
def test_rewind_inbox_growth(monkeypatch):
    monkeypatch.delenv("SGN_LOCAL_PERSIST", raising=False)
    monkeypatch.setenv("SGN_XBIN", "0")
    n, k = 500, 4
    bw = np.where(np.arange(n) % 10 == 0, 100_000_000, 4_000_000).astype(np.uint64)
    args = scenario(n=n, V=30, kind=sgn.TRAFFIC_TGEN, stop_ns=400_000_000, bw=bw, tor=True, tgen_think=50_000_000)
    one = unsharded(args)
    monkeypatch.setenv("SGN_XISLOT", "6")
    shards, arr = group(args, k)
    snaps, at, saved_at = None, None, -1
    for r in range(400):
        if shards[0].engine_info()["inbox_grows"] >= 1:
            break
        if snaps is not None:
            for c, s in zip(shards, snaps):
                c.snapshot_free(s)
        snaps, at, saved_at = sgn.shards_snapshot_save(shards), merged(shards, n), r
        assert run_group(shards, arr, 1) == 1
    print("saved at round", saved_at)
    i1 = [c.engine_info() for c in shards]
    assert snaps is not None and i1[0]["inbox_grows"] >= 1 and i1[0]["inbox_slot_runs"] > 6, i1[0]
    assert all(c.snapshot_info(s)["rounds"] == saved_at for c, s in zip(shards, snaps))
    run_group(shards, arr)
    assert all(c.engine_info()["exchange_mode"] == 2 for c in shards)
    compare(one, shards, n)
    before = [c.engine_info() for c in shards]
    sgn.shards_snapshot_restore(shards, snaps)
    after = [c.engine_info() for c in shards]
    for b, a in zip(before, after):  # the no-shrink rule: the exchange layer is not rewound
        assert a["inbox_slot_runs"] >= b["inbox_slot_runs"] and a["inbox_grows"] == b["inbox_grows"], (b, a)
    assert_merged(merged(shards, n), at, "after restore")
    run_group(shards, arr)
    compare(one, shards, n)


# ---- 4. rewind across a CoDel pool growth on the shards ----
def test_rewind_codel_pool_grows_after_save(oracle, monkeypatch):
    monkeypatch.delenv("SGN_LOCAL_PERSIST", raising=False)
    args = _codel_args(n=300)
    n, k = args[2].n, 2
    o = ref_run(oracle, "codel", args)
    shards, arr = group(args, k)
    keys = ("codel_pages", "codel_pool_grows")
    snaps, at, i0, saved_at = None, None, None, -1
    for r in range(40):  # the last round edge before the first growth on any shard
        info = [c.engine_info() for c in shards]
        if any(i["codel_pool_grows"] >= 1 for i in info):
            break
        if snaps is not None:
            for c, s in zip(shards, snaps):
                c.snapshot_free(s)
        snaps, at, i0, saved_at = sgn.shards_snapshot_save(shards), merged(shards, n), info, r
        assert run_group(shards, arr, 1) == 1
    print("saved at round", saved_at)
    assert snaps is not None and any(c.engine_info()["codel_pool_grows"] >= 1 for c in shards)
    assert all(i["codel_pool_grows"] == 0 for i in i0), i0
    run_group(shards, arr)
    i1 = [c.engine_info() for c in shards]
    assert_merged(merged(shards, n), state(o, n), "first pass")
    sgn.shards_snapshot_restore(shards, snaps)
    i2 = [c.engine_info() for c in shards]
    for a, b in zip(i2, i0):
        for key in keys:
            assert a[key] == b[key], (key, a[key], b[key])
        _pages_ok(a)
    assert_merged(merged(shards, n), at, "after restore")
    run_group(shards, arr)
    i3 = [c.engine_info() for c in shards]
    for a, b in zip(i3, i1):
        for key in keys:
            assert a[key] == b[key], (key, a[key], b[key])
        _pages_ok(a)
    assert_merged(merged(shards, n), state(o, n), "second pass")


# ---- 5. pause, save, restore, run-until again: what a console does ----
@pytest.mark.parametrize("persist", [None, "0"])
def test_console_sequence(oracle, monkeypatch, persist):
    set_persist(monkeypatch, persist)
    args, o, marks = until_ref(oracle, "periodic")
    n, k = args[2].n, 2
    (t0, r0, at0), (t1, r1, at1) = marks[:2]
    shards, arr = group(args, k)
    assert sgn.shards_run_until(shards, t0) == r0
    s0 = sgn.shards_snapshot_save(shards)
    assert sgn.shards_run_until(shards, t1) == r1 - r0
    s1 = sgn.shards_snapshot_save(shards)
    assert_merged(merged(shards, n), at1, "second mark")
    run_group(shards, arr)
    assert_merged(merged(shards, n), state(o, n), "end")
    sgn.shards_snapshot_restore(shards, s1)  # in reverse order
    assert_merged(merged(shards, n), at1, "restored second mark")
    assert sgn.shards_run_until(shards, marks[2][0]) == marks[2][1] - r1
    assert_merged(merged(shards, n), marks[2][2], "second mark to the end")
    sgn.shards_snapshot_restore(shards, s0)
    assert_merged(merged(shards, n), at0, "restored first mark")
    assert sgn.shards_run_until(shards, t1) == r1 - r0
    assert_merged(merged(shards, n), at1, "first mark to the second")
    run_group(shards, arr)
    assert_merged(merged(shards, n), state(o, n), "end again")
    check_mode(shards, persist)


# ---- 6. errors, none of which changes the state ----
def test_errors(monkeypatch):
    monkeypatch.delenv("SGN_LOCAL_PERSIST", raising=False)
    args = scenario(n=60, V=10, stop_ns=40_000_000)
    g, used, hosts, cfg, tr = args
    n, k = hosts.n, 3
    shards, arr = group(args, k)
    L = shards[0].L
    assert run_group(shards, arr, 5) == 5
    s5 = sgn.shards_snapshot_save(shards)
    assert run_group(shards, arr, 5) == 5
    s10 = sgn.shards_snapshot_save(shards)
    at = merged(shards, n)
    t = at[0][0] + 5_000_000
    done = C.c_uint64(9)
    out = (C.c_void_p * k)()

    def snaparr(snaps):
        return (C.c_void_p * len(snaps))(*[s.value for s in snaps])

    # a null pointer
    holes = (C.c_void_p * k)(shards[0].h.value, None, shards[2].h.value)
    assert L.sgn_shards_run_until(None, k, t, C.byref(done)) == EINVAL and done.value == 0
    assert L.sgn_shards_run_until(holes, k, t, None) == EINVAL
    assert L.sgn_shards_snapshot_save(holes, k, out) == EINVAL and not any(out)
    assert L.sgn_shards_snapshot_save(arr, k, None) == EINVAL
    assert L.sgn_shards_snapshot_restore(arr, k, None) == EINVAL
    assert L.sgn_shards_snapshot_restore(arr, k, snaparr([s10[0], C.c_void_p(), s10[2]])) == EINVAL
    # a partial group
    for call in (lambda: sgn.shards_run_until(shards[:2], t), lambda: sgn.shards_snapshot_save(shards[:2]),
                 lambda: sgn.shards_snapshot_restore(shards[:2], s10[:2]),
                 lambda: sgn.shards_run_until(shards[::-1], t)):
        with pytest.raises(sgn.SgnError, match="every context of the local shard group") as e:
            call()
        assert e.value.rc == ESTATE
    # an unsharded context
    one = sgn.Context(flags=2)
    one.routes_build(g, used)
    one.hosts_set(hosts)
    one.sim_init(cfg, tr)
    for call in (lambda: sgn.shards_run_until([one], t), lambda: sgn.shards_snapshot_save([one])):
        with pytest.raises(sgn.SgnError, match="not a sharded context") as e:
            call()
        assert e.value.rc == ESTATE
    assert one.stats()["rounds"] == 0
    # snapshots of two different rounds in one restore; a shard's snapshot in another's place
    with pytest.raises(sgn.SgnError, match="different round edges") as e:
        sgn.shards_snapshot_restore(shards, [s10[0], s5[1], s10[2]])
    assert e.value.rc == EINVAL
    with pytest.raises(sgn.SgnError, match="not a snapshot of this context") as e:
        sgn.shards_snapshot_restore(shards, [s10[1], s10[0], s10[2]])
    assert e.value.rc == EINVAL
    assert_merged(merged(shards, n), at, "after the refused calls")
    # the plain calls keep refusing a shard
    with pytest.raises(sgn.SgnError, match="sharded context") as e:
        shards[1].snapshot_restore(s10[1])
    assert e.value.rc == ESTATE
    # ... and the state is intact: both snapshots still restore and run to the same end
    run_group(shards, arr)
    end = merged(shards, n)
    sgn.shards_snapshot_restore(shards, s5)
    assert all(c.stats()["rounds"] == 5 for c in shards)
    run_group(shards, arr)
    assert_merged(merged(shards, n), end, "from round 5")
    # a snapshot from before the last sgn_sim_init
    for c in shards:
        c.sim_init(cfg, tr)
    with pytest.raises(sgn.SgnError, match="before the last sgn_sim_init") as e:
        sgn.shards_snapshot_restore(shards, s10)
    assert e.value.rc == ESTATE
    assert all(c.stats()["rounds"] == 0 for c in shards)
