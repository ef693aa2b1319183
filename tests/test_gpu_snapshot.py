"""Snapshot / restore of a running simulation and run-until-time (-m gpu).

The engine is bit-deterministic, so "restore, then run" must reproduce the run that followed the
save. Every case compares the restored run with the oracle's ONE uninterrupted run of the same
scenario — which also proves that a save in the middle does not disturb the run. The oracle runs
once per scenario (module cache) and is never stepped again afterwards.
"""
import ctypes as C

import numpy as np
import pytest

import sgn
from test_gpu_parity import assert_same_run, ctxf, scenario  # noqa: F401 (ctxf: fixture)
from test_gpu_pools import _codel_args, _hot_args, _pages_ok

pytestmark = pytest.mark.gpu

S0 = sgn.SIMULATION_START
EINVAL, ESTATE = -22, -71
DIG = ("tx", "rx", "app", "rng", "next_event_id", "n_sent", "n_popped", "n_delivered", "n_codel_dropped")
# (diagnostic counters the oracle does not define the same way: assert_same_run skips them too)
SKIP = ("max_pending_events", "sched_heavy_hosts", "sched_sorted_segments", "event_runs")

_REF = {}


def ref_run(oracle, key, args, trace=False):
    """The oracle's uninterrupted run of a scenario, once per module."""
    if key not in _REF:
        g, used, hosts, cfg, tr = args
        lat, loss = oracle.routes(g, used)
        o = oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=trace)
        o.run()
        _REF[key] = o
    return _REF[key]


def make_ctx(ctxf, args, trace=False):
    g, used, hosts, cfg, tr = args
    c = ctxf()
    c.routes_build(g, used)
    c.hosts_set(hosts)
    if trace:
        c.trace_enable(1 << 22)
    c.sim_init(cfg, tr)
    return c


def state(s, n):
    st = s.stats()
    return s.window(), {k: v for k, v in st.items() if k not in SKIP}, s.digests(0, n)


def assert_state(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    assert a[1] == b[1], (what, a[1], b[1])
    for f in DIG:
        assert np.array_equal(a[2][f], b[2][f]), (what, f)


# ---- 1. rewind, PERIODIC ----
@pytest.mark.parametrize("persistent,trace", [("1", False), ("0", False), ("1", True), ("0", True)])
def test_rewind_periodic(ctxf, oracle, monkeypatch, persistent, trace):
    monkeypatch.setenv("SGN_PERSISTENT", persistent)
    args = scenario()
    n = args[2].n
    o = ref_run(oracle, "periodic", args, trace=True)
    c = make_ctx(ctxf, args, trace=trace)
    assert c.run(150) == 150
    at = state(c, n)
    snap = c.snapshot_save()
    info = c.snapshot_info(snap)
    assert info["rounds"] == 150 and (info["window_start"], info["window_end"]) == at[0][:2], info
    assert info["calendar_runs"] > 0 and info["calendar_bytes"] == 32 * info["calendar_runs"], info
    assert_state(state(c, n), at, "after save")
    c.run()
    end = state(c, n)
    assert_same_run(o, c, n, trace=trace)  # the save did not disturb the run
    c.snapshot_restore(snap)
    assert_state(state(c, n), at, "after restore")
    c.run()
    assert_state(state(c, n), end, "second pass")
    assert_same_run(o, c, n, trace=trace)  # (traced: the whole trace, rewritten from the save on)
    assert (c.engine_info()["persistent_grid"] > 0) == (persistent == "1" and not trace)
    c.snapshot_free(snap)


# ---- 2. rewind, TGEN with standing CoDel queues; the pool grows after the save ----
@pytest.mark.parametrize("persistent", ["1", "0"])
def test_rewind_codel_pool_grows_after_save(ctxf, oracle, monkeypatch, persistent):
    monkeypatch.setenv("SGN_PERSISTENT", persistent)
    args = _codel_args(n=300)
    n = args[2].n
    o = ref_run(oracle, "codel", args)
    c = make_ctx(ctxf, args)
    # The pool starts at one page per host plus 64, so it grows within the first rounds that carry
    # traffic (before round 20 on an MI355X). The save is therefore the last round edge BEFORE the
    # first growth: a snapshot per round edge, the previous one freed, until a round grew the pool
    # (round 5 on an MI355X, with and without persistent rounds).
    snap, at, i0, saved_at = None, None, None, -1
    for r in range(40):
        info = c.engine_info()
        if info["codel_pool_grows"] >= 1:
            break
        if snap is not None:
            c.snapshot_free(snap)
        snap, at, i0, saved_at = c.snapshot_save(), state(c, n), info, r
        assert c.run(1) == 1
    print("saved at round", saved_at)
    assert snap is not None and c.engine_info()["codel_pool_grows"] >= 1
    assert i0["codel_pool_grows"] == 0, i0  # the premise: the save precedes the first growth
    assert c.snapshot_info(snap)["rounds"] == saved_at
    c.run()
    i1 = c.engine_info()
    assert i1["codel_pool_grows"] >= 1 and i1["codel_pages"] > i0["codel_pages"], i1
    assert_same_run(o, c, n, trace=False)
    c.snapshot_restore(snap)
    i2 = c.engine_info()
    for k in ("codel_pages", "codel_pool_grows", "codel_page_allocs", "rounds_held"):
        assert i2[k] == i0[k], (k, i2[k], i0[k])
    _pages_ok(i2)
    assert_state(state(c, n), at, "after restore")
    c.run()
    i3 = c.engine_info()
    for k in ("codel_pages", "codel_pool_grows"):
        assert i3[k] == i1[k], (k, i3[k], i1[k])
    _pages_ok(i3)
    assert (i3["persistent_grid"] > 0) == (persistent == "1"), i3
    assert_same_run(o, c, n, trace=False)


# ---- 3. the calendar is re-laid out after the save; the save is of an empty calendar ----
def test_rewind_calendar_relayout_after_save(ctxf, oracle, monkeypatch):
    monkeypatch.setenv("SGN_SLAB_CAP", "16")
    n = 2000
    args = scenario(n=n, V=100, period_ns=500_000, stop_ns=150_000_000, bw=100_000_000)
    o = ref_run(oracle, "relayout", args)
    c = make_ctx(ctxf, args)
    at = state(c, n)
    snap = c.snapshot_save()  # right after sgn_sim_init: nothing in the calendar yet
    info = c.snapshot_info(snap)
    assert info["rounds"] == 0 and info["calendar_runs"] == 0 and info["calendar_bytes"] == 0, info
    assert info["calendar_pool_bytes"] > 0 and info["device_bytes"] > 0, info
    assert c.engine_info()["slab_capacity"] == 16
    c.run()
    i1 = c.engine_info()
    assert i1["calendar_grows"] >= 1 and i1["slab_capacity"] > 16, i1
    assert_same_run(o, c, n, trace=False)
    c.snapshot_restore(snap)
    i2 = c.engine_info()
    assert i2["slab_capacity"] == 16 and i2["calendar_grows"] == 0 and i2["calendar_spill_runs"] == 0, i2
    assert_state(state(c, n), at, "after restore")
    c.run()
    i3 = c.engine_info()
    for k in ("slab_capacity", "calendar_grows", "calendar_spill_runs", "slab_extensions"):
        assert i3[k] == i1[k], (k, i3[k], i1[k])
    assert_same_run(o, c, n, trace=False)


# ---- 4. slab extensions inside the snapshot ----
def test_rewind_with_slab_extensions(ctxf, oracle, monkeypatch):
    monkeypatch.setenv("SGN_SLAB_CAP", "16")
    monkeypatch.setenv("SGN_SLAB_LIM", "32")
    n = 1200
    args = _hot_args(n)
    o = ref_run(oracle, "hot", args)
    c = make_ctx(ctxf, args)
    snap, info = None, None
    for _ in range(200):  # the first round edge with an extension and a calendar that is not empty
        assert c.run(1) == 1
        if c.engine_info()["slab_extensions"] >= 1:
            snap = c.snapshot_save()
            info = c.snapshot_info(snap)
            if info["calendar_runs"] > 0:
                break
            c.snapshot_free(snap)
            snap = None
    assert snap is not None
    i0 = c.engine_info()
    assert i0["slab_extensions"] >= 1 and info["calendar_runs"] > 0, (i0, info)
    assert info["calendar_bytes"] == 32 * info["calendar_runs"], info
    assert info["calendar_bytes"] < info["calendar_pool_bytes"], info
    at = state(c, n)
    c.run()
    i1 = c.engine_info()
    assert_same_run(o, c, n, trace=False)
    c.snapshot_restore(snap)
    i2 = c.engine_info()
    for k in ("slab_extensions", "slab_extension_runs", "slab_capacity", "calendar_grows"):
        assert i2[k] == i0[k], (k, i2[k], i0[k])
    assert_state(state(c, n), at, "after restore")
    c.run()
    i3 = c.engine_info()
    for k in ("slab_extensions", "slab_extension_runs", "slab_capacity", "big_slab_pieces"):
        assert i3[k] == i1[k], (k, i3[k], i1[k])
    assert_same_run(o, c, n, trace=False)


# ---- 5. several snapshots, any order, after the end, after freeing one ----
def test_several_snapshots(ctxf, oracle):
    args = scenario()
    n = args[2].n
    o = ref_run(oracle, "periodic", args, trace=True)
    c = make_ctx(ctxf, args)
    c.run(50)
    w50 = c.window()
    s50 = c.snapshot_save()
    c.run(150)
    w200 = c.window()
    s200 = c.snapshot_save()
    c.run()
    assert c.window()[2] is False  # finished: a restore still works
    assert_same_run(o, c, n, trace=False)
    for snap, w, r in ((s200, w200, 200), (s50, w50, 50), (s50, w50, 50)):
        c.snapshot_restore(snap)
        assert c.window() == w and c.stats()["rounds"] == r
        c.run()
        assert_same_run(o, c, n, trace=False)
    c.snapshot_free(s200)
    c.snapshot_restore(s50)
    assert c.window() == w50 and c.stats()["rounds"] == 50
    with pytest.raises(sgn.SgnError, match="not a snapshot of this context") as e:
        c.snapshot_restore(s200)  # freed
    assert e.value.rc == EINVAL
    c.run()
    assert_same_run(o, c, n, trace=False)


# ---- 6. EXTERNAL traffic and the host RNG ----
def _drive(sims, dg, nxt, rounds, until, rng_hosts=(1, 2)):
    """external_common.drive from datagram nxt and round count `rounds` on, for at most `until`
    rounds in all (None: to the end, with a last drain). Returns per sim the drain records and the
    CPU-side RNG draws, and the position reached."""
    from external_common import RUNAHEAD
    src, dip, pay, t, handle, wire = dg
    drains = [[] for _ in sims]
    draws = [[] for _ in sims]
    while until is None or rounds < until:
        wins = [s.window() for s in sims]
        assert all(w == wins[0] for w in wins), wins
        ws, we, active = wins[0]
        if nxt < len(t) and (not active or int(t[nxt]) < ws):
            ws, we = int(t[nxt]), int(t[nxt]) + RUNAHEAD
            for s in sims:
                s.set_window(ws, we)
            we = sims[0].window()[1]
        elif not active:
            break
        j = nxt
        while j < len(t) and int(t[j]) < we:
            j += 1
        if j > nxt:
            for s in sims:
                s.submit(src[nxt:j], dip[nxt:j], pay[nxt:j], t[nxt:j], handle[nxt:j], wire_len=wire[nxt:j])
            nxt = j
        mins = [s.round() for s in sims]
        assert all(m == mins[0] for m in mins), mins
        rounds += 1
        if rounds % 7 == 0:
            h = rng_hosts[rounds % len(rng_hosts)]
            for i, s in enumerate(sims):
                draws[i].append((s.rng_next_u64(h), s.rng_double(h), s.rng_fill_bytes(h, rounds % 13)))
        if rounds % 5 == 0:
            for i, s in enumerate(sims):
                drains[i].append(s.drain(0, 30, cap=1 << 16))
                drains[i].append(s.drain(30, 1 << 31, cap=1 << 16))
    if until is None:
        for i, s in enumerate(sims):
            drains[i].append(s.drain(cap=1 << 16))
    cat = [np.concatenate(d) if d else np.zeros(0, sgn.DRAIN_DTYPE) for d in drains]
    return cat, draws, nxt, rounds


def test_rewind_external_traffic_and_rng(ctxf, oracle):
    from external_common import datagrams, external_world
    world = external_world()
    g, used, hosts, cfg, tr = world
    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=False)
    c = ctxf()
    c.routes_build(g, used)
    c.hosts_set(hosts)
    c.drain_enable(1 << 16)
    c.sim_init(cfg, tr)
    dg = datagrams(hosts)
    # 43 rounds in lockstep: the last drain was at round 40, so records wait on the device, and a
    # CPU-held RNG state (host 3's) is outstanding at the save
    _, _, nxt, rounds = _drive([o, c], dg, 0, 0, 43)
    assert rounds == 43 and 0 < nxt < len(dg[3])
    assert o.rng_next_u64(3) == c.rng_next_u64(3)
    at = state(c, hosts.n)
    snap = c.snapshot_save()
    (do, dc), (wo, wc), _, total = _drive([o, c], dg, nxt, rounds, None)
    assert total > 50 and len(dc) > 0 and len(wc) > 0 and wo == wc
    for f in sgn.DRAIN_DTYPE.names:
        assert np.array_equal(do[f], dc[f]), f
    more = (o.rng_next_u64(3), o.rng_next_u64(1))
    assert more == (c.rng_next_u64(3), c.rng_next_u64(1))
    assert_same_run(o, c, hosts.n, trace=False)
    # back to the save; the same calls again (the oracle is not driven again)
    c.snapshot_restore(snap)
    assert_state(state(c, hosts.n), at, "after restore")
    (dc2,), (wc2,), _, total2 = _drive([c], dg, nxt, rounds, None)
    assert total2 == total and wc2 == wc
    assert len(dc2) == len(dc)
    for f in sgn.DRAIN_DTYPE.names:
        assert np.array_equal(dc2[f], dc[f]), f
    assert (c.rng_next_u64(3), c.rng_next_u64(1)) == more
    assert_same_run(o, c, hosts.n, trace=False)


# ---- 7. run-until ----
def _until_args(kind):
    if kind == "tgen":
        bw = np.where(np.arange(300) % 10 == 0, 100_000_000, 4_000_000).astype(np.uint64)
        return scenario(n=300, V=30, kind=sgn.TRAFFIC_TGEN, stop_ns=600_000_000, bw=bw, tor=True,
                        tgen_think=100_000_000), 600_000_000
    if kind == "dynamic":
        # edge latencies of 1-10 ms: with 1-ms buckets (the self-loops' latency) the longest path
        # keeps the calendar within the 256 buckets persistent rounds need (scenario()'s 1-50 ms
        # edges give 512 buckets and per-round launches in both legs)
        args = scenario(n=150, dynamic=True, runahead_ns=0, bootstrap_ns=100_000_000, stop_ns=400_000_000)
        g = sgn.random_graph(50, seed=1, lat_lo_us=1000, lat_hi_us=10_000)
        return (g,) + tuple(args[1:]), 400_000_000
    return scenario(stop_ns=200_000_000), 200_000_000


def until_ref(oracle, kind):
    """The oracle stepped a round at a time, once: for three targets t — an exact window start,
    one mid-run that is no window start, one past the stop time — the state at the first round
    edge whose window starts at or after t (or at the end)."""
    key = "until-" + kind
    if key in _REF:
        return _REF[key]
    args, stop = _until_args(kind)
    g, used, hosts, cfg, tr = args
    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr)
    n = hosts.n
    t_mid, t_past = S0 + stop // 2 + 12_345, S0 + stop + 1_000_000_000
    marks = []
    rounds = 0
    while o.window()[2]:
        o.round()
        rounds += 1
        ws = o.window()[0]
        if rounds == 30:
            assert ws < t_mid
            marks.append((ws, rounds, state(o, n)))  # t = this window start, exactly
        if len(marks) == 1 and ws >= t_mid and o.window()[2]:
            assert ws != t_mid
            marks.append((t_mid, rounds, state(o, n)))
    assert len(marks) == 2 and rounds > marks[1][1] > 30, (rounds, [m[:2] for m in marks])
    marks.append((t_past, rounds, state(o, n)))
    _REF[key] = (args, o, marks)
    return _REF[key]


@pytest.mark.parametrize("persistent", ["1", "0"])
@pytest.mark.parametrize("kind", ["periodic", "tgen", "dynamic"])
def test_run_until(ctxf, oracle, monkeypatch, kind, persistent):
    monkeypatch.setenv("SGN_PERSISTENT", persistent)
    args, o, marks = until_ref(oracle, kind)
    n = args[2].n
    c = make_ctx(ctxf, args)
    assert c.run_until(S0) == 0 and c.run_until(0) == 0 and c.stats()["rounds"] == 0
    done = 0
    for t, rounds, ref in marks[:2]:
        done += c.run_until(t)
        assert done == rounds, (kind, t - S0, done, rounds)
        got = state(c, n)
        assert_state(got, ref, (kind, t - S0))
        assert got[0][0] >= t and got[0][2]
        # a target at or below the current window start runs nothing and changes nothing
        assert c.run_until(t) == 0 and c.run_until(got[0][0]) == 0 and c.run_until(S0) == 0
        assert_state(state(c, n), ref, (kind, "no-op"))
    info = c.engine_info()
    assert (info["persistent_grid"] > 0) == (persistent == "1"), info  # the device-side check ran
    assert info["rounds_held"] == 0 or kind == "tgen", info            # (a pause is not a held round)
    c.run()  # a plain run after a pause finishes bit-exact
    assert_same_run(o, c, n, trace=False)
    # a target past the stop time: to the end, in one call
    t, rounds, ref = marks[2]
    c.sim_init(args[3], args[4])
    assert c.run_until(t) == rounds
    assert_state(state(c, n), ref, (kind, "past the end"))
    assert c.run_until(t) == 0
    assert_same_run(o, c, n, trace=False)


# ---- 8. errors ----
def test_errors(ctxf):
    args = scenario(n=40, V=10, stop_ns=20_000_000)
    g, used, hosts, cfg, tr = args
    c = ctxf()
    c.routes_build(g, used)
    c.hosts_set(hosts)
    for call in (c.snapshot_save, lambda: c.run_until(S0 + 1)):  # before sgn_sim_init
        with pytest.raises(sgn.SgnError, match="no simulation") as e:
            call()
        assert e.value.rc == ESTATE
    c.sim_init(cfg, tr)
    c.run(5)
    snap = c.snapshot_save()
    # null arguments
    assert c.L.sgn_snapshot_save(c.h, None) == EINVAL and b"null" in c.L.sgn_last_error(c.h)
    assert c.L.sgn_snapshot_restore(c.h, None) == EINVAL and b"null" in c.L.sgn_last_error(c.h)
    # another context's snapshot
    c2 = make_ctx(ctxf, args)
    with pytest.raises(sgn.SgnError, match="not a snapshot of this context") as e:
        c2.snapshot_restore(snap)
    assert e.value.rc == EINVAL
    c2.snapshot_free(snap)  # (not its own: no effect)
    c.snapshot_restore(snap)
    # a snapshot of the simulation before the last sgn_sim_init
    c.sim_init(cfg, tr)
    with pytest.raises(sgn.SgnError, match="before the last sgn_sim_init") as e:
        c.snapshot_restore(snap)
    assert e.value.rc == ESTATE
    c.snapshot_free(snap)
    # a shard of a local two-shard group
    shards = [ctxf(shard_rank=r, shard_count=2) for r in range(2)]
    arr = (C.c_void_p * 2)(*[s.h.value for s in shards])
    for s in shards:
        s.routes_build(g, used)
        s.hosts_set(hosts)
    shards[0].check(shards[0].L.sgn_comm_init_local(arr, 2, 1 << 12))
    for s in shards:
        s.sim_init(cfg, tr)
    with pytest.raises(sgn.SgnError, match="sharded context") as e:
        shards[1].snapshot_save()
    assert e.value.rc == ESTATE
    with pytest.raises(sgn.SgnError, match="single shard") as e:
        shards[0].run_until(S0 + 1_000_000)
    assert e.value.rc == ESTATE
