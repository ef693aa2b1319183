"""The backlog report (-m gpu): sgn_backlog (backlog.hip) and Context.backlog against the oracle.

The expected values never come from libsgn: tests/backlog_model.py derives every row field from
the oracle's trace at the edge sgn_run_until stops at (tests/test_backlog_model.py shows on the
oracle alone that the scenarios are not trivial there). Rows, totals, maxima, window and round
count are compared exactly; router_bytes under TGEN on the hosts whose queued packets are all
delivered later (the model's bytes_known), elsewhere the device's own sum is checked against its
rows. No test provokes a device fault: every error path here is a host-side refusal.
"""
import ctypes as C

import numpy as np
import pytest

import backlog_model as bm
import sgn
from test_backlog_model import external_run
from test_gpu_parity import assert_same_run, ctxf  # noqa: F401 (ctxf: a fixture)

pytestmark = pytest.mark.gpu

S0, MS = sgn.SIMULATION_START, 1_000_000
ESTATE, ERANGE, EINVAL = -71, -34, -22
ROUTER_HELD, OUT_HELD = sgn.BACKLOG_ROUTER_HELD, sgn.BACKLOG_OUT_HELD


def make(ctxf, args, trace=0, **kw):
    g, used, hosts, cfg, tr = args
    c = ctxf(**kw)
    c.routes_build(g, used)
    c.hosts_set(hosts)
    if trace:
        c.trace_enable(trace)
    c.sim_init(cfg, tr)
    return c


def check(b, x, lo=0, hi=None):
    """One report of the hosts [lo, hi) against the model at that edge."""
    hi = x.n if hi is None else hi
    rows, info = b.rows, b.info
    what = ((x.ws - S0) / MS, lo, hi)
    assert x.send_known, what
    h = rows["host"].astype(np.int64)
    assert np.array_equal(h, np.nonzero(x.has_row()[lo:hi])[0] + lo), what  # ascending, owned, no row for an idle host
    for f in bm.ROW_FIELDS:
        got, want = rows[f].astype(np.uint64), x.r[f][h]
        if f == "router_bytes":
            k = x.bytes_known[h]
            got, want = got[k], want[k]
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (what, f, h[bad[:4]], got[bad[:4]], want[bad[:4]])
    e = x.edge
    assert (info["rounds"], info["window_start"], info["window_end"]) == (e["stats"]["rounds"],) + e["win"][:2], what
    assert info["hosts"] == hi - lo and info["rows"] == len(rows), what
    # the device's fold against its rows, then against the model
    folded = [int(rows["router_packets"].sum()), int(rows["router_bytes"].sum(dtype=np.uint64)),
              int((rows["flags"] & ROUTER_HELD != 0).sum()), int(rows["send_packets"].sum()),
              int(rows["send_bytes"].sum(dtype=np.uint64)), int((rows["flags"] & OUT_HELD != 0).sum()),
              int(rows["inflight_packets"].sum()), int(rows["submit_pending"].sum())]
    assert info["total"] == folded, (what, info["total"], folded)
    want = x.total(lo, hi)
    if not x.bytes_known[lo:hi].all():
        want[1] = folded[1]
    assert info["total"] == want, (what, info["total"], want)
    mq, hq, ms, hs, ie = x.maxima(lo, hi)
    assert (info["max_router_packets"], info["max_router_host"]) == (mq, hq), what
    assert (info["max_sojourn_ns"], info["max_sojourn_host"]) == (ms, hs), what
    assert info["inflight_earliest"] == ie, what


# ---- the oracle, once per scenario (never modified afterwards) ----
@pytest.fixture(scope="module")
def periodic(oracle):
    args = bm.periodic_world()
    o, xs = bm.expect_at(oracle, args, bm.PERIODIC_TARGETS)
    return args, o, xs


# ---- 1. PERIODIC rows against the model ----
def test_periodic_rows(ctxf, periodic):
    args, o, xs = periodic
    c = make(ctxf, args)
    packet_next = 0
    for t, x in zip(bm.PERIODIC_TARGETS, xs):
        c.run_until(t)
        b = c.backlog()
        check(b, x)
        # a host's next event is at or before the first packet in flight towards it, and the next
        # event of all is no later than the report's earliest delivery
        nxt = c.next_event_times(0, 200)
        early = np.full(200, sgn.EMUTIME_INVALID, dtype=np.uint64)
        early[b.rows["host"]] = b.rows["inflight_earliest"]
        assert np.all(nxt <= early) and int(nxt.min()) <= b.info["inflight_earliest"]
        packet_next += int((nxt == early).sum())
        assert np.array_equal(b.dense("router_packets"), x.r["router_packets"])
        assert b.totals["inflight_packets"] == int(x.r["inflight_packets"].sum())
    assert packet_next > 100  # (hosts whose next event IS their earliest packet in flight)
    t = c.backlog_timing()
    assert t["hosts"] == 200 and t["rows"] == b.info["rows"] and t["total_ms"] > 0 and t["calendar_runs"] > 0
    assert t["calendar_runs"] <= b.totals["inflight_packets"]  # (a run holds at least one packet)


# ---- 2. wave and group boundaries ----
@pytest.mark.parametrize("n,hpw", [(63, 0), (64, 0), (65, 64), (65, 8), (65, 1)])
def test_wave_and_group_boundaries(ctxf, oracle, n, hpw):
    args = bm.periodic_world(n=n, hosts_per_wave=hpw)
    targets = [S0 + k * 40 * MS for k in range(1, 4)]
    o, xs = bm.expect_at(oracle, args, targets)
    assert xs[-1].has_row()[n - 1] and xs[-1].r["router_packets"].max() > 16
    c = make(ctxf, args)
    assert c.engine_info()["hosts_per_wave"] == (hpw or 64)
    for t, x in zip(targets, xs):
        c.run_until(t)
        check(c.backlog(), x)


# ---- 3. TGEN rows against the model ----
def test_tgen_rows(ctxf, oracle):
    args = bm.tgen_world()
    o, xs = bm.expect_at(oracle, args, bm.TGEN_TARGETS, full=True)
    c = make(ctxf, args)
    for t, x in zip(bm.TGEN_TARGETS, xs):
        c.run_until(t)
        check(c.backlog(), x)


# ---- 4. stale cold lines ----
def test_stale_cold_lines(ctxf, oracle):
    args = bm.cold_world()
    o, xs = bm.expect_at(oracle, args, bm.COLD_TARGETS)
    c = make(ctxf, args)
    for t, x in zip(bm.COLD_TARGETS, xs):
        c.run_until(t)
        check(c.backlog(), x)  # (an idle host with stale cold lines: no row, or a row without queue fields)


# ---- 5. send-ring wrap, submit_pending (EXTERNAL) ----
def test_send_ring_wrap(ctxf, oracle):
    from external_common import external_world
    c = make(ctxf, external_world(fifo=8))
    got = []
    world, dg, o, edges, drains = external_run(oracle, [c], on_step=lambda k: got.append(c.backlog()))
    m = bm.Model(o.trace(), world[2], world[3], world[4])
    assert len(got) == len(edges) >= 10
    for b, (k, e) in zip(got, edges):
        check(b, m.at(e, bm.External(dg, bm.submitted_by(dg, k), drains)))
    assert got[-1].info["rows"] == 0


# ---- 6. slab extensions ----
def test_extensions(ctxf, oracle, monkeypatch):
    from test_gpu_pools import _hot_args
    monkeypatch.setenv("SGN_SLAB_CAP", "16")
    monkeypatch.setenv("SGN_SLAB_LIM", "32")
    args = _hot_args(1200)
    o = bm.oracle_sim(oracle, args)
    edges = []
    for _ in range(4):
        o.round()
        edges.append(bm.edge_of(o))
    m = bm.Model(o.trace(), args[2], args[3], args[4])
    c = make(ctxf, args)
    ext = 0
    for e in edges:
        c.run_until(e["win"][0])
        assert c.window() == e["win"]
        b = c.backlog()
        ext = max(ext, c.engine_info()["slab_extensions"])
        x = m.at(e)
        assert np.array_equal(b.dense("inflight_packets"), x.r["inflight_packets"])
        assert np.array_equal(b.dense("inflight_earliest"), np.where(x.r["inflight_packets"] > 0, x.r["inflight_earliest"], 0))
        assert np.array_equal(b.dense("inflight_latest"), x.r["inflight_latest"])
        assert b.totals["inflight_packets"] == int(x.r["inflight_packets"].sum())
    assert ext > 0


# ---- 7. identities against counters that are already verified (no oracle) ----
def test_identities_5000(ctxf):
    args = bm.periodic_world(n=5000)
    c = make(ctxf, args)
    for t in (S0 + 50 * MS, S0 + 100 * MS):
        c.run_until(t)
        b = c.backlog()
        d, st = c.digests(0, 5000), c.stats()
        held = (b.dense("flags") & ROUTER_HELD != 0).astype(np.uint64)
        assert np.array_equal(b.dense("router_packets") + held, d["n_popped"] - d["n_delivered"] - d["n_codel_dropped"])
        assert int(b.rows["inflight_packets"].sum()) == b.totals["inflight_packets"] == st["packets_sent"] - st["packet_events_popped"]
        assert b.info["max_router_packets"] == int(b.rows["router_packets"].max()) > 16
        assert np.all(np.diff(b.rows["host"].astype(np.int64)) > 0) and b.info["rows"] == len(b.rows)


# ---- 8. the simulation is untouched ----
def test_simulation_untouched(ctxf, oracle):
    args = bm.periodic_world()
    g, used, hosts, cfg, tr = args
    o = bm.oracle_sim(oracle, args)
    c = make(ctxf, args, trace=1 << 22)
    b = c.backlog()
    assert b.info["rows"] == 0 and len(b.rows) == 0 and b.info["total"] == [0] * 8  # a fresh simulation
    assert b.info["inflight_earliest"] == sgn.EMUTIME_INVALID and b.info["hosts"] == 200
    k = 0
    while c.window()[2]:
        k += 1
        c.run_until(S0 + k * 20 * MS)
        c.backlog()
        c.backlog(rows=False)
    o.run()
    assert k >= 14 and not o.window()[2]
    assert_same_run(o, c, 200, trace=True)
    # a finished simulation reports what is truly left
    m = bm.Model(o.trace(), hosts, cfg, tr)
    x = m.at(bm.edge_of(o))
    assert x.has_row().sum() > 50
    check(c.backlog(), x)


# ---- 9. capacity rules ----
def test_capacity_rules(ctxf, periodic):
    args, o, xs = periodic
    c = make(ctxf, args)
    c.run_until(bm.PERIODIC_TARGETS[2])
    full = c.backlog()
    n_rows = full.info["rows"]
    assert n_rows == int(xs[2].has_row().sum()) > 2
    tot = c.backlog(rows=False)
    assert tot.info == full.info and len(tot.rows) == 0
    with pytest.raises(sgn.SgnError) as ei:
        c.backlog(cap=n_rows - 1)
    e = ei.value
    assert e.rc == ERANGE and e.needed == n_rows and e.info == full.info
    assert not e.out.view(np.uint8).any()  # nothing was written to the caller's array
    # the sentinel form through the C ABI: a filled array stays as it is
    out = np.full(n_rows, 0xAB, dtype=np.uint8).repeat(64).view(sgn.BACKLOG_ROW_DTYPE)
    n, info = C.c_uint64(), sgn.BacklogInfo()
    rc = c.L.sgn_backlog(c.h, out.ctypes.data_as(C.POINTER(sgn.BacklogRow)), n_rows - 1, C.byref(n), C.byref(info))
    assert rc == ERANGE and n.value == n_rows and info.rows == n_rows and np.all(out.view(np.uint8) == 0xAB)
    assert c.L.sgn_backlog(c.h, None, 5, C.byref(n), C.byref(info)) == EINVAL
    assert c.L.sgn_backlog(c.h, None, 0, None, C.byref(info)) == EINVAL
    assert c.L.sgn_backlog(c.h, None, 0, C.byref(n), None) == EINVAL
    big = c.backlog(cap=n_rows + 7)  # (a larger array: the rows, no more)
    assert np.array_equal(big.rows, full.rows) and big.info == full.info
    c2 = ctxf()
    assert c2.L.sgn_backlog(c2.h, None, 0, C.byref(n), C.byref(info)) == ESTATE  # no simulation


# ---- 10. snapshot ----
def test_snapshot(ctxf, periodic):
    args, o, xs = periodic
    c = make(ctxf, args)
    c.run_until(bm.PERIODIC_TARGETS[4])
    at_save = c.backlog()
    check(at_save, xs[4])
    snap = c.snapshot_save()
    c.run_until(bm.PERIODIC_TARGETS[7])
    later = c.backlog()
    check(later, xs[7])
    assert later.info != at_save.info
    c.snapshot_restore(snap)
    again = c.backlog()
    assert again.info == at_save.info and again.rows.tobytes() == at_save.rows.tobytes()
    c.snapshot_free(snap)


# ---- 11. two shards in one process ----
def two_shards(ctxf, args):
    g, used, hosts, cfg, tr = args
    shards = []
    for r in range(2):
        c = ctxf(shard_rank=r, shard_count=2)
        c.routes_build(g, used)
        c.hosts_set(hosts)
        shards.append(c)
    arr = (C.c_void_p * 2)(*[c.h.value for c in shards])
    shards[0].check(shards[0].L.sgn_comm_init_local(arr, 2, 1 << 16))
    for c in shards:
        c.sim_init(cfg, tr)
    return shards


def test_two_shards(ctxf, periodic):
    args, o, xs = periodic
    shards = two_shards(ctxf, args)
    single = make(ctxf, args)
    for t, x in list(zip(bm.PERIODIC_TARGETS, xs))[:6]:
        sgn.shards_run_until(shards, t)
        single.run_until(t)
        a, b = shards[0].backlog(), shards[1].backlog()
        check(a, x, 0, 100)
        check(b, x, 100, 200)
        one = single.backlog()
        assert np.concatenate([a.rows, b.rows]).tobytes() == one.rows.tobytes()
        assert [p + q for p, q in zip(a.info["total"], b.info["total"])] == one.info["total"]


# ---- 12. run_sampled(backlog=True) ----
def test_run_sampled_backlog(ctxf, periodic):
    args, o, xs = periodic
    until = bm.PERIODIC_TARGETS[-1]
    c = make(ctxf, args)
    c.sample_enable(400)
    s = sgn.run_sampled(c, 20 * MS, until=until, backlog=True)
    assert len(s) == 10 and s.backlog_total.shape == (10, 8) and s.backlog_max_router.shape == (10,)
    assert np.array_equal(s.backlog_total, np.array([x.total() for x in xs], dtype=np.uint64))
    assert np.array_equal(s.backlog_max_router, [x.maxima()[0] for x in xs])
    # without the keyword: what it returned before
    c2 = make(ctxf, args)
    c2.sample_enable(400)
    s2 = sgn.run_sampled(c2, 20 * MS, until=until)
    assert s2.rows.tobytes() == s.rows.tobytes() and s2.infos.tobytes() == s.infos.tobytes()
    assert not hasattr(s2, "backlog_total") and not hasattr(s2, "backlog_max_router")
    # two shards: summed and maxed
    shards = two_shards(ctxf, args)
    for sh in shards:
        sh.sample_enable(400)
    sa, sb = sgn.run_sampled(shards, 20 * MS, until=until, backlog=True)
    assert np.array_equal(sa.backlog_total, s.backlog_total) and np.array_equal(sb.backlog_total, s.backlog_total)
    assert np.array_equal(sa.backlog_max_router, s.backlog_max_router)
