"""Interval statistics (-m gpu): sgn_sample_* (sample.hip) and sgn.run_sampled against the oracle.

The expected values never come from libsgn. The oracle (trace=True) is stepped round by round to the
edges sgn_run_until stops at — round() while the simulation is active and the window starts below
the target — and at each edge its cumulative per-host figures are taken: digests()' n_sent /
n_popped / n_delivered / n_codel_dropped, and per-host counts of its trace's SEND records with
flags == 2 (unknown destination) and of its LOCAL records. `blocked` has no per-host oracle figure:
its per-sample sum is compared with the growth of the oracle's stats()["app_blocked"], and a host
whose only change is `blocked` is the one kind of row the per-host figures do not predict. All seven
totals of a sample are compared with the growth of the oracle's stats(), rounds and window of every
info with the oracle's. The figures quoted in the tests' comments are the oracle's own and are
asserted on the oracle alone.
"""
import ctypes as C

import numpy as np
import pytest

import sgn
from external_common import datagrams, drive_ahead, external_world
from test_gpu_parity import assert_same_run, ctxf, scenario  # noqa: F401 (ctxf: a fixture)

pytestmark = pytest.mark.gpu

S0 = sgn.SIMULATION_START
ESTATE, EOVERFLOW, ERANGE, EINVAL = -71, -75, -34, -22
PER_HOST = ("sent", "popped", "delivered", "codel_dropped", "unknown_dst", "local_delivered")  # blocked: sums only
STATS = ("packets_sent", "packet_events_popped", "delivered", "codel_dropped", "packets_unknown_dst",
         "local_delivered", "app_blocked")  # sgn_sample_info::total order
EXT_STEP = 20_000_000


# ---- the oracle at the sample edges ----
def next_target(ws, interval, until=None):
    t = S0 + ((ws - S0) // interval + 1) * interval
    return t if until is None else min(t, until)


def edge_of(o):
    d = o.digests(0, o.n)
    return {"win": o.window(), "stats": o.stats(), "trace_n": int(o.L.ora_sim_trace_count(o.h)),
            "dig": np.stack([d["n_sent"], d["n_popped"], d["n_delivered"], d["n_codel_dropped"]]).astype(np.uint64)}


def oracle_edges(o, interval, until=None):
    """Steps the oracle as run_sampled steps libsgn; one entry per sample."""
    edges = []
    while True:
        ws, _, active = o.window()
        if not active or (until is not None and ws >= until):
            return edges
        t = next_target(ws, interval, until)
        while True:
            ws, _, active = o.window()
            if not active or ws >= t:
                break
            o.round()
        edges.append(edge_of(o))


def cumulative(edges, trace, n):
    """[edges, 6, n]: the per-host figures at every edge (PER_HOST order). The oracle appends its
    trace as it runs: the records up to an edge are a prefix."""
    unknown = (trace["kind"] == sgn.TRACE_SEND) & (trace["flags"] == 2)
    local = trace["kind"] == sgn.TRACE_LOCAL
    out = np.zeros((len(edges), 6, n), dtype=np.uint64)
    for k, e in enumerate(edges):
        t = trace[: e["trace_n"]]
        out[k, :4] = e["dig"]
        out[k, 4] = np.bincount(t["host"][unknown[: e["trace_n"]]], minlength=n)
        out[k, 5] = np.bincount(t["host"][local[: e["trace_n"]]], minlength=n)
    return out


class Expect:
    """What a run sampled at every edge from the start returns."""

    def __init__(self, o, interval, until=None):
        self.n = o.n
        zero = edge_of(o)
        assert zero["stats"]["packets_sent"] == 0 and zero["trace_n"] == 0  # (the baseline: a fresh simulation)
        self.edges = oracle_edges(o, interval, until)
        trace = o.trace()
        cum = cumulative([zero] + self.edges, trace, o.n)
        self.delta = cum[1:] - cum[:-1]                          # [samples, 6, n]
        st = [zero["stats"]] + [e["stats"] for e in self.edges]
        self.total = np.array([[b[f] - a[f] for f in STATS] for a, b in zip(st[:-1], st[1:])], dtype=np.uint64)
        self.active = (self.delta != 0).any(axis=1)              # [samples, n]: hosts the per-host figures predict
        self.busy = (self.delta[:, :4] != 0).any(axis=1).sum(axis=1)  # [samples]: hosts whose digest counters moved
        assert np.array_equal(self.delta.sum(axis=2), self.total[:, :6])  # (the oracle agrees with itself)

    def __len__(self):
        return len(self.edges)


def check_sample(rows, info, exp, k, lo=0, hi=None, index=None, whole=True):
    """The rows of one sample (of the hosts [lo, hi) of one context) against sample k of exp."""
    hi = exp.n if hi is None else hi
    what = (k, lo, hi)
    assert info["rows"] == len(rows), what
    assert int(info["sample"]) == (k if index is None else index) and np.all(rows["sample"] == info["sample"]), what
    e = exp.edges[k]
    assert (int(info["rounds"]), int(info["window_start"]), int(info["window_end"])) == (e["stats"]["rounds"],) + e["win"][:2], what
    h = rows["host"].astype(np.int64)
    assert np.all(np.diff(h) > 0) and (len(h) == 0 or (h[0] >= lo and h[-1] < hi)), what  # ascending, owned
    got = np.stack([rows[f] for f in PER_HOST])                  # [6, rows]
    assert np.array_equal(got, exp.delta[k][:, h]), what
    # no row for an unchanged host, every changed host has one; the rows the per-host figures do not
    # predict are those of hosts that only had sends refused
    known = exp.active[k][h]
    assert np.all(rows["blocked"][~known] > 0), what
    assert set(np.nonzero(exp.active[k][lo:hi])[0] + lo) <= set(h.tolist()), what
    tot = np.array([rows[f].sum(dtype=np.uint64) for f in sgn.SAMPLE_FIELDS], dtype=np.uint64)
    assert np.array_equal(tot, np.asarray(info["total"], dtype=np.uint64)), what  # the device's fold
    if whole:
        assert np.array_equal(tot, exp.total[k]), (what, tot, exp.total[k])
    return tot


def check_samples(s, exp, lo=0, hi=None, whole=True):
    assert len(s) == len(exp), (len(s), len(exp))
    tots = []
    for k in range(len(exp)):
        i = s.infos[k]
        rows = s.rows[int(i["first_row"]): int(i["first_row"] + i["rows"])]
        tots.append(check_sample(rows, i, exp, k, lo, hi, whole=whole))
    return np.array(tots)


def make(ctxf, args, row_capacity=None, **kw):
    g, used, hosts, cfg, tr = args
    c = ctxf(**kw)
    c.routes_build(g, used)
    c.hosts_set(hosts)
    c.sim_init(cfg, tr)
    if row_capacity:
        c.sample_enable(row_capacity)
    return c


def ref(oracle, args):
    g, used, hosts, cfg, tr = args
    lat, loss = oracle.routes(g, used)
    return oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=True)


def rc_of(fn, *a):
    with pytest.raises(sgn.SgnError) as e:
        fn(*a)
    return e.value


# ---- the oracle, once per scenario (never modified afterwards) ----
PERIODIC = dict(n=200, V=50, period_ns=5_000_000, stop_ns=30_000_000)
MS = 1_000_000


@pytest.fixture(scope="module")
def periodic(oracle):
    args = scenario(**PERIODIC)
    o = ref(oracle, args)
    return args, o, Expect(o, MS)


@pytest.fixture(scope="module")
def periodic1100(oracle):
    args = scenario(**dict(PERIODIC, n=1100))
    o = ref(oracle, args)
    return args, o, Expect(o, MS)


@pytest.fixture(scope="module")
def tgen(oracle):
    bw = np.where(np.arange(300) % 10 == 0, 100_000_000, 4_000_000).astype(np.uint64)
    args = scenario(n=300, V=30, kind=sgn.TRAFFIC_TGEN, stop_ns=2_000_000_000, bw=bw, tor=True, tgen_think=200_000_000)
    o = ref(oracle, args)
    return args, o, Expect(o, 100 * MS)


@pytest.fixture(scope="module")
def blocked(oracle):
    args = scenario(n=100, bw=1_000_000, fifo=2, period_ns=500_000, stop_ns=100_000_000)
    o = ref(oracle, args)
    return args, o, Expect(o, 10 * MS)


# the sampled libsgn runs that several tests look at (run once: {name: (context, Samples)})
@pytest.fixture(scope="module")
def runs():
    return {}


def sampled(runs, ctxf, name, args, interval):
    if name not in runs:
        # (a capacity of two samples at most: run_sampled takes whenever more than half is pending)
        c = make(ctxf, args, row_capacity=2 * args[2].n)
        runs[name] = (c, sgn.run_sampled(c, interval))
    return runs[name]


# ---- 1. PERIODIC layout (the dense n_cnt rows, permuted slots), compaction gaps ----
def test_periodic_rows(ctxf, periodic, runs):
    args, o, exp = periodic
    n_act = exp.active.sum(axis=1)
    assert len(exp) == 28 and exp.busy.min() == 1 and exp.busy.max() == 83
    assert 0 < n_act.min() and n_act.max() < 200  # every sample has rows, and compaction gaps
    assert exp.total[:, 4].sum() == 12 and exp.total[:, 5].sum() == 4   # unknown-destination and local packets
    c, s = sampled(runs, ctxf, "periodic", args, MS)
    check_samples(s, exp)
    assert np.array_equal(s.infos["sample"], np.arange(28))
    # the dense forms: a [samples, hosts] array per field, and its running sum
    for f, field in enumerate(PER_HOST):
        assert np.array_equal(s.dense(field, 200), exp.delta[:, f])
    assert np.array_equal(s.cumulative("sent", 200)[-1], o.digests(0, 200)["n_sent"])
    t = c.sample_timing()
    assert t["hosts"] == 200 and t["rows"] == int(s.infos["rows"][-1]) and t["total_ms"] > 0


# ---- 2. scan-tile and wave boundaries ----
def test_periodic_1100_hosts(ctxf, periodic1100):
    """1100 hosts: 18 waves (the last one of 12 lanes), five workgroups of k_sample_count."""
    args, o, exp = periodic1100
    assert len(exp) == 30 and exp.busy.min() == 13 and exp.busy.max() == 394
    c = make(ctxf, args, row_capacity=2200)
    check_samples(sgn.run_sampled(c, MS), exp)


@pytest.mark.parametrize("n", [63, 64, 65])
def test_wave_boundary(ctxf, oracle, n):
    args = scenario(**dict(PERIODIC, n=n, stop_ns=10_000_000))
    exp = Expect(ref(oracle, args), MS)
    assert len(exp) >= 5 and exp.active.any(axis=0).sum() > n // 2 and exp.active[:, n - 1].any()
    c = make(ctxf, args, row_capacity=2 * n)
    check_samples(sgn.run_sampled(c, MS), exp)


# ---- 3. TGEN layout (the counters in the host records), CoDel drops ----
def test_tgen_rows(ctxf, tgen, runs):
    args, o, exp = tgen
    assert len(exp) == 20 and exp.busy.min() == 111 and exp.busy.max() == 300
    assert exp.total[:, 3].sum() == 16_272  # CoDel drops
    c, s = sampled(runs, ctxf, "tgen", args, 100 * MS)
    check_samples(s, exp)
    assert np.array_equal(s.cumulative("codel_dropped", 300)[-1], o.digests(0, 300)["n_codel_dropped"])


# ---- 4. blocked sends, local deliveries ----
def test_blocked_and_local(ctxf, blocked):
    args, o, exp = blocked
    assert exp.total[:, 6].sum() == 18_102 and exp.total[:, 5].sum() == 9 and exp.total[:, 4].sum() == 13
    c = make(ctxf, args, row_capacity=200)
    s = sgn.run_sampled(c, 10 * MS)
    tots = check_samples(s, exp)
    assert np.array_equal(tots[:, 6], exp.total[:, 6]) and tots[:, 6].sum() == o.stats()["app_blocked"]


# ---- 5. the simulation is untouched ----
def test_simulation_untouched_periodic(ctxf, periodic, runs):
    args, o, _ = periodic
    c, _ = sampled(runs, ctxf, "periodic", args, MS)
    assert not o.window()[2]
    assert_same_run(o, c, 200, trace=False)


def test_simulation_untouched_tgen(ctxf, tgen, runs):
    args, o, _ = tgen
    c, _ = sampled(runs, ctxf, "tgen", args, 100 * MS)
    assert not o.window()[2]
    assert_same_run(o, c, 300, trace=False)


# ---- 6. overflow and take ----
def step(c, interval=MS):
    """To the next sample edge; False at the end."""
    ws, _, active = c.window()
    if not active:
        return False
    c.run_until(next_target(ws, interval))
    return True


def test_overflow_and_take(ctxf, periodic):
    args, o, exp = periodic
    r = exp.active.sum(axis=1)  # (scenario 1 refuses no send: the rows are the active hosts)
    assert exp.total[:, 6].sum() == 0 and r[0] >= 2 and r[1] >= 2
    # a buffer below one sample's rows
    c = make(ctxf, args, row_capacity=int(r[0]) - 1)
    assert step(c)
    e = rc_of(c.sample)
    assert e.rc == EOVERFLOW and str(int(r[0])) in str(e), e
    assert c.sample_pending() == (0, 0)
    assert rc_of(c.sample).rc == EOVERFLOW and c.sample_pending() == (0, 0)
    c.close()
    # a buffer of about 1.5 samples
    cap = int(max(r[0], r[1]) + min(r[0], r[1]) // 2)
    assert max(r[0], r[1]) <= cap < r[0] + r[1]
    c = make(ctxf, args, row_capacity=cap)
    assert rc_of(c.sample_enable, 0).rc == EINVAL and c.sample_pending() == (0, 0)
    assert step(c)
    i0 = c.sample()
    assert (i0["sample"], i0["first_row"], i0["rows"]) == (0, 0, r[0]) and c.sample_pending() == (r[0], 1)
    assert step(c)
    e = rc_of(c.sample)
    assert e.rc == EOVERFLOW and c.sample_pending() == (r[0], 1)
    # a take one row short, and one without room for the info, take nothing
    for cap_rows, cap_infos in ((int(r[0]) - 1, 1), (int(r[0]), 0)):
        e = rc_of(c.sample_take, cap_rows, cap_infos)
        assert e.rc == ERANGE and e.needed == (r[0], 1) and c.sample_pending() == (r[0], 1)
    rows, infos = c.sample_take()
    assert len(infos) == 1 and c.sample_pending() == (0, 0)
    check_sample(rows, infos[0], exp, 0)
    # the refused sample changed nothing: the same call now returns exactly sample 1
    i1 = c.sample()
    assert (i1["sample"], i1["first_row"], i1["rows"]) == (1, 0, r[1])
    rows, infos = c.sample_take()
    check_sample(rows, infos[0], exp, 1)
    assert c.sample_take()[0].size == 0  # (nothing pending: an empty take)


# ---- 7. rewind ----
def test_rewind_and_rebase(ctxf, periodic):
    args, o, exp = periodic
    c = make(ctxf, args, row_capacity=4000)
    for k in range(6):
        assert step(c) and c.sample()["sample"] == k
    snap = c.snapshot_save()
    first = []
    for k in range(6, 11):
        assert step(c)
        first.append(c.sample())
    rows, infos = c.sample_take()
    for k in range(11):
        i = infos[k]
        check_sample(rows[int(i["first_row"]): int(i["first_row"] + i["rows"])], i, exp, k)
    c.snapshot_restore(snap)
    for _ in range(2):
        e = rc_of(c.sample)
        assert e.rc == ESTATE and "sgn_sample_rebase" in str(e) and c.sample_pending() == (0, 0)
    c.sample_rebase()
    assert c.sample_pending() == (0, 0)
    for k in range(6, 11):
        assert step(c)
        i = c.sample()
        assert i["sample"] == k + 5  # the index goes on from 11
        assert (i["rounds"], i["window_start"], i["window_end"], i["rows"], i["total"]) == tuple(
            first[k - 6][f] for f in ("rounds", "window_start", "window_end", "rows", "total"))
    rows2, infos2 = c.sample_take()
    assert np.array_equal(infos2["sample"], np.arange(11, 16))
    again = rows[int(infos[6]["first_row"]):]
    for f in ("host",) + sgn.SAMPLE_FIELDS:
        assert np.array_equal(rows2[f], again[f]), f
    for k in range(6, 11):
        i = infos2[k - 6]
        check_sample(rows2[int(i["first_row"]): int(i["first_row"] + i["rows"])], i, exp, k, index=k + 5)
    c.snapshot_free(snap)


# ---- 8. two shards in one process ----
def test_two_shards(ctxf, periodic):
    args, o, exp = periodic
    assert exp.total[:, 6].sum() == 0  # (no send refused: the rows are the hosts the per-host figures predict)
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
        c.sample_enable(400)
    a, b = sgn.run_sampled(shards, MS)
    check_samples(a, exp, 0, 100, whole=False)
    check_samples(b, exp, 100, 200, whole=False)
    for f in ("sample", "rounds", "window_start", "window_end"):
        assert np.array_equal(a.infos[f], b.infos[f]), f
    assert np.array_equal(a.infos["total"] + b.infos["total"], exp.total)
    # the two contexts' rows, joined per sample, are the unsharded rows
    for k in range(len(exp)):
        ia, ib = a.infos[k], b.infos[k]
        rows = np.concatenate([a.rows[int(ia["first_row"]): int(ia["first_row"] + ia["rows"])],
                               b.rows[int(ib["first_row"]): int(ib["first_row"] + ib["rows"])]])
        assert np.array_equal(np.nonzero(exp.active[k])[0], rows["host"])
        assert np.array_equal(np.stack([rows[f] for f in PER_HOST]), exp.delta[k][:, rows["host"]])


# ---- 9. EXTERNAL traffic ----
def test_external(ctxf, oracle):
    world = external_world()
    n = world[2].n
    dg = datagrams(world[2])
    o = ref(oracle, world)
    c = make(ctxf, world, row_capacity=40 * n)
    edges = [edge_of(o)]
    infos = []

    def on_step(_k):
        edges.append(edge_of(o))
        infos.append(c.sample())

    drive_ahead([o, c], dg, EXT_STEP, on_step=on_step)
    cum = cumulative(edges, o.trace(), n)
    delta = cum[1:] - cum[:-1]
    # (the oracle's run: 17 steps; 397 sends, 25 to unknown addresses, 40 local, 119 refused)
    assert len(infos) >= 5 and cum[-1, 0].sum() > 300 and cum[-1, 4].sum() > 0 and cum[-1, 5].sum() > 0
    assert edges[-1]["stats"]["app_blocked"] > 0
    rows, got = c.sample_take()
    assert len(got) == len(infos) and np.array_equal(got["rows"], [i["rows"] for i in infos])
    s = sgn.Samples(rows, got)
    for f, field in enumerate(PER_HOST):
        assert np.array_equal(s.dense(field, n), delta[:, f]), field
    for k, e in enumerate(edges[1:]):
        i = got[k]
        r = rows[int(i["first_row"]): int(i["first_row"] + i["rows"])]
        assert np.all(np.diff(r["host"].astype(np.int64)) > 0) and np.all(r["sample"] == k)
        assert (int(i["rounds"]), int(i["window_start"]), int(i["window_end"])) == (e["stats"]["rounds"],) + e["win"][:2]
        want = [e["stats"][f] - edges[k]["stats"][f] for f in STATS]
        assert want == [int(v) for v in i["total"]], (k, want, i["total"])
