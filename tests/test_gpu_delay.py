"""The router delay report (-m gpu): sgn_delay_enable / _fold / _get / _clear and
sgn_selftest_delay_fold (delay.hip).

The kernels alone run on record streams drawn here, through the self-test call, against the model of
tests/delay_model.py, which matches by key where the kernels match by rank. The class limits (records
a wave, and a workgroup per pass, handle at once) are read from the timing struct, so the shapes
follow them. The simulations run the fan-in scenario of tests/drain_take_cases.py beside the oracle,
whose ONE trace (a module fixture, never modified) goes through the model: every row, total and
histogram bin is an integer and is compared exactly."""
import ctypes as C
import re

import numpy as np
import pytest

import sgn
from delay_model import CODEL_DROP, DELIVER, POP, DelayModel, assert_report, ordered, run_model
from drain_take_cases import MS, S0, fan_in_case
from test_gpu_external import run_group, shard_ranges, submit_to_owners
from test_gpu_parity import assert_same_run, ctxf  # noqa: F401 (ctxf: fixture)

pytestmark = pytest.mark.gpu

EDEVICE, ESTATE = -5, -71
HOST_LO = 1000  # the self-test's host range starts here
NOISE = (sgn.TRACE_SEND, sgn.TRACE_IF_POP, sgn.TRACE_LOCAL)


@pytest.fixture(scope="module")
def dctx():
    c = sgn.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def limits(dctx):
    t = dctx.delay_timing()
    assert t["wave_max"] == 64 and t["tile"] > t["wave_max"] and t["tile"] % 64 == 0, t
    return t["wave_max"], t["tile"]


def stream(rng, host, m, standing0=0, noise=0.15, p_exit=0.45):
    """m records of one host in seq order: a FIFO router fed by POPs and emptied by DELIVER / CODEL_DROP
    exits, other kinds in between; the first standing0 exits are of packets popped before the stream
    began (keys no POP of the stream has). Times never decrease, so some delays are 0."""
    r = np.zeros(m, sgn.TRACE_DTYPE)
    r["host"] = host
    r["seq"] = np.arange(m, dtype=np.uint64) + np.uint64(rng.integers(0, 1000))
    r["rng_pos"] = rng.integers(0, 1 << 40, m)
    r["b"] = rng.integers(0, 1 << 40, m)
    queue = [None] * standing0
    t, eid = 1000 + int(rng.integers(0, 50)), int(rng.integers(0, 1 << 40))
    for i in range(m):
        t += int(rng.integers(0, 4)) * int(rng.integers(0, 1000))
        u = rng.random()
        if u < noise:
            r[i]["kind"], r[i]["peer"], r[i]["c"], r[i]["a"] = NOISE[int(rng.integers(0, 3))], rng.integers(0, 50), rng.integers(0, 1 << 40), t
        elif queue and u < noise + p_exit:
            e = queue.pop(0)
            peer, c = e if e is not None else (0xFFFF0000 + i % 7, (1 << 50) + i)
            r[i]["kind"], r[i]["peer"], r[i]["c"], r[i]["a"] = (DELIVER if rng.random() < 0.7 else CODEL_DROP), peer, c, t
            r[i]["flags"] = 0
        else:
            eid += 1 + int(rng.integers(0, 3))
            peer = int(rng.integers(0, 50))
            queue.append((peer, eid))
            r[i]["kind"], r[i]["peer"], r[i]["c"], r[i]["a"] = POP, peer, eid, t
    return r


def check(c, recs, ends, n_hosts, standing0=None, lo=HOST_LO, what=""):
    d = sgn.selftest_delay_fold(c, recs, ends, lo, n_hosts, standing0)
    rows, info = run_model(recs, ends, standing0, lo)
    assert_report(d, rows, info, what)
    assert d.info["hosts"] == n_hosts and np.all(d.rows["reserved"] == 0)
    assert d.info["total"][0] == sum(d.info["hist_delivered"]) and d.info["total"][1] == sum(d.info["hist_dropped"])
    return d


def size_of(label, wave, tile):
    """'2' -> 2, 'W-1' -> wave - 1, '3T+5' -> 3 * tile + 5."""
    m = re.fullmatch(r"(?:(\d*)([WT]))?([+-]?\d+)?", label)
    unit = {"W": wave, "T": tile, None: 0}[m.group(2)]
    return int(m.group(1) or 1) * unit + int(m.group(3) or 0)


def classes_of(recs, wave):
    count = np.bincount(recs["host"] - HOST_LO)
    count = count[count > 0]
    return [int((count <= wave).sum()), int((count > wave).sum())]


@pytest.mark.parametrize("n", [0, 1])
def test_empty_and_single(dctx, n):
    recs = stream(np.random.default_rng(n), HOST_LO + 2, n, noise=0)
    d = check(dctx, recs, [n], 4)
    assert d.info["rows"] == n and d.info["total"][4] == n  # the one record is a POP: it stands
    check(dctx, recs, [], 4)  # no piece at all
    check(dctx, recs, [0, n, n], 4, standing0=[0, 0, 3, 0])  # empty pieces are folds too


@pytest.mark.parametrize("label", ["2", "W-1", "W", "W+1", "T-1", "T", "T+1", "2T+1", "3T+5"])
def test_one_host(dctx, limits, label):
    m = size_of(label, *limits)
    rng = np.random.default_rng(m)
    recs = stream(rng, HOST_LO + 1, m)
    d = check(dctx, recs, [m], 3, what=label)
    t = dctx.delay_timing()
    assert t["spans_by_class"] == classes_of(recs, limits[0]) and t["largest_span"] == m and t["records"] == m
    assert d.info["total"][0] + d.info["total"][1] > 0 or m < 8
    recs = stream(rng, HOST_LO + 1, m, standing0=2)
    check(dctx, recs[rng.permutation(m)], [m], 3, standing0=[0, 2, 0], what=label + " shuffled")


@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 1025])
def test_many_small_hosts(dctx, n_hosts):
    """0 to 6 records a host, some hosts empty, some with packets standing at the start; 1025 hosts
    cross a tile of the scan."""
    rng = np.random.default_rng(n_hosts)
    per = rng.integers(0, 7, n_hosts)
    standing0 = rng.integers(0, 3, n_hosts).astype(np.uint32)
    recs = np.concatenate([np.zeros(0, sgn.TRACE_DTYPE)] +
                          [stream(rng, HOST_LO + h, int(per[h]), int(standing0[h])) for h in range(n_hosts)])
    recs = recs[rng.permutation(len(recs))]
    d = check(dctx, recs, [len(recs)], n_hosts, standing0)
    assert d.info["total"][5] > 0 or n_hosts == 1  # unmatched exits


def test_one_large_host_among_small_ones(dctx, limits):
    rng = np.random.default_rng(77)
    per = rng.integers(0, 7, 201)
    per[117] = 3 * limits[1]
    recs = np.concatenate([stream(rng, HOST_LO + h, int(per[h])) for h in range(201)])
    recs = recs[rng.permutation(len(recs))]
    check(dctx, recs, [len(recs)], 201)
    assert dctx.delay_timing()["spans_by_class"][1] == 1


@pytest.mark.parametrize("order", ["ordered", "reversed"])
def test_presorted_input(dctx, limits, order):
    rng = np.random.default_rng(5)
    per = [3, limits[0], limits[0] + 1, limits[1], 2 * limits[1] + 9, 0, 1]
    recs = ordered(np.concatenate([stream(rng, HOST_LO + h, m, standing0=h % 2) for h, m in enumerate(per)]))
    check(dctx, recs[::-1].copy() if order == "reversed" else recs, [len(recs)], len(per), standing0=[h % 2 for h in range(len(per))])


def test_pieces_cross_the_carry_at_the_class_borders(dctx, limits):
    """One host's stream cut so that successive spans are a wave's, a workgroup's and a wave's again,
    with packets standing at every cut (p_exit is low: the queue grows), beside a host whose pieces
    stay small and one that appears in the last piece only."""
    wave, tile = limits
    rng = np.random.default_rng(11)
    a = stream(rng, HOST_LO, 2 * tile + 2 * wave + 7, standing0=3, p_exit=0.3)
    b = stream(rng, HOST_LO + 1, 40, p_exit=0.3)
    cuts_a = [wave - 1, 2 * wave, 2 * wave + tile + 1, 2 * wave + tile + 6, len(a)]
    cuts_b = [5, 6, 20, 20, 40]
    late = stream(rng, HOST_LO + 4, 70)
    pieces, pa, pb = [], 0, 0
    for i, (ea, eb) in enumerate(zip(cuts_a, cuts_b)):
        p = np.concatenate([a[pa:ea], b[pb:eb]] + ([late] if i == len(cuts_a) - 1 else []))
        pieces.append(p[rng.permutation(len(p))])
        pa, pb = ea, eb
    recs = np.concatenate(pieces)
    ends = np.cumsum([len(p) for p in pieces])
    # the carry is crossed: a packet popped in one piece exits in a later one, at every cut
    m = DelayModel([3, 0, 0, 0, 0], HOST_LO)
    for p in pieces[:-1]:
        m.fold(p)
        assert m.result()[0][0]["standing"] > 0
    d = check(dctx, recs, ends, 5, standing0=[3, 0, 0, 0, 0])
    assert d.info["folds"] == 5 and d.info["total"][5] == 3
    whole = check(dctx, np.concatenate([a, b, late]), [len(recs)], 5, standing0=[3, 0, 0, 0, 0])
    assert whole.rows.tobytes() == d.rows.tobytes()


def test_standing0_exits_are_unmatched(dctx, limits):
    rng = np.random.default_rng(21)
    recs = np.concatenate([stream(rng, HOST_LO + h, m, standing0=s, p_exit=0.6)
                           for h, (m, s) in enumerate([(30, 5), (limits[0] + 9, 70), (limits[1] + 3, 100), (4, 9)])])
    d = check(dctx, recs[rng.permutation(len(recs))], [len(recs)], 4, standing0=[5, 70, 100, 9])
    assert d.rows["unmatched"][0] == 5 and np.all(d.rows["unmatched"] > 0)
    assert d.rows["standing"][3] > 0 and d.rows["standing_oldest"][3] == sgn.EMUTIME_INVALID  # unknown packets still stand


def test_bin_edges_and_wide_sums(dctx):
    """Delays of exactly 0, 1, 2^k - 1 and 2^k for k in 1, 20, 32, 46, 47: each in its bin, the sums
    and the maximum in 64 bits."""
    delays = [0, 1] + [v for k in (1, 20, 32, 46, 47) for v in ((1 << k) - 1, 1 << k)]
    bins = [0, 1, 1, 2, 20, 21, 32, 33, 46, 47, 47, 47]
    r = np.zeros(2 * len(delays), sgn.TRACE_DTYPE)
    r["host"], r["seq"] = HOST_LO + 1, np.arange(len(r)) + 17
    t = 5
    for i, d in enumerate(delays):
        r[2 * i]["kind"], r[2 * i]["a"] = POP, t
        r[2 * i + 1]["kind"], r[2 * i + 1]["a"] = (DELIVER, CODEL_DROP)[i % 2], t + d
        r["peer"][2 * i: 2 * i + 2], r["c"][2 * i: 2 * i + 2] = 7 + i, (1 << 40) + i
        t += d + 3
    d = check(dctx, r, [len(r)], 2)
    hist = np.array(d.info["hist_delivered"]) + np.array(d.info["hist_dropped"])
    assert hist.tolist() == np.bincount(bins, minlength=sgn.DELAY_BINS).tolist()
    assert d.info["hist_dropped"][47] == 2 and d.info["hist_delivered"][47] == 1
    row = d.rows[0]
    assert row["delay_sum_delivered"] == sum(delays[0::2]) > 1 << 46 and row["delay_sum_dropped"] == sum(delays[1::2]) > 1 << 47
    assert row["delay_max"] == 1 << 47 == d.info["delay_max"] and d.info["delay_max_host"] == HOST_LO + 1
    assert d.quantile(1.0) == sgn.EMUTIME_INVALID and d.quantile(0.01) == 0


@pytest.mark.parametrize("m", ["40", "T+50"])
@pytest.mark.parametrize("what", ["keys", "time", "one exit too many"])
def test_bad_streams_are_refused(dctx, limits, what, m):
    """A pair whose keys disagree, an exit earlier than its pop, a host with one exit too many:
    SGN_EDEVICE naming the host, in the wave's kernel and in the workgroup's; the same call on the
    correct stream then gives the correct report."""
    m = size_of(m, *limits)
    rng = np.random.default_rng(m)
    good = np.concatenate([stream(rng, HOST_LO + 2, 30), stream(rng, HOST_LO + 5, m, p_exit=0.5), stream(rng, HOST_LO + 6, 9)])
    bad = good.copy()
    at5 = np.nonzero(bad["host"] == HOST_LO + 5)[0]
    exits = at5[(bad["kind"][at5] == DELIVER) | (bad["kind"][at5] == CODEL_DROP)]
    if what == "keys":
        bad["c"][exits[len(exits) // 2]] += 1
    elif what == "time":
        bad["a"][exits[len(exits) // 2]] = 1
    else:  # the queue's rest leaves at the stream's end, and one more
        extra = np.zeros(int((bad["kind"][at5] == POP).sum()) - len(exits) + 1, sgn.TRACE_DTYPE)
        extra["kind"], extra["host"], extra["a"] = DELIVER, HOST_LO + 5, bad["a"][at5].max()
        extra["seq"] = bad["seq"][at5].max() + np.uint64(1) + np.arange(len(extra), dtype=np.uint64)
        bad = np.concatenate([bad, extra])
    with pytest.raises(sgn.SgnError, match="host %d" % (HOST_LO + 5)) as e:
        sgn.selftest_delay_fold(dctx, bad, [len(bad)], HOST_LO, 8)
    assert e.value.rc == EDEVICE
    check(dctx, good, [len(good)], 8)


def test_short_cap_many_rows(dctx):
    """SGN_ERANGE on a short cap: the count needed, the info filled, nothing written."""
    rng = np.random.default_rng(8)
    recs = np.concatenate([stream(rng, HOST_LO + h, 12) for h in range(0, 300, 2)])
    full = check(dctx, recs, [len(recs)], 300)
    assert full.info["rows"] == 150
    for cap in (149, 1):
        rows = np.zeros(cap, sgn.DELAY_ROW_DTYPE)
        info, n = sgn.DelayInfo(), C.c_uint64()
        ends = np.array([len(recs)], np.uint64)
        rc = dctx.L.sgn_selftest_delay_fold(dctx.h, recs.ctypes.data_as(C.POINTER(sgn.TraceRec)), sgn.ptr(ends, C.c_uint64), 1, HOST_LO,
                                            300, None, rows.ctypes.data_as(C.POINTER(sgn.DelayRow)), cap, C.byref(n), C.byref(info))
        assert rc == sgn.ERANGE and n.value == 150 and sgn.Delay(info).info == full.info
        assert not rows.tobytes().strip(b"\0")


# ---- simulations, beside the oracle ----
TRACE_CAP = 1 << 16


def traced_oracle(oracle, world):
    g, used, hosts, cfg, tr = world
    lat, loss = oracle.routes(g, used)
    return oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=True)


def traced_ctx(ctxf, world, hosts=None, enable=True):
    g, used, hst, cfg, tr = world
    c = ctxf()
    c.routes_build(g, used)
    c.hosts_set(hst)
    c.trace_enable(TRACE_CAP)
    if hosts is not None:
        c.trace_hosts(hosts)
    c.drain_enable(1 << 16)
    c.sim_init(cfg, tr)
    if enable:
        c.delay_enable()
    return c


def submit_all(sims, dg):
    for s in sims:
        s.submit(dg[0], dg[1], dg[2], dg[3], dg[4], wire_len=dg[5])


@pytest.fixture(scope="module")
def fan_in(oracle, dctx):
    """The scenario, the oracle's run of it with its ordered trace, and the model's report of that."""
    tile = dctx.drain_take_timing()["tile"]
    world, dg, dst = fan_in_case(tile)
    o = traced_oracle(oracle, world)
    submit_all([o], dg)
    rounds = o.run()
    t = ordered(o.trace())
    rows, info = run_model(t)
    assert info["total"][1] >= 20 and info["delay_max"] > 1_000_000_000
    return dict(world=world, dg=dg, dst=dst, oracle=o, rounds=rounds, trace=t, rows=rows, info=info, n=world[2].n)


def expect(case, folds=None):
    info = dict(case["info"])
    if folds is None:
        del info["folds"]
    else:
        info["folds"] = folds
    return case["rows"], info


def test_lockstep_with_the_oracle(ctxf, oracle, fan_in):
    """A second oracle and libsgn round by round, a fold every 3 rounds and one at the end."""
    o = traced_oracle(oracle, fan_in["world"])
    c = traced_ctx(ctxf, fan_in["world"])
    assert c.delay().info["rows"] == 0  # right after sim_init nothing stands
    submit_all([o, c], fan_in["dg"])
    rounds = folds = 0
    standing = 0
    while True:
        assert o.window() == c.window()
        if not o.window()[2]:
            break
        assert o.round() == c.round()
        rounds += 1
        if rounds % 3 == 0:
            info = c.delay_fold()
            folds += 1
            standing = max(standing, info["total"][4])
            assert info["rounds"] > 0 and info["folds"] == folds and c.trace_pending() == 0
    c.delay_fold()
    d = c.delay()
    assert_report(d, *expect(fan_in, folds + 1))
    assert rounds == fan_in["rounds"] > 100 and standing > 100 and d.info["hosts"] == fan_in["n"]
    assert d.quantile(1.0) >= d.info["delay_max"] and d.quantile(0.5) > 0
    assert len(c.trace()) == 0
    assert_same_run(o, c, fan_in["n"], trace=False)  # the report changes nothing of the simulation


def test_standing_is_the_backlog(ctxf, fan_in):
    """Paused where packets stand: the carry is what sgn_backlog finds at the routers, and the whole
    report is the model's of the records taken so far (the takes fold them too). standing_oldest is
    router_oldest where the queue is not empty and relay_inet_in holds no packet — at these pauses the
    bottleneck's relay always holds one, so the model's value is what checks the head's pop time."""
    c = traced_ctx(ctxf, fan_in["world"])
    submit_all([c], fan_in["dg"])
    n = fan_in["n"]
    m = DelayModel()
    for t_ms in (60, 100, 150, 250, 400, 600, 900, 1200):
        c.run_until(S0 + t_ms * MS)
        m.fold(c.trace_take()[0])
        d, bl = c.delay(), c.backlog()
        assert_report(d, *m.result(), what=t_ms)
        held = (bl.dense("flags", n) & sgn.BACKLOG_ROUTER_HELD) != 0
        standing = np.zeros(n, np.uint64)
        standing[d.rows["host"]] = d.rows["standing"]
        assert np.array_equal(standing, bl.dense("router_packets", n) + held), t_ms
        oldest = np.zeros(n, np.uint64)
        oldest[d.rows["host"]] = d.rows["standing_oldest"]
        plain = (bl.dense("router_packets", n) > 0) & ~held
        assert np.array_equal(oldest[plain], bl.dense("router_oldest", n)[plain]), t_ms
        assert d.info["total"][4] == int(standing.sum())
        if t_ms == 400:
            assert standing[fan_in["dst"]] > 100 and oldest[fan_in["dst"]] not in (0, sgn.EMUTIME_INVALID)
    d = sgn.run_delays(c, 200 * MS)
    assert_report(d, *expect(fan_in))


def test_enable_at_an_edge_where_packets_stand(ctxf, fan_in):
    c = traced_ctx(ctxf, fan_in["world"], enable=False)
    submit_all([c], fan_in["dg"])
    c.run_until(S0 + 300 * MS)
    with pytest.raises(sgn.SgnError) as e:  # records are pending: the caller takes them first
        c.delay_enable()
    assert e.value.rc == ESTATE and "pending" in str(e.value)
    taken, _ = c.trace_take()
    bl = c.backlog()
    n = fan_in["n"]
    standing0 = (bl.dense("router_packets", n) + ((bl.dense("flags", n) & sgn.BACKLOG_ROUTER_HELD) != 0)).astype(np.uint32)
    assert standing0[fan_in["dst"]] > 100
    c.delay_enable()
    d0 = c.delay()
    assert np.array_equal(d0.rows["host"], np.nonzero(standing0)[0]) and np.array_equal(d0.rows["standing"], standing0[standing0 > 0])
    assert np.all(d0.rows["standing_oldest"] == sgn.EMUTIME_INVALID) and d0.info["total"][4] == int(standing0.sum())
    d = sgn.run_delays(c, 100 * MS)
    # the oracle's records after those the take handed out
    t = fan_in["trace"]
    last = np.full(n, -1, np.int64)
    np.maximum.at(last, taken["host"], taken["seq"].astype(np.int64))
    rest = t[t["seq"].astype(np.int64) > last[t["host"]]]
    assert len(rest) + len(taken) == len(t)
    rows, info = run_model(rest, standing0=standing0)
    del info["folds"]
    assert_report(d, rows, info)
    unmatched = np.zeros(n, np.uint64)
    unmatched[d.rows["host"]] = d.rows["unmatched"]
    assert np.array_equal(unmatched, standing0)


def test_trace_take_on_an_enabled_context(ctxf, fan_in):
    """Takes with the report enabled return the bytes and spans of takes without it, and the report
    is that of a run that only folds."""
    plain = traced_ctx(ctxf, fan_in["world"], enable=False)
    both = traced_ctx(ctxf, fan_in["world"])
    folds = traced_ctx(ctxf, fan_in["world"])
    submit_all([plain, both, folds], fan_in["dg"])
    k = 0
    while plain.window()[2]:
        k += 1
        for c in (plain, both, folds):
            c.run_until(S0 + k * 150 * MS)
        (ra, sa), (rb, sb) = plain.trace_take(), both.trace_take()
        assert ra.tobytes() == rb.tobytes() and sa.tobytes() == sb.tobytes()
        folds.delay_fold()
    assert k > 5 and plain.trace_pending() == both.trace_pending() == 0
    da, db = both.delay(), folds.delay()
    assert da.info == db.info and da.rows.tobytes() == db.rows.tobytes()
    assert_report(da, *expect(fan_in, k))


def test_trace_hosts_subset(ctxf, fan_in):
    hosts = [fan_in["dst"], 3, 21, 44]
    c = traced_ctx(ctxf, fan_in["world"], hosts=hosts)
    submit_all([c], fan_in["dg"])
    d = sgn.run_delays(c, 250 * MS)
    want = fan_in["rows"][np.isin(fan_in["rows"]["host"], hosts)]
    # (the fan-in has one destination: of the listed hosts only the bottleneck has a row)
    assert len(want) == 1 and want["host"][0] == fan_in["dst"] and d.rows.tobytes() == want.tobytes()
    assert d.info["total"][0] == int(want["delivered"].sum()) and d.info["delay_max_host"] == fan_in["dst"]


def test_subset_enable_seeds_only_listed_hosts(ctxf, fan_in):
    hosts = [3, 21]  # not the bottleneck: its queue stands, but it is not traced
    c = traced_ctx(ctxf, fan_in["world"], hosts=hosts, enable=False)
    submit_all([c], fan_in["dg"])
    c.run_until(S0 + 300 * MS)
    c.trace_take()
    assert c.backlog().dense("router_packets", fan_in["n"])[fan_in["dst"]] > 100
    c.delay_enable()
    assert set(c.delay().rows["host"].tolist()) <= set(hosts)


def test_two_shards(fan_in):
    """A local group of two: each shard's rows are the unsharded rows of the hosts it owns."""
    world, dg, n = fan_in["world"], fan_in["dg"], fan_in["n"]
    g, used, hosts, cfg, tr = world
    shards = [sgn.Context(shard_rank=r, shard_count=2) for r in range(2)]
    arr = (C.c_void_p * 2)(*[c.h.value for c in shards])
    for c in shards:
        c.routes_build(g, used)
        c.hosts_set(hosts)
        c.trace_enable(TRACE_CAP)
        c.drain_enable(1 << 16)
    shards[0].check(shards[0].L.sgn_comm_init_local(arr, 2, 1 << 14))
    for c in shards:
        c.sim_init(cfg, tr)
        c.delay_enable()
    ranges = shard_ranges(shards[0], n, 2)
    submit_to_owners(shards, ranges, dg, np.ones(len(dg[3]), bool))
    assert run_group(shards, arr) == fan_in["rounds"]
    seen = 0
    for c, (lo, hi) in zip(shards, ranges):
        c.delay_fold()
        d = c.delay()
        want = fan_in["rows"][(fan_in["rows"]["host"] >= lo) & (fan_in["rows"]["host"] < hi)]
        assert d.rows.tobytes() == want.tobytes() and d.info["hosts"] == hi - lo
        assert d.info["total"] == [int(want[f].sum(dtype=np.uint64)) for f in sgn.DELAY_TOTALS]
        seen += len(want)
    assert seen == len(fan_in["rows"])


def test_state_errors(ctxf, fan_in):
    g, used, hst, cfg, tr = fan_in["world"]
    c = ctxf()
    assert c.L.sgn_delay_enable(c.h) == ESTATE and c.L.sgn_delay_fold(c.h, None) == ESTATE  # no simulation
    c.routes_build(g, used)
    c.hosts_set(hst)
    c.drain_enable(1 << 16)
    c.sim_init(cfg, tr)
    with pytest.raises(sgn.SgnError, match="sgn_trace_enable") as e:  # a simulation without a trace
        c.delay_enable()
    assert e.value.rc == ESTATE
    c = traced_ctx(ctxf, fan_in["world"], enable=False)
    n64, info = C.c_uint64(5), sgn.DelayInfo()
    assert c.L.sgn_delay_fold(c.h, None) == ESTATE and "sgn_delay_enable" in c.L.sgn_last_error(c.h).decode()
    assert c.L.sgn_delay_get(c.h, None, 0, C.byref(n64), C.byref(info)) == ESTATE and n64.value == 0
    assert c.L.sgn_delay_clear(c.h) == ESTATE


def test_rewind_needs_a_new_enable(ctxf, fan_in):
    c = traced_ctx(ctxf, fan_in["world"])
    submit_all([c], fan_in["dg"])
    snap = c.snapshot_save()
    c.run_until(S0 + 200 * MS)
    c.delay_fold()
    c.run_until(S0 + 400 * MS)
    before = c.delay()
    c.snapshot_restore(snap)  # the taken count goes back to the save's
    for _ in range(2):
        with pytest.raises(sgn.SgnError, match="sgn_delay_enable") as e:
            c.delay_fold()
        assert e.value.rc == ESTATE
    with pytest.raises(sgn.SgnError) as e:
        c.trace_take()
    assert e.value.rc == ESTATE
    after = c.delay()
    assert after.info == before.info and after.rows.tobytes() == before.rows.tobytes()  # nothing changed
    c.delay_enable()
    d = sgn.run_delays(c, 300 * MS)
    assert_report(d, *expect(fan_in))
    c.snapshot_free(snap)


def test_short_cap_writes_nothing_and_clear_keeps_the_carry(ctxf, fan_in):
    c = traced_ctx(ctxf, fan_in["world"])
    submit_all([c], fan_in["dg"])
    c.run_until(S0 + 300 * MS)
    c.delay_fold()
    first = c.delay()
    rows = first.info["rows"]
    assert rows >= 1  # (the fan-in has one destination; test_short_cap_many_rows has a row per host)
    out = np.zeros(rows, sgn.DELAY_ROW_DTYPE)
    n64, info = C.c_uint64(), sgn.DelayInfo()
    rc = c.L.sgn_delay_get(c.h, out.ctypes.data_as(C.POINTER(sgn.DelayRow)), rows - 1, C.byref(n64), C.byref(info))
    assert rc == sgn.ERANGE and n64.value == rows and sgn.Delay(info).info == first.info
    assert not out.tobytes().strip(b"\0")
    assert c.delay(rows=False).info == first.info and len(c.delay(rows=False).rows) == 0
    # intervals: get + clear; the carry stays, so the two intervals add up to the whole run
    c.delay_clear()
    cleared = c.delay()
    assert cleared.info["folds"] == 0 and cleared.info["total"][:4] == [0, 0, 0, 0] and sum(cleared.info["hist_delivered"]) == 0
    assert cleared.info["total"][4] == first.info["total"][4] and np.array_equal(cleared.rows["standing"], first.rows["standing"][first.rows["standing"] > 0])
    second = sgn.run_delays(c, 300 * MS)
    _, whole = expect(fan_in)
    for k in range(4):
        assert first.info["total"][k] + second.info["total"][k] == whole["total"][k]
    assert (np.array(first.info["hist_delivered"]) + np.array(second.info["hist_delivered"])).tolist() == whole["hist_delivered"]
    assert (np.array(first.info["hist_dropped"]) + np.array(second.info["hist_dropped"])).tolist() == whole["hist_dropped"]
    assert max(first.info["delay_max"], second.info["delay_max"]) == whole["delay_max"] and second.info["total"][4] == 0
