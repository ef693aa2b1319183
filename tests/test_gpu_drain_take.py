"""The ordered drain (-m gpu): sgn_drain_pending / sgn_drain_take / sgn_selftest_drain_order.

The ordering kernels alone run on records drawn here, through the self-test call, against
np.lexsort; the class limits (records a wave, and a workgroup, orders at once) are read from the
timing struct, so the shapes follow them. The simulations run beside the oracle, which calls
drain() where libsgn calls drain_take(): every field of every record is compared, and the spans
with the runs of `host` in the oracle's array. Expected values come from numpy or the oracle."""
import ctypes as C
import re

import numpy as np
import pytest

import sgn
from drain_take_cases import MS, S0, fan_in_case, segments_case, spans_of
from external_common import RUNAHEAD, advance_to, datagrams, external_world
from test_gpu_external import (assert_records, by_key, make_group, make_pair, run_group, shard_case,
                               shard_ranges, submit_to_owners, oracle_of)
from test_gpu_parity import assert_same_run, ctxf  # noqa: F401 (ctxf: fixture)

pytestmark = pytest.mark.gpu

EDEVICE, ESTATE = -5, -71
HOST_LO = 1000  # the self-test's host range starts here
FIELDS = ("status", "tag", "src_eid", "src_host", "time", "host")  # np.lexsort: the last key is the primary one


@pytest.fixture(scope="module")
def order_ctx():
    c = sgn.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def limits(order_ctx):
    t = order_ctx.drain_take_timing()
    assert t["wave_max"] == 64 and t["tile"] > t["wave_max"] and t["tile"] % 64 == 0, t
    return t["wave_max"], t["tile"]


def draw(rng, host):
    """One record per entry of `host`, every key unique (src_eid's low 32 bits are a permutation)
    while time, src_host, tag and status repeat often, in every half of their width."""
    n = len(host)
    r = np.zeros(n, sgn.DRAIN_DTYPE)
    r["host"] = host
    r["time"] = rng.integers(0, 3, n).astype(np.uint64) << np.uint64(32) | rng.integers(0, 3, n).astype(np.uint64)
    r["src_host"] = rng.choice(np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32), n)
    r["src_eid"] = rng.integers(0, 3, n).astype(np.uint64) << np.uint64(32) | rng.permutation(n).astype(np.uint64)
    r["tag"] = rng.choice(np.array([0, 5, 0x80000001], np.uint32), n)
    r["status"] = rng.integers(0, 6, n)
    r["dst_host"] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    r["payload_len"] = rng.integers(0, 1 << 16, n)
    r["handle"] = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    return r


def expected(recs):
    return recs[np.lexsort([recs[f] for f in FIELDS])]


def check_order(c, recs, n_hosts, host_lo=HOST_LO):
    exp = expected(recs)
    out, spans = sgn.selftest_drain_order(c, recs, host_lo, n_hosts)
    assert len(out) == len(exp)
    for f in sgn.DRAIN_DTYPE.names:
        bad = np.nonzero(out[f] != exp[f])[0]
        assert len(bad) == 0, (f, bad[:3], exp[bad[:3]], out[bad[:3]])
    assert out.tobytes() == exp.tobytes()
    host, first, count = spans_of(exp)
    assert np.array_equal(spans["host"], host) and np.array_equal(spans["first"], first)
    assert np.array_equal(spans["count"], count) and np.all(spans["reserved"] == 0)
    t = c.drain_take_timing()
    wave_max, tile = t["wave_max"], t["tile"]
    if len(recs):
        by = [int((count <= wave_max).sum()), int(((count > wave_max) & (count <= tile)).sum()), int((count > tile).sum())]
        assert t["spans_by_class"] == by and t["largest_span"] == count.max() and t["records"] == len(recs)
        assert t["hosts"] == len(host)
    return out, spans


ONE_HOST = ("2", "63", "64", "65", "T-1", "T", "T+1", "2T", "2T+1", "3T+5", "5T+3")


def size_of(label, tile):
    """'65' -> 65, 'T-1' -> tile - 1, '3T+5' -> 3 * tile + 5."""
    m = re.fullmatch(r"(?:(\d*)T)?([+-]?\d+)?", label)
    return (int(m.group(1) or 1) * tile if "T" in label else 0) + int(m.group(2) or 0)


@pytest.mark.parametrize("n", [0, 1])
def test_empty_and_single(order_ctx, n):
    check_order(order_ctx, draw(np.random.default_rng(n), np.full(n, HOST_LO + 2, np.uint32)), 4)


@pytest.mark.parametrize("label", ONE_HOST)
def test_one_host(order_ctx, limits, label):
    """Both class borders, and both parities of the merge pass count (2T: one pass, made two;
    2T+1 and 3T+5: two; 5T+3: three, made four)."""
    m = size_of(label, limits[1])
    check_order(order_ctx, draw(np.random.default_rng(m), np.full(m, HOST_LO + 1, np.uint32)), 3)


@pytest.mark.parametrize("n_hosts", [1, 63, 64, 65, 1025])
def test_many_small_hosts(order_ctx, n_hosts):
    """0 to 5 records a host, some hosts empty; 1025 hosts cross a tile of the scan."""
    rng = np.random.default_rng(n_hosts)
    per = rng.integers(0, 6, n_hosts)
    if n_hosts > 1:
        per[rng.integers(0, n_hosts, max(1, n_hosts // 8))] = 0
    host = (HOST_LO + np.repeat(np.arange(n_hosts), per)).astype(np.uint32)
    host = host[rng.permutation(len(host))]
    check_order(order_ctx, draw(rng, host), n_hosts)


def test_one_large_host_among_small_ones(order_ctx, limits):
    rng = np.random.default_rng(77)
    per = rng.integers(0, 6, 201)
    per[117] = 3 * limits[1]
    host = (HOST_LO + np.repeat(np.arange(201), per)).astype(np.uint32)
    host = host[rng.permutation(len(host))]
    _, spans = check_order(order_ctx, draw(rng, host), 201)
    assert order_ctx.drain_take_timing()["spans_by_class"][2] == 1


@pytest.mark.parametrize("reverse", [False, True], ids=["sorted", "reversed"])
def test_presorted_input(order_ctx, limits, reverse):
    rng = np.random.default_rng(5)
    per = np.array([3, 64, 65, limits[1], 2 * limits[1] + 9, 0, 1])
    host = (HOST_LO + np.repeat(np.arange(len(per)), per)).astype(np.uint32)
    recs = expected(draw(rng, host))
    check_order(order_ctx, recs[::-1].copy() if reverse else recs, len(per))


def tie_case(rng, field, m):
    """m records of one host whose keys differ in `field` alone (later fields are drawn freely:
    they must not matter), in a random order."""
    r = np.zeros(m, sgn.DRAIN_DTYPE)
    r["host"] = HOST_LO + 3
    r["time"], r["src_host"], r["src_eid"], r["tag"], r["status"] = 0x0000000700000009, 11, 0x0000000500000006, 13, 2
    p = rng.permutation(m).astype(np.uint64)
    hi, lo = np.uint64(32), np.uint64(0xFFFFFFFF)
    order = ["time", "src_host", "src_eid", "tag", "status"]
    if field == "time_hi":
        r["time"], field = p << hi | np.uint64(9), "time"
    elif field == "time_lo":
        r["time"], field = np.uint64(7) << hi | p, "time"
    elif field == "src_host":
        r["src_host"] = (p * np.uint64(0xFFFFFFFF // m)).astype(np.uint32)  # (over the whole 32 bits)
    elif field == "src_eid_hi":
        r["src_eid"], field = p << hi | np.uint64(6), "src_eid"
    elif field == "src_eid_lo":
        r["src_eid"], field = np.uint64(5) << hi | p, "src_eid"
    elif field == "src_eid":
        r["src_eid"] = rng.permutation(m).astype(np.uint64) * np.uint64((1 << 64) // m - 1) & ~lo | p
    elif field == "tag":
        r["tag"] = (p * np.uint64(0xFFFFFFFF // m)).astype(np.uint32)
    elif field == "status":
        r["status"] = (p * np.uint64(0xFFFFFFFF // m)).astype(np.uint32)
    for f in order[order.index(field) + 1:]:  # what comes after the deciding field: anything
        r[f] = rng.integers(0, 1 << 32, m, dtype=np.uint64).astype(r[f].dtype)
    r["handle"] = np.arange(m)
    assert len(np.unique(r[field])) == m
    return r


@pytest.mark.parametrize("size", ["40", "300", "2T+7"])
@pytest.mark.parametrize("field", ["time_hi", "time_lo", "src_host", "src_eid", "src_eid_hi", "src_eid_lo", "tag", "status"])
def test_one_field_decides(order_ctx, limits, field, size):
    """Every field of the key decides alone, in each of the three ordering kernels (a wave, a
    workgroup, tiles and merges), and the 64-bit fields in each of their halves."""
    m = size_of(size, limits[1])
    check_order(order_ctx, tie_case(np.random.default_rng(m), field, m), 8)


def test_equal_keys_come_out_as_a_permutation(order_ctx, limits):
    rng = np.random.default_rng(9)
    per = np.array([50, 500, 2 * limits[1] + 100])
    host = (HOST_LO + np.repeat(np.arange(3), per)).astype(np.uint32)
    recs = draw(rng, host)
    recs["src_eid"] = rng.integers(0, 4, len(recs))  # many equal keys
    recs["handle"] = np.arange(len(recs))
    recs = recs[rng.permutation(len(recs))]
    out, _ = sgn.selftest_drain_order(order_ctx, recs, HOST_LO, 3)
    exp = expected(recs)
    for f in FIELDS:
        assert np.array_equal(out[f], exp[f]), f
    assert np.array_equal(np.sort(out["handle"]), np.arange(len(recs)))
    assert out[np.argsort(out["handle"])].tobytes() == recs[np.argsort(recs["handle"])].tobytes()


@pytest.mark.parametrize("where", ["below", "above"])
def test_record_outside_the_host_range(order_ctx, where):
    rng = np.random.default_rng(4)
    host = (HOST_LO + rng.integers(0, 10, 500)).astype(np.uint32)
    host[321] = HOST_LO - 1 if where == "below" else HOST_LO + 10
    with pytest.raises(sgn.SgnError, match=str(int(host[321]))) as e:
        sgn.selftest_drain_order(order_ctx, draw(rng, host), HOST_LO, 10)
    assert e.value.rc == EDEVICE
    assert not e.value.out.tobytes().strip(b"\0")  # untouched
    check_order(order_ctx, draw(rng, np.full(70, HOST_LO, np.uint32)), 10)  # the context still works


def test_selftest_span_capacity(order_ctx):
    rng = np.random.default_rng(6)
    host = (HOST_LO + np.repeat(np.arange(5), 3)).astype(np.uint32)
    with pytest.raises(sgn.SgnError) as e:
        sgn.selftest_drain_order(order_ctx, draw(rng, host), HOST_LO, 5, span_cap=4)
    assert e.value.rc == sgn.ERANGE and e.value.needed == 5


# ---- simulations, beside the oracle ----
def check_take(o, c, expect=()):
    """One pause: the oracle drains, libsgn takes; returns the records."""
    exp = o.drain()
    assert c.drain_pending() == len(exp)
    recs, spans = c.drain_take()
    assert_records(exp, recs, expect)
    assert recs.tobytes() == exp.tobytes()
    host, first, count = spans_of(exp)
    assert np.array_equal(spans["host"], host) and np.array_equal(spans["first"], first)
    assert np.array_equal(spans["count"], count)
    assert int(count.sum()) == len(recs)  # the spans tile the records
    assert c.drain_pending() == 0
    assert len(c.drain()) == 0  # nothing left on the device, nothing held
    return recs


def test_lockstep_with_the_oracle(ctxf, oracle):
    """external_common.drive's loop with a pause every 3 rounds and at the end."""
    world = external_world()
    src, dip, pay, t, handle, wire = datagrams(world[2])
    o, c = make_pair(ctxf, oracle, world)
    sims = (o, c)
    nxt = rounds = takes = 0
    got = []
    while rounds < 100_000:
        assert o.window() == c.window()
        ws, we, active = o.window()
        if nxt < len(t) and (not active or int(t[nxt]) < ws):
            ws = int(t[nxt])
            for s in sims:
                s.set_window(ws, ws + RUNAHEAD)
            we = o.window()[1]
        elif not active:
            break
        j = nxt
        while j < len(t) and int(t[j]) < we:
            j += 1
        if j > nxt:
            for s in sims:
                s.submit(src[nxt:j], dip[nxt:j], pay[nxt:j], t[nxt:j], handle[nxt:j], wire_len=wire[nxt:j])
            nxt = j
        assert o.round() == c.round()
        rounds += 1
        if rounds % 7 == 0:
            assert o.rng_next_u64(1) == c.rng_next_u64(1)
        if rounds % 3 == 0:
            got.append(check_take(o, c))
            takes += 1
    got.append(check_take(o, c))
    got = np.concatenate(got)
    assert len(got) == len(t) and takes > 10
    st = np.bincount(got["status"], minlength=6)
    assert all(st[s] > 0 for s in (sgn.DRAIN_DELIVERED, sgn.DRAIN_LOCAL, sgn.DRAIN_LOSS, sgn.DRAIN_UNKNOWN)), st
    assert_same_run(o, c, world[2].n, trace=False)


def submit_all(sims, dg):
    for s in sims:
        s.submit(dg[0], dg[1], dg[2], dg[3], dg[4], wire_len=dg[5])


def test_exact_segments_from_a_simulation(ctxf, oracle, limits):
    world, dg, counts = segments_case(limits[1])
    o, c = make_pair(ctxf, oracle, world)
    submit_all((o, c), dg)
    assert o.run() == c.run()
    recs = check_take(o, c, (sgn.DRAIN_UNKNOWN,))
    host, _, count = spans_of(recs)
    assert dict(zip(host.tolist(), count.tolist())) == counts
    assert c.drain_take_timing()["spans_by_class"] == [4, 1, 1]


def test_fan_in_to_a_slow_host(ctxf, oracle, limits):
    world, dg, dst = fan_in_case(limits[1])
    o, c = make_pair(ctxf, oracle, world)
    info = c.engine_info()
    assert int(dg[3][-1]) < S0 + (info["calendar_buckets"] - 2) * info["bucket_width_ns"]
    submit_all((o, c), dg)
    assert o.run() == c.run() > 100
    recs = check_take(o, c, (sgn.DRAIN_DELIVERED, sgn.DRAIN_CODEL))
    at = recs[recs["host"] == dst]
    assert len(at) >= limits[1] + 100 and set(at["status"].tolist()) == {sgn.DRAIN_DELIVERED, sgn.DRAIN_CODEL}
    assert c.drain_take_timing()["spans_by_class"][2] == 1
    assert_same_run(o, c, world[2].n, trace=False)


def paused_pair(ctxf, oracle, t_ms=40):
    """The default world with every datagram submitted ahead, run to S0 + t_ms: records are pending."""
    world = external_world()
    dg = datagrams(world[2], span_ns=100 * MS)
    o, c = make_pair(ctxf, oracle, world)
    info = c.engine_info()
    assert int(dg[3][-1]) < S0 + (info["calendar_buckets"] - 2) * info["bucket_width_ns"]
    submit_all((o, c), dg)
    assert advance_to(o, S0 + t_ms * MS) == advance_to(c, S0 + t_ms * MS) > 10
    return world, o, c


def raw_take(c, cap, span_cap):
    recs = np.zeros(max(cap, 1), sgn.DRAIN_DTYPE)
    spans = np.zeros(max(span_cap, 1), sgn.SPAN_DTYPE)
    n, ns = C.c_uint64(), C.c_uint64()
    rc = c.L.sgn_drain_take(c.h, recs.ctypes.data_as(C.POINTER(sgn.DrainRec)), cap, C.byref(n),
                            spans.ctypes.data_as(C.POINTER(sgn.TraceSpan)), span_cap, C.byref(ns))
    return rc, n.value, ns.value, recs, spans


def test_capacity_rule(ctxf, oracle):
    _, o, c = paused_pair(ctxf, oracle)
    n = c.drain_pending()
    exp = o.drain()
    n_hosts = len(np.unique(exp["host"]))
    assert n == len(exp) > 50 and n_hosts > 5
    for cap, span_cap in ((n - 1, n_hosts), (n, n_hosts - 1), (0, 0)):
        rc, need, need_spans, recs, spans = raw_take(c, cap, span_cap)
        assert (rc, need, need_spans) == (sgn.ERANGE, n, n_hosts)
        assert not recs.tobytes().strip(b"\0") and not spans.tobytes().strip(b"\0")
        assert c.drain_pending() == n
    with pytest.raises(sgn.SgnError) as e:
        c.drain_take(cap=n - 1)
    assert e.value.rc == sgn.ERANGE and e.value.needed == (n, n_hosts)
    recs, spans = c.drain_take(cap=n + 3, span_cap=0)  # no spans asked for
    assert len(spans) == 0 and recs.tobytes() == exp.tobytes()
    assert c.drain_pending() == 0
    recs, spans = c.drain_take()  # nothing pending: OK, both empty
    assert len(recs) == 0 and len(spans) == 0
    assert o.run() == c.run()
    assert c.drain_take()[0].tobytes() == o.drain().tobytes()
    assert_same_run(o, c, 60, trace=False)


def test_held_records_are_part_of_the_take(ctxf, oracle):
    """drain(0, 30, cap=5) copies everything to the host and leaves all but five records held; more
    rounds then put new records on the device: the take reads both."""
    _, o, c = paused_pair(ctxf, oracle, 30)
    before = c.drain_pending()
    five = c.drain(0, 30, cap=5)
    assert len(five) == 5 and c.drain_pending() == before - 5 > 20
    assert advance_to(o, S0 + 60 * MS) == advance_to(c, S0 + 60 * MS) > 10
    assert c.drain_pending() > before  # held records and new ones on the device
    take, spans = c.drain_take()
    exp = o.drain()
    both = by_key(np.concatenate([five, take]))
    assert both.tobytes() == by_key(exp).tobytes() == exp.tobytes()
    assert take.tobytes() == by_key(take).tobytes()  # ordered by itself
    tail = exp[exp["host"] < 30][5:]
    assert len(tail) > 0  # the held tail of the short drain is in the take
    keys = set(zip(take["host"].tolist(), take["time"].tolist(), take["src_host"].tolist(), take["src_eid"].tolist(),
                   take["tag"].tolist()))
    assert all(k in keys for k in zip(tail["host"].tolist(), tail["time"].tolist(), tail["src_host"].tolist(),
                                      tail["src_eid"].tolist(), tail["tag"].tolist()))
    host, first, count = spans_of(take)
    assert np.array_equal(spans["host"], host) and np.array_equal(spans["count"], count)
    assert c.drain_pending() == 0 and len(c.drain()) == 0


def test_snapshot_brings_pending_records_back(ctxf, oracle):
    world, o, c = paused_pair(ctxf, oracle)
    held = c.drain(0, 10, cap=2)  # (the caller's from here on; a tail stays held in the snapshot)
    assert len(held) == 2
    assert advance_to(o, S0 + 50 * MS) == advance_to(c, S0 + 50 * MS) > 5  # (held records, and new ones on the device)
    exp = o.drain()
    snap = c.snapshot_save()
    n = c.drain_pending()
    a, sa = c.drain_take()
    assert len(a) == n == len(exp) - 2 and c.drain_pending() == 0
    c.snapshot_restore(snap)
    assert c.drain_pending() == n
    b, sb = c.drain_take()
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()
    assert by_key(np.concatenate([held, b])).tobytes() == exp.tobytes()
    c.snapshot_free(snap)
    assert o.run() == c.run() > 10
    assert c.drain_take()[0].tobytes() == o.drain().tobytes()
    assert_same_run(o, c, world[2].n, trace=False)  # (the oracle only ever called drain())


def test_two_shards_take_their_own_records(oracle):
    """A local group of two: each context takes the records of the hosts it owns. In rank order they
    are the unsharded run's records (the oracle's drain()) in every field, with the two differences
    sgn.h documents for shards: the slot bits of `tag` count the submitting shard's own submissions,
    and `handle` is the submitted one only where the taking shard owns the source. Both are
    asserted exactly: the expected slot is the datagram's rank among its shard's submissions."""
    case = shard_case(oracle)
    dg, n = case["dg"], case["world"][2].n
    shards, arr = make_group(case["world"], 2)
    ranges = shard_ranges(shards[0], n, 2)
    submit_to_owners(shards, ranges, dg, np.ones(len(dg[3]), bool))
    o = oracle_of(oracle, case)
    o.submit(dg[0], dg[1], dg[2], dg[3], dg[4], wire_len=dg[5])
    assert run_group(shards, arr) == o.run() > 100
    exp = o.drain()
    parts = []
    for c, (lo, hi) in zip(shards, ranges):
        p = c.drain_pending()
        recs, spans = c.drain_take()
        assert len(recs) == p > 0 and np.all((recs["host"] >= lo) & (recs["host"] < hi))
        host, first, count = spans_of(recs)
        assert np.array_equal(spans["host"], host) and np.array_equal(spans["first"], first)
        assert np.array_equal(spans["count"], count)
        assert c.drain_pending() == 0 and len(c.drain()) == 0
        parts.append(recs)
    got = np.concatenate(parts)
    assert len(got) == len(exp) == len(dg[3])
    for f in ("time", "src_eid", "host", "src_host", "dst_host", "status", "payload_len"):
        assert np.array_equal(got[f], exp[f]), f
    slot_mask = np.uint32(0x1FFFFFFF)  # SGN_TAG_SLOT_MASK
    owner = lambda h: np.searchsorted([hi for _, hi in ranges], h, side="right")  # noqa: E731
    dg_owner = owner(dg[0])
    rank_in_shard = np.zeros(len(dg[0]), np.uint32)
    for r in range(2):
        rank_in_shard[dg_owner == r] = np.arange((dg_owner == r).sum())
    oslot = exp["tag"] & slot_mask  # the oracle's slot: the datagram's index
    assert np.array_equal(got["tag"], (exp["tag"] & ~slot_mask) | rank_in_shard[oslot])
    same = owner(got["src_host"]) == owner(got["host"])
    assert np.array_equal(got["handle"], np.where(same, exp["handle"], 0))
    assert same.any() and (~same).any() and np.all(exp["handle"] != 0)


def test_state_errors(ctxf):
    c = ctxf()
    rc, n, ns, _, _ = raw_take(c, 4, 4)
    assert (rc, n, ns) == (ESTATE, 0, 0)
    n64 = C.c_uint64(5)
    assert c.L.sgn_drain_pending(c.h, C.byref(n64)) == ESTATE and n64.value == 0
    g = sgn.random_graph(8, seed=3)
    hosts = sgn.HostArrays(sgn.assign_ips(16), np.arange(16) % 8, np.full(16, 10_000_000), np.full(16, 10_000_000),
                           sgn.derive_seeds(1, sgn.host_names(16)))
    c.routes_build(g, np.arange(8))
    c.hosts_set(hosts)
    assert raw_take(c, 4, 4)[0] == ESTATE  # hosts, but no simulation yet
    c.sim_init(sgn.make_config(50 * MS, event_capacity=1 << 16), sgn.make_traffic(period_ns=2 * MS))
    rc, n, ns, _, _ = raw_take(c, 4, 4)
    assert (rc, n, ns) == (ESTATE, 0, 0) and "EXTERNAL" in c.L.sgn_last_error(c.h).decode()
    with pytest.raises(sgn.SgnError) as e:
        c.drain_take()
    assert e.value.rc == ESTATE
    c.run(5)  # the simulation is untouched
