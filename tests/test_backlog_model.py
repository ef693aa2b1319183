"""The backlog model (tests/backlog_model.py) on the oracle alone (CPU only): the scenarios that
tests/test_gpu_backlog.py compares sgn_backlog with are not trivial at the chosen edges — queues
past one CoDel page, held packets in both relays, send queues, packets in flight, a send ring that
wraps, hosts that fall idle after having had cold state — and the oracle's own identities hold (the
model asserts them while it runs: every POP follows a SEND, every DELIVER / CODEL_DROP a POP,
nothing below the window start is still in flight, at most one packet is held by relay_inet_out,
bytes and packets of the send queue vanish together)."""
import numpy as np
import pytest

import backlog_model as bm
import sgn
from external_common import datagrams, drive_ahead, external_world

ROUTER_HELD, OUT_HELD = sgn.BACKLOG_ROUTER_HELD, sgn.BACKLOG_OUT_HELD


def flag(x, bit):
    return (x.r["flags"] & np.uint64(bit)) != 0


def test_periodic_scenario_is_not_trivial(oracle):
    args = bm.periodic_world()
    o, xs = bm.expect_at(oracle, args, bm.PERIODIC_TARGETS)
    assert len(xs) == 10 and all(x.edge["win"][2] for x in xs)  # (every edge below the stop time)
    assert [x.edge["win"][0] for x in xs] == sorted(set(x.edge["win"][0] for x in xs))
    last = xs[-1]
    assert all(x.send_known for x in xs)                       # no push refused: the send queue is modelled
    assert (last.r["router_packets"] > 16).sum() >= 1          # more than one CoDel page
    assert flag(last, ROUTER_HELD).sum() >= 1 and flag(last, OUT_HELD).sum() >= 1
    assert (last.r["send_packets"] > 0).sum() >= 1 and (last.r["inflight_packets"] > 0).sum() >= 10
    # the early edges differ from the late ones: queues within a page, hosts without a router backlog
    assert xs[0].r["router_packets"].max() <= 16 and (xs[0].r["router_packets"] == 0).sum() > 100
    for x in xs:
        # PERIODIC payloads are all equal
        assert np.array_equal(x.r["router_bytes"], x.r["router_packets"] * np.uint64(1024 + 28))
        assert np.array_equal(x.r["send_bytes"], x.r["send_packets"] * np.uint64(1024 + 28))
        assert x.bytes_known.all()
        # a held packet's queue: the oldest queued packet arrived before the window start
        q = x.r["router_packets"] > 0
        assert np.all(x.r["router_oldest"][q] < x.ws) and np.all(x.r["router_oldest"][~q] == bm.INVALID)
        # the oracle's totals: what was sent and not popped is in flight
        st = x.edge["stats"]
        assert int(x.r["inflight_packets"].sum()) == st["packets_sent"] - st["packet_events_popped"]
        assert int(x.r["router_packets"].sum() + flag(x, ROUTER_HELD).sum()) == \
            st["packet_events_popped"] - st["delivered"] - st["codel_dropped"]
        mq, hq, ms, hs, ie = x.maxima()
        assert mq == x.r["router_packets"].max() and x.r["router_packets"][hq] == mq
        assert ie == x.r["inflight_earliest"].min() >= x.ws


def test_cold_scenario_has_hosts_that_fall_idle(oracle):
    o, xs = bm.expect_at(oracle, bm.cold_world(), bm.COLD_TARGETS)
    cold = [flag(x, ROUTER_HELD) | flag(x, OUT_HELD) | (x.r["router_packets"] > 0) | (x.r["send_packets"] > 0) for x in xs]
    had = np.zeros(200, dtype=bool)
    idle_after = 0    # (host, edge) pairs: cold state at an earlier edge, none now
    no_row_after = 0  # ... and not even a packet in flight: no row at all
    for x, c in zip(xs, cold):
        idle_after += int((had & ~c).sum())
        no_row_after += int((had & ~x.has_row()).sum())
        had |= c
    assert had.sum() >= 10 and idle_after >= 20 and no_row_after >= 1, (had.sum(), idle_after, no_row_after)


def test_tgen_scenario_is_not_trivial(oracle):
    o, xs = bm.expect_at(oracle, bm.tgen_world(), bm.TGEN_TARGETS, full=True)
    assert all(x.send_known for x in xs)
    last = xs[-1]
    assert last.r["router_packets"].max() > 100 and (last.r["router_packets"] > 16).sum() >= 10
    assert flag(last, ROUTER_HELD).sum() >= 10 and flag(last, OUT_HELD).sum() >= 1
    slow = np.arange(300)[7::37]
    assert flag(last, ROUTER_HELD)[slow].any()                 # a held packet on a slow client
    servers = np.arange(0, 300, 10)
    assert (last.r["send_packets"][servers] > 16).sum() >= 1   # trains in a server's send queue
    assert (last.r["inflight_packets"] > 0).sum() >= 10
    for x in xs:
        # router_bytes is modelled where every queued packet is delivered later: the hosts left out
        # are at most 10 % of the hosts with a router backlog
        q = x.r["router_packets"] > 0
        assert (q & ~x.bytes_known).sum() * 10 <= q.sum(), ((q & ~x.bytes_known).sum(), q.sum())
        st = x.edge["stats"]
        assert int(x.r["inflight_packets"].sum()) == st["packets_sent"] - st["packet_events_popped"]


def external_run(oracle, sims_extra=(), on_step=None):
    """The EXTERNAL scenario (fifo 8, slow uplinks) driven by drive_ahead on the oracle (and on
    sims_extra in lockstep): (world, datagrams, oracle, edges, drains of the oracle)."""
    world = external_world(fifo=8)
    dg = datagrams(world[2])
    o = bm.oracle_sim(oracle, world)
    edges = []

    def step(k):
        edges.append((k, bm.edge_of(o)))
        if on_step:
            on_step(k)

    drains, _ = drive_ahead([o] + list(sims_extra), dg, bm.EXT_STEP, on_step=step)
    return world, dg, o, edges, drains[0]


def test_external_scenario_wraps_the_send_ring(oracle):
    world, dg, o, edges, drains = external_run(oracle)
    m = bm.Model(o.trace(), world[2], world[3], world[4])
    xs = [m.at(e, bm.External(dg, bm.submitted_by(dg, k), drains)) for k, e in edges]
    assert len(xs) >= 10
    assert max(int(x.r["submit_pending"].sum()) for x in xs) > 0
    assert max(int(x.r["send_packets"].max()) for x in xs) == 8  # a full ring
    assert sum(int(flag(x, OUT_HELD).sum()) for x in xs) > 10 and sum(int(flag(x, ROUTER_HELD).sum()) for x in xs) > 10
    # the ring's head moves by one per IF_POP while the queue never runs empty: a host whose queue
    # stood at every edge so far and whose head + length passes the ring's 8 entries
    busy = np.ones(world[2].n, dtype=bool)
    wrapped = 0
    for x in xs:
        busy &= x.r["send_packets"] > 0
        wrapped += int((busy & (x.if_pops % 8 + x.r["send_packets"].astype(np.int64) > 8)).sum())
    assert wrapped >= 1
    assert not xs[-1].has_row().any() and not xs[-1].edge["win"][2]  # a finished run: nothing is left


def test_hot_slab_scenario_keeps_hundreds_in_flight(oracle):
    from test_gpu_pools import _hot_args
    args = _hot_args(1200)
    o = bm.oracle_sim(oracle, args)
    edges = []
    for _ in range(4):
        o.round()
        edges.append(bm.edge_of(o))
    m = bm.Model(o.trace(), args[2], args[3], args[4])
    xs = [m.at(e) for e in edges]
    # after the first round every client's request is in flight to one of the four servers
    assert int(xs[0].r["inflight_packets"].sum()) == 1196 and (xs[0].r["inflight_packets"] > 0).sum() == 4
    assert xs[0].r["inflight_packets"].max() > 256


@pytest.mark.parametrize("field", ["router_packets", "inflight_earliest", "flags"])
def test_backlog_dense(field):
    info = sgn.BacklogInfo()
    info.hosts, info.rows = 6, 2
    rows = np.zeros(2, sgn.BACKLOG_ROW_DTYPE)
    rows["host"] = [1, 4]
    rows["flags"] = [1, 3]
    rows["router_packets"] = [7, 0]
    rows["inflight_earliest"] = [sgn.EMUTIME_INVALID, 5]
    b = sgn.Backlog(info, rows)
    want = {"router_packets": [0, 7, 0, 0, 0, 0], "inflight_earliest": [0, 0, 0, 0, 5, 0], "flags": [0, 1, 0, 0, 3, 0]}[field]
    assert b.dense(field).tolist() == want and b.dense(field, 8).tolist() == want + [0, 0]
    assert b.info["hosts"] == 6 and len(b.info["total"]) == 8 and set(b.totals) == set(sgn.BACKLOG_TOTALS)
    assert len(sgn.Backlog(info).rows) == 0
