"""The TGEN round kernel's lane table against the oracle (-m gpu).

k_rounds<TGEN, *> reads DevSim from the lanes of four vector registers that it fills once per
launch (csrc/sgn_internal.h; tests/test_ktab.py checks the index arithmetic on the CPU). The
table is only as fresh as the launch: every host-side change of DevSim — a grown CoDel pool
with its new cq_pages / div_cq, a re-laid calendar, a restored snapshot — has to be seen by the
next launch. 200 TGEN hosts on a 16-node graph (four host groups of 64, the last with 8 valid
lanes), persistent launches of 25 rounds, every case bit for bit against the oracle on the
counters, the window and every host's digests, and every case checks that its trigger happened.
The oracle of the shared scenario runs once per module and is never stepped again.
"""
import numpy as np
import pytest

import sgn
from test_gpu_parity import assert_same_run, ctxf, scenario  # noqa: F401 (ctxf: fixture)
from test_gpu_pools import _pages_ok
from test_gpu_snapshot import assert_state, make_ctx, state

pytestmark = pytest.mark.gpu

N, V, LAUNCH = 200, 16, 25
R_UNTIL, R_SNAP, R_PLAIN = 37, 50, 300  # round edges of the shared scenario the cases stop at


def _base_args():
    return scenario(n=N, V=V, kind=sgn.TRAFFIC_TGEN, stop_ns=1_000_000_000, tor=True, tgen_think=20_000_000)


_REF = {}


def base_ref(oracle):
    """The oracle's one run of the shared scenario: its state at the round edges the cases stop
    at, then the run to the end."""
    if "base" not in _REF:
        args = _base_args()
        g, used, hosts, cfg, tr = args
        lat, loss = oracle.routes(g, used)
        o = oracle.Sim(used, lat, loss, hosts, cfg, tr)
        marks, rounds = {}, 0
        while o.window()[2]:
            o.round()
            rounds += 1
            if rounds in (R_UNTIL, R_SNAP, R_PLAIN):
                marks[rounds] = state(o, N)
        assert rounds > R_PLAIN + LAUNCH and len(marks) == 3, rounds
        _REF["base"] = (args, o, marks, rounds)
    return _REF["base"]


def _run_in_launches(c, limit=1 << 30):
    """Persistent launches of LAUNCH rounds until the simulation ends (or `limit` rounds)."""
    done = 0
    while c.window()[2] and done < limit:
        k = c.run(min(LAUNCH, limit - done))
        assert k > 0
        done += k
    return done


def _shape_ok(info):
    assert info["persistent_grid"] > 0 and info["persistent_fallbacks"] == 0, info
    assert info["hosts_per_wave"] == 64 and info["host_groups"] == 4, info  # 64 + 64 + 64 + 8 hosts


def test_plain_run(ctxf, oracle):
    args, o, marks, rounds = base_ref(oracle)
    c = make_ctx(ctxf, args)
    assert _run_in_launches(c, R_PLAIN) == R_PLAIN
    _shape_ok(c.engine_info())
    assert_state(state(c, N), marks[R_PLAIN], "after 300 rounds")
    assert marks[R_PLAIN][1]["packets_sent"] > 1000
    assert _run_in_launches(c) == rounds - R_PLAIN
    assert_same_run(o, c, N, trace=False)


def test_codel_pool_grows_between_launches(ctxf, oracle):
    # slow down-links make CoDel queues stand; the pool starts at one page per host plus 64, so a
    # round edge holds and the host grows it: the next launch must read the new cq_pages / div_cq
    bw = np.where(np.arange(N) % 10 == 0, 100_000_000, 4_000_000).astype(np.uint64)
    args = scenario(n=N, V=V, kind=sgn.TRAFFIC_TGEN, stop_ns=1_000_000_000, bw=bw, tor=True,
                    tgen_think=200_000_000, codel=1)
    g, used, hosts, cfg, tr = args
    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr)
    o.run()
    c = make_ctx(ctxf, args)
    i0 = c.engine_info()
    _run_in_launches(c)
    info, st = c.engine_info(), c.stats()
    _shape_ok(info)
    assert info["codel_pool_grows"] >= 1 and info["codel_pages"] > i0["codel_pages"], info
    assert info["codel_page_allocs"] > i0["codel_pages"], info  # (the free ring wrapped: div_cq in use)
    assert st["codel_dropped"] > 0, st
    _pages_ok(info)
    assert_same_run(o, c, N, trace=False)


def _hot_args():
    """test_gpu_pools' hot-slab fan-in at this file's size: every client fetches a one-packet file
    from one of four servers (HostIds 0-3: host group 0) at the same instant. The hosts sit on two
    of the graph's 16 nodes, so the ~196 requests share four latencies and land in a few 1-ms
    buckets: ~50 to ~100 runs for one (bucket, group) slab of 16."""
    g = sgn.tor_graph(V, seed=3)
    bw = np.full(N, 1_000_000_000, np.uint64)
    hosts = sgn.HostArrays(sgn.assign_ips(N), np.arange(N) % 2, bw, bw, sgn.derive_seeds(1, sgn.host_names(N)))
    cfg = sgn.make_config(600_000_000, event_capacity=1 << 20, codel_cap=64)
    tr = sgn.make_traffic(sgn.TRAFFIC_TGEN, period_ns=100_000_000, period_jitter_ns=100_000_000, start_jitter_ns=0,
                          servers=np.arange(4), file_bytes=(1000, 1400, 1400))
    return g, np.arange(V), hosts, cfg, tr


def test_small_calendar_runs_the_big_slab_kernel(ctxf, oracle, monkeypatch):
    # 16-run slabs that may grow to 32 (test hooks): the servers' slabs spill, the calendar is
    # re-laid out with extensions, and the launches after that are the kBig instantiation
    monkeypatch.setenv("SGN_SLAB_CAP", "16")
    monkeypatch.setenv("SGN_SLAB_LIM", "32")
    args = _hot_args()
    g, used, hosts, cfg, tr = args
    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr)
    o.run()
    c = make_ctx(ctxf, args)
    _run_in_launches(c)
    info = c.engine_info()
    print({k: info[k] for k in ("slab_extensions", "calendar_grows", "big_slab_pieces", "slab_capacity",
                                "calendar_spill_runs", "rounds_held")})
    _shape_ok(info)
    assert info["slab_extensions"] >= 1 and info["big_slab_pieces"] > 0, info  # (launches of the kBig kernel)
    assert c.stats()["packets_sent"] > 1000
    assert_same_run(o, c, N, trace=False)


def test_snapshot_restore_at_a_round_edge(ctxf, oracle):
    args, o, marks, rounds = base_ref(oracle)
    c = make_ctx(ctxf, args)
    assert _run_in_launches(c, R_SNAP) == R_SNAP
    at = state(c, N)
    assert_state(at, marks[R_SNAP], "at the save")
    snap = c.snapshot_save()
    assert c.snapshot_info(snap)["rounds"] == R_SNAP
    assert _run_in_launches(c) == rounds - R_SNAP
    assert_same_run(o, c, N, trace=False)
    c.snapshot_restore(snap)
    assert_state(state(c, N), at, "after restore")
    assert _run_in_launches(c) == rounds - R_SNAP
    _shape_ok(c.engine_info())
    assert_same_run(o, c, N, trace=False)
    c.snapshot_free(snap)


def test_run_until_a_time_inside_a_launch(ctxf, oracle):
    args, o, marks, rounds = base_ref(oracle)
    c = make_ctx(ctxf, args)
    ws = marks[R_UNTIL][0][0]  # the window start after 37 rounds: the launch pauses at its 37th edge
    assert R_UNTIL % LAUNCH != 0
    assert c.run_until(ws) == R_UNTIL
    assert_state(state(c, N), marks[R_UNTIL], "paused")
    assert c.run_until(ws) == 0
    _shape_ok(c.engine_info())
    assert _run_in_launches(c) == rounds - R_UNTIL
    assert_same_run(o, c, N, trace=False)
