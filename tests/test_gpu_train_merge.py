"""A blocked train's cached packet goes out with its head run (engine.hip forward_out_step).

A TGEN server in mid-file ends a round blocked on its token bucket, the refused packet cached
(Relay::next_packet). At the next refill the TGEN round kernels send the cached packet and
the head run of the same train in ONE step: one removal from the bucket, one send_batch (the
same loss draws in the same order), one event run at the client instead of two. Results must
not move: every case runs 2-4 hosts on a 2-node graph through ctx.run (the persistent kernel)
to the end of the transfers and is compared with the oracle bit for bit (counters, window,
per-host digests; the traced case record for record). File sizes are no multiple of the MSS.

Run counts (cases 1-4). From the oracle's POP trace alone: G = the maximal groups of POP
records of one (host, time, source) with consecutive event ids, T = the trains completed.
The merged form files G runs, plus at most one per train for its short last packet, which stays
a step of its own: G <= event_runs <= G + T. The two-step form would file one more run for
every instant at which a cached packet and packets of the run behind it go out together (M);
the cases' premises, checked on the CPU, make M large against T wherever the bucket lets more
than one packet pass per refill, so the bound tells the two forms apart:
 - R, the mid-train rounds (a refill instant that begins with a full-size packet cached), is at
   least G / 2 in every case;
 - M is at least G / 2 with a 100 Mbit or 1 Gbit server; a 10 Mbit server's refill is less than
   one packet, so its merged take is refused whole or passes the cached packet only (M = 0,
   and both happen).
"""
import numpy as np
import pytest

import sgn

pytestmark = pytest.mark.gpu

MSS = 1472
SKIP_STATS = ("max_pending_events", "sched_heavy_hosts", "sched_sorted_segments", "event_runs")
DIGEST_FIELDS = ("tx", "rx", "app", "rng", "next_event_id", "n_sent", "n_popped", "n_delivered",
                 "n_codel_dropped")
TRACE_FIELDS = ("kind", "host", "peer", "flags", "a", "b", "c", "seq", "rng_pos")


def world(server_bw, file_bytes, *, clients=1, loss=0.0, qdisc=0, stop_ms=400, jitter_ns=0):
    """Host 0 the server (node 0), hosts 1.. the clients (node 1, 1 Gbit), one fetch each: the
    think time is longer than the run."""
    assert file_bytes % MSS != 0
    g = sgn.GraphArrays([0, 1], [0, 1, 0], [0, 1, 1], [1_000_000, 1_000_000, 5_000_000],
                        np.array([0.0, 0.0, loss], np.float32), False)
    n = 1 + clients
    bw = np.array([server_bw] + [1_000_000_000] * clients, dtype=np.uint64)
    hosts = sgn.HostArrays(sgn.assign_ips(n), [0] + [1] * clients, bw, bw, sgn.derive_seeds(1, sgn.host_names(n)))
    cfg = sgn.make_config(stop_ms * 1_000_000, out_fifo_cap=64, codel_cap=4096, event_capacity=1 << 16, qdisc=qdisc)
    tr = sgn.make_traffic(sgn.TRAFFIC_TGEN, start_ns=2_000_000, start_jitter_ns=jitter_ns,
                          period_ns=3600 * 1_000_000_000, period_jitter_ns=0, servers=[0],
                          file_bytes=(file_bytes,) * 3)
    return g, [0, 1], hosts, cfg, tr


# name -> world arguments
CASES = {
    "plain_100M": dict(server_bw=100_000_000, file_bytes=199 * MSS + 972),
    "1G_loss_0.3pct": dict(server_bw=1_000_000_000, file_bytes=2500 * MSS + 700, loss=0.003),
    "1G_loss_25pct": dict(server_bw=1_000_000_000, file_bytes=2500 * MSS + 700, loss=0.25),
    "10M": dict(server_bw=10_000_000, file_bytes=40 * MSS + 972, stop_ms=200),
    "round_robin_two_clients": dict(server_bw=100_000_000, file_bytes=60 * MSS + 972, clients=2,
                                    qdisc=sgn.QDISC_ROUND_ROBIN),
    "cached_last_then_other_train": dict(server_bw=100_000_000, file_bytes=34 * MSS + 972, clients=2),
}

_refs = {}


@pytest.fixture(scope="module")
def ref(oracle):
    """The oracle's run of a case (traced), made once and shared; never changed."""
    def get(name):
        if name not in _refs:
            args = world(**CASES[name])
            g, used, hosts, cfg, tr = args
            lat, loss = oracle.routes(g, used)
            o = oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=True)
            o.run()
            t = o.trace()
            t = t[np.lexsort((t["seq"], t["host"]))]
            t.setflags(write=False)
            _refs[name] = (args, o.stats(), o.window(), o.digests(0, hosts.n), t)
        return _refs[name]
    return get


def gpu_run(args, trace=False):
    g, used, hosts, cfg, tr = args
    c = sgn.Context()
    c.routes_build(g, used)
    c.hosts_set(hosts)
    if trace:
        c.trace_enable(1 << 20)
    c.sim_init(cfg, tr)
    c.run()
    return c


def assert_same(r, c, trace=False):
    args, so, wo, do, to = r
    sg = c.stats()
    for k in so:
        if k not in SKIP_STATS:
            assert so[k] == sg[k], (k, so[k], sg[k])
    assert wo == c.window()
    dg = c.digests(0, args[2].n)
    for f in DIGEST_FIELDS:
        assert np.array_equal(do[f], dg[f]), f
    if trace:
        tg = c.trace()
        tg = tg[np.lexsort((tg["seq"], tg["host"]))]
        assert len(to) == len(tg)
        for f in TRACE_FIELDS:
            bad = np.nonzero(to[f] != tg[f])[0]
            assert len(bad) == 0, (f, to[bad[:3]], tg[bad[:3]])


def pop_groups(t):
    """G: maximal groups of the POP trace by (host, time, source) with consecutive event ids."""
    p = t[t["kind"] == sgn.TRACE_POP]  # (sorted by host, then seq)
    if not len(p):
        return 0
    same = ((p["host"][1:] == p["host"][:-1]) & (p["a"][1:] == p["a"][:-1]) &
            (p["peer"][1:] == p["peer"][:-1]) & (p["c"][1:] == p["c"][:-1] + 1))
    return int(1 + np.count_nonzero(~same))


def server_sends(t, server=0):
    """The server's packets in the order it popped them from its interface: (pop time, send
    time, peer, payload, outcome). send_packet follows the pops in order, so the k-th SEND record
    is the k-th IF_POP's."""
    h = t[t["host"] == server]
    pops = h[h["kind"] == sgn.TRACE_IF_POP]
    sends = h[h["kind"] == sgn.TRACE_SEND]
    assert len(pops) == len(sends) and len(pops) > 0
    assert np.array_equal(pops["peer"], sends["peer"])
    return pops["a"], sends["a"], sends["peer"], (pops["b"] & 0xFFFFFFFF).astype(np.int64), sends["flags"]


def merge_counts(t, last_payload):
    """T (trains completed), R (mid-train rounds: a full-size packet sent at a later instant than
    it was popped, i.e. from the cache), M (of those, the ones whose instant also sends the next
    packet of the same train: the two-step form's extra runs), Z (refill instants that pass the
    cached packet only) from the oracle's trace."""
    tp, ts, peer, pay, _ = server_sends(t)
    T = int(np.count_nonzero(pay == last_payload))
    cached = (ts > tp) & (pay == MSS)
    nxt = np.zeros(len(ts), bool)
    nxt[:-1] = (ts[1:] == ts[:-1]) & (peer[1:] == peer[:-1]) & (pay[1:] == MSS)
    return T, int(np.count_nonzero(cached)), int(np.count_nonzero(cached & nxt)), \
        int(np.count_nonzero(cached & ~nxt))


@pytest.mark.parametrize("name", ["plain_100M", "1G_loss_0.3pct", "1G_loss_25pct", "10M"])
def test_merged_runs_match_oracle(ref, name):
    r = ref(name)
    args, so, _, _, t = r
    kw = CASES[name]
    last = kw["file_bytes"] % MSS
    n_pkt = kw["file_bytes"] // MSS + 1
    # premises, from the oracle alone
    assert so["packets_sent"] + so["packets_loss_dropped"] == 1 + n_pkt  # the request, the whole train
    G = pop_groups(t)
    T, R, M, Z = merge_counts(t, last)
    print(name, "G", G, "T", T, "mid-train rounds", R, "two-record instants", M, "cached alone", Z)
    assert T == 1
    assert R >= G // 2 and R >= 10, (G, R)
    if kw["server_bw"] > 10_000_000:
        assert M >= G // 2 and M >= 10, (G, M)
    else:
        # less than a packet per refill: never two at one instant, and some refills pass none
        assert M == 0 and Z >= 10, (M, Z)
        _, ts, _, _, _ = server_sends(t)
        assert np.diff(ts).max() >= 2_000_000
    if kw.get("loss"):
        lost = so["packets_loss_dropped"]
        assert lost >= (3 if kw["loss"] < 0.1 else 200), lost
    c = gpu_run(args)
    assert_same(r, c)
    runs = c.stats()["event_runs"]
    print(name, "event_runs", runs)
    assert G <= runs <= G + T, (G, runs, T)
    c.close()


def test_round_robin_does_not_merge(ref):
    """Two clients' trains queued under the round-robin qdisc: one packet per socket in turn, so a
    cached packet's successor in the queue is the other client's."""
    r = ref("round_robin_two_clients")
    _, _, _, _, t = r
    tp, ts, peer, pay, _ = server_sends(t)
    alt = (ts[1:] == ts[:-1]) & (peer[1:] != peer[:-1])
    cached = ts > tp
    assert np.count_nonzero(alt) >= 40 and np.count_nonzero(cached) >= 10
    # a cached packet followed at its instant by the other socket's packet
    assert np.count_nonzero(cached[:-1] & alt) >= 5
    c = gpu_run(r[0])
    assert_same(r, c)
    c.close()


def test_cached_last_packet_then_other_train(ref):
    """FIFO qdisc, two clients: the first train's short last packet is the one the bucket
    refuses, and the head of the queue behind it is the other client's train."""
    r = ref("cached_last_then_other_train")
    _, _, _, _, t = r
    last = CASES["cached_last_then_other_train"]["file_bytes"] % MSS
    tp, ts, peer, pay, _ = server_sends(t)
    k = np.nonzero((pay == last) & (ts > tp))[0]
    assert len(k) >= 1 and k[0] + 1 < len(ts), (pay.tolist(), (ts - tp).tolist())
    k = k[0]
    assert peer[k + 1] != peer[k] and ts[k + 1] == ts[k] and pay[k + 1] == MSS
    c = gpu_run(r[0])
    assert_same(r, c)
    c.close()


def test_traced_kernel_records(ref):
    """Case 1 on the traced kernel (k_execute): record for record the oracle's trace, so the
    cached packet has no second IF_POP and the head packets sent with it have theirs."""
    r = ref("plain_100M")
    c = gpu_run(r[0], trace=True)
    assert_same(r, c, trace=True)
    tg = c.trace()
    assert np.count_nonzero(tg["kind"] == sgn.TRACE_IF_POP) == np.count_nonzero(tg["kind"] == sgn.TRACE_SEND)
    c.close()
