"""What stands in the network at a round edge, from the ORACLE's trace alone (CPU only; the expected
values of tests/test_gpu_backlog.py never come from libsgn).

The oracle (trace=True) is stepped round by round to an edge — round() while the simulation is
active and the window starts below the target, the rule of sgn_run_until — and its trace up to that
edge is a prefix, cut at ora_sim_trace_count. Every packet is followed by (source host, source
event id): SEND (flags == 0; peer = destination, b = delivery time, c = event id), then POP at the
destination (peer = source, c = event id, a = time), then DELIVER or CODEL_DROP there. Per host h
at the edge:

  in flight      the successful SENDs to h without a POP: their count, the min and max of b;
  router         POPs at h minus DELIVERs minus CODEL_DROPs = router_packets + (ROUTER_HELD ? 1 : 0).
                 The queue is FIFO in POP order. relay_inet_in runs in the event that queued a packet
                 and forwards until the queue is empty or the token bucket refuses the packet it
                 took, so at a round edge a non-empty backlog has its oldest packet held:
                 ROUTER_HELD <=> backlog > 0, router_packets = backlog - 1, and router_oldest is the
                 POP time of the oldest packet that is not the held one;
  router_bytes   wire bytes of the queued packets: packets * (payload_len + 28) under PERIODIC
                 traffic; else from the later DELIVER record of each queued packet (it carries
                 payload and tag) — a host with a queued packet that is dropped later, or never
                 delivered, is left out (bytes_known False);
  out held       IF_POPs at h minus SENDs of any flag minus LOCALs (0 or 1; before the stop time);
  send queue     datagrams pushed minus IF_POPs, bytes likewise (an IF_POP record carries payload
                 and tag). Pushed: under EXTERNAL traffic the submitted datagrams with send_time
                 below the window start minus the BLOCKED drain records; for the synthetic apps
                 the firings of the app timer below the window start (PERIODIC: start + k * period;
                 a TGEN client: start, then think(k) apart — sgn_workload.h) and, on a TGEN server,
                 one response train per delivered request. The synthetic figures hold while the
                 oracle counts no refused push (app_blocked == 0 at the edge: send_known);
  submit_pending under EXTERNAL traffic the submitted datagrams at or after the window start.
"""
import numpy as np

import sgn

S0 = sgn.SIMULATION_START
INVALID = sgn.EMUTIME_INVALID
M64 = (1 << 64) - 1
MSS = 1472
TAG_REQ = 0x10000
SALT_START, SALT_THINK = 0xFFFFFFFF00000001, 0xFFFFFFFF00000002
DRAIN_BLOCKED = 5
ROW_FIELDS = ("flags", "router_packets", "send_packets", "router_bytes", "send_bytes", "router_oldest",
              "inflight_packets", "submit_pending", "inflight_earliest", "inflight_latest")


# ---- sgn_workload.h, restated ----
def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def flow_hash(seed, a, b):
    return mix64(mix64(seed ^ ((0x9E3779B97F4A7C15 * (a + 1)) & M64)) ^ ((0xD1B54A32D192ED03 * (b + 1)) & M64))


def app_start(tr, host):
    j = flow_hash(tr.flow_seed, host, SALT_START) % (tr.start_jitter_ns + 1) if tr.start_jitter_ns else 0
    return S0 + tr.start_ns + j


def tgen_think(tr, host, k):
    j = flow_hash(tr.flow_seed ^ SALT_THINK, host, k) % (tr.period_jitter_ns + 1) if tr.period_jitter_ns else 0
    return tr.period_ns + j


def header_bytes(tag):
    k = (np.asarray(tag, dtype=np.uint64) >> np.uint64(29)) & np.uint64(3)
    return np.where(k == 0, 28, np.where(k == 1, 40, 44)).astype(np.uint64)


def wire_of(b):
    """Wire bytes of a DELIVER / IF_POP record's b = payload | tag << 32."""
    b = np.asarray(b, dtype=np.uint64)
    return (b & np.uint64(0xFFFFFFFF)) + header_bytes(b >> np.uint64(32))


# ---- the oracle at the edges ----
def advance(o, t):
    """Whole windows until the next one would start at or after t (or the end)."""
    while True:
        ws, _, active = o.window()
        if not active or ws >= t:
            return
        o.round()


def edge_of(o):
    return {"win": o.window(), "stats": o.stats(), "trace_n": int(o.L.ora_sim_trace_count(o.h))}


def oracle_edges(o, targets):
    out = []
    for t in targets:
        advance(o, t)
        out.append(edge_of(o))
    return out


def pkey(host, eid):
    host, eid = np.asarray(host, dtype=np.uint64), np.asarray(eid, dtype=np.uint64)
    assert eid.size == 0 or int(eid.max()) < 1 << 40
    return (host << np.uint64(40)) | eid


class External:
    """What the CPU side of an EXTERNAL run knows at an edge: the datagrams submitted so far (the
    first `submitted` of dg, in send-time order) and the oracle's drain records of the whole run."""

    def __init__(self, dg, submitted, drains):
        self.dg, self.submitted, self.drains = dg, submitted, drains


class Model:
    def __init__(self, trace, hosts, cfg, tr):
        """trace: the oracle's WHOLE trace (the payloads of queued packets come from later DELIVER
        records); an edge's state is computed from its prefix."""
        self.trace, self.n, self.cfg, self.tr = trace, hosts.n, cfg, tr
        self.kind = int(tr.kind)
        d = trace[trace["kind"] == sgn.TRACE_DELIVER]
        k = pkey(d["peer"], d["c"])
        order = np.argsort(k)
        self.deliver_key, self.deliver_wire = k[order], wire_of(d["b"])[order]
        self.servers = set()
        if self.kind == sgn.TRAFFIC_TGEN:
            self.servers = set(int(s) for s in np.ctypeslib.as_array(tr.server_hosts, (tr.n_servers,)))
        self.start = [app_start(tr, h) for h in range(self.n)]

    # synthetic apps: datagrams pushed by host h's app timer before ws, and their wire bytes
    def _timer_pushes(self, h, ws):
        tr = self.tr
        ws = min(ws, S0 + int(self.cfg.stop_time_ns))  # (no event at or after the stop time runs)
        if self.kind == sgn.TRAFFIC_PERIODIC:
            t0 = self.start[h]
            k = 0 if t0 >= ws else (ws - 1 - t0) // tr.period_ns + 1
            return k, k * (tr.payload_len + 28)
        if self.kind == sgn.TRAFFIC_TGEN and h not in self.servers:
            t, k = self.start[h], 0
            while t < ws:
                t += tgen_think(tr, h, k)
                k += 1
            return k, k * (tr.req_payload + 28)
        return 0, 0

    def at(self, edge, ext=None):
        n = self.n
        ws = edge["win"][0]
        T = self.trace[: edge["trace_n"]]
        kind = T["kind"]
        r = {f: np.zeros(n, dtype=np.uint64) for f in ROW_FIELDS}
        # ---- in flight ----
        send = T[(kind == sgn.TRACE_SEND) & (T["flags"] == 0)]
        pop = T[kind == sgn.TRACE_POP]
        sk, pk = pkey(send["host"], send["c"]), pkey(pop["peer"], pop["c"])
        assert len(np.unique(sk)) == len(sk) and np.all(np.isin(pk, sk))  # (the oracle's own identities)
        fl = send[~np.isin(sk, pk)]
        dst = fl["peer"].astype(np.int64)
        r["inflight_packets"] = np.bincount(dst, minlength=n).astype(np.uint64)
        r["inflight_earliest"][:] = INVALID
        np.minimum.at(r["inflight_earliest"], dst, fl["b"])
        np.maximum.at(r["inflight_latest"], dst, fl["b"])
        assert len(fl) == 0 or int(fl["b"].min()) >= ws  # (everything below the window start was popped)
        # ---- router ----
        done = T[(kind == sgn.TRACE_DELIVER) | (kind == sgn.TRACE_CODEL_DROP)]
        dk = pkey(done["peer"], done["c"])
        assert np.all(np.isin(dk, pk))
        out = pop[~np.isin(pk, dk)]
        out = out[np.lexsort((out["seq"], out["host"]))]  # per host, in POP order
        backlog = np.bincount(out["host"].astype(np.int64), minlength=n)
        r["router_oldest"][:] = INVALID
        bytes_known = np.ones(n, dtype=bool)
        first = np.concatenate([[0], np.cumsum(backlog)])
        for h in np.nonzero(backlog)[0]:
            q = out[first[h] + 1: first[h + 1]]  # (the oldest one is held by relay_inet_in)
            r["flags"][h] |= sgn.BACKLOG_ROUTER_HELD
            r["router_packets"][h] = len(q)
            if len(q):
                assert np.all(np.diff(q["a"].astype(np.int64)) >= 0)
                r["router_oldest"][h] = q["a"][0]
                if self.kind == sgn.TRAFFIC_PERIODIC:
                    r["router_bytes"][h] = len(q) * (self.tr.payload_len + 28)
                else:
                    qk = pkey(q["peer"], q["c"])
                    i = np.searchsorted(self.deliver_key, qk)
                    i[i >= len(self.deliver_key)] = 0
                    hit = len(self.deliver_key) > 0 and np.all(self.deliver_key[i] == qk)
                    if hit:
                        r["router_bytes"][h] = self.deliver_wire[i].sum(dtype=np.uint64)
                    else:
                        bytes_known[h] = False
        # ---- relay_inet_out ----
        ifpop = T[kind == sgn.TRACE_IF_POP]
        n_ifpop = np.bincount(ifpop["host"].astype(np.int64), minlength=n)
        n_send = np.bincount(T["host"][kind == sgn.TRACE_SEND].astype(np.int64), minlength=n)
        n_local = np.bincount(T["host"][kind == sgn.TRACE_LOCAL].astype(np.int64), minlength=n)
        held = n_ifpop - n_send - n_local
        assert held.min() >= 0 and held.max() <= 1
        r["flags"][held == 1] |= sgn.BACKLOG_OUT_HELD
        popped_bytes = np.zeros(n, dtype=np.uint64)
        np.add.at(popped_bytes, ifpop["host"].astype(np.int64), wire_of(ifpop["b"]))
        # ---- send queue ----
        pushed = np.zeros(n, dtype=np.int64)
        pushed_bytes = np.zeros(n, dtype=np.uint64)
        send_known = True
        if self.kind == sgn.TRAFFIC_EXTERNAL:
            src, dip, pay, t, handle, wire = ext.dg
            j = ext.submitted
            src, pay, t, handle, wire = src[:j], pay[:j], t[:j], handle[:j], wire[:j]
            w = np.where(wire == 0, pay + 28, wire).astype(np.uint64)
            dr = ext.drains
            blocked = dr[(dr["status"] == DRAIN_BLOCKED) & (dr["time"] < ws)]
            ok = (t < ws) & ~np.isin(handle, blocked["handle"])
            assert len(np.unique(handle)) == len(handle) and int(((t < ws) & ~ok).sum()) == len(blocked)
            pushed = np.bincount(src[ok].astype(np.int64), minlength=n)
            np.add.at(pushed_bytes, src[ok].astype(np.int64), w[ok])
            r["submit_pending"] = np.bincount(src[t >= ws].astype(np.int64), minlength=n).astype(np.uint64)
        else:
            send_known = edge["stats"]["app_blocked"] == 0
            for h in range(n):
                pushed[h], pushed_bytes[h] = self._timer_pushes(h, ws)
            if self.kind == sgn.TRAFFIC_TGEN:  # a response train per request delivered at a server
                dl = T[kind == sgn.TRACE_DELIVER]
                tag = dl["b"] >> np.uint64(32)
                for rec, tg in zip(dl, tag):
                    h = int(rec["host"])
                    if h in self.servers and int(tg) & TAG_REQ:
                        size = int(self.tr.file_bytes[int(tg) & 3])
                        k = (size + MSS - 1) // MSS
                        if k:
                            pushed[h] += k
                            pushed_bytes[h] += np.uint64((k - 1) * (MSS + 28) + (size - (k - 1) * MSS) + 28)
        if send_known:
            assert np.all(pushed >= n_ifpop) and np.all(pushed_bytes >= popped_bytes)
            r["send_packets"] = (pushed - n_ifpop).astype(np.uint64)
            r["send_bytes"] = pushed_bytes - popped_bytes
            assert np.all((r["send_packets"] == 0) == (r["send_bytes"] == 0))
            if self.kind != sgn.TRAFFIC_TGEN:  # (one datagram per entry; a TGEN entry is a train)
                assert int(r["send_packets"].max()) <= self.cfg.out_fifo_cap
        x = Expect(edge, r, bytes_known, send_known)
        x.if_pops = n_ifpop  # (per host, cumulative: where the send ring's head has come to)
        return x


class Expect:
    """Per-host arrays (ROW_FIELDS, u64, indexed by HostId) at one edge; bytes_known[h]: router_bytes
    of h is modelled; send_known: the send queue's fields are."""

    def __init__(self, edge, r, bytes_known, send_known):
        self.edge, self.r, self.bytes_known, self.send_known = edge, r, bytes_known, send_known
        self.n = len(bytes_known)
        self.ws = edge["win"][0]

    def has_row(self):
        nz = np.zeros(self.n, dtype=bool)
        for f in ("flags", "router_packets", "send_packets", "router_bytes", "inflight_packets", "submit_pending"):
            nz |= self.r[f] != 0
        return nz

    def total(self, lo=0, hi=None):
        """sgn_backlog_info::total over the hosts [lo, hi)."""
        s = slice(lo, self.n if hi is None else hi)
        r = self.r
        return [int(r["router_packets"][s].sum()), int(r["router_bytes"][s].sum()),
                int((r["flags"][s] & sgn.BACKLOG_ROUTER_HELD != 0).sum()), int(r["send_packets"][s].sum()),
                int(r["send_bytes"][s].sum()), int((r["flags"][s] & sgn.BACKLOG_OUT_HELD != 0).sum()),
                int(r["inflight_packets"][s].sum()), int(r["submit_pending"][s].sum())]

    def maxima(self, lo=0, hi=None):
        """(max_router_packets, its host, max_sojourn_ns, its host, inflight_earliest) over [lo, hi):
        over the hosts with a queued packet, the lowest HostId on equal values; 0 / 0 without one."""
        hi = self.n if hi is None else hi
        rp, old = self.r["router_packets"][lo:hi], self.r["router_oldest"][lo:hi]
        ie = self.r["inflight_earliest"][lo:hi]
        earliest = int(ie.min()) if len(ie) else INVALID
        if not rp.any():
            return 0, 0, 0, 0, earliest
        hq = int(np.argmax(rp))  # (the first of equal values)
        ho = int(np.argmin(old))
        return int(rp[hq]), lo + hq, self.ws - int(old[ho]), lo + ho, earliest


# ---- the scenarios of tests/test_backlog_model.py and tests/test_gpu_backlog.py ----
MS = 1_000_000


def periodic_world(n=200, hosts_per_wave=0):
    """A 1 ms period against links of 1 Mbit/s at every fourth host (20 Mbit/s elsewhere): the slow
    hosts' CoDel queues pass one page (16 runs) from 60 ms on and their send queues grow to ~170
    datagrams by 200 ms (fifo 256: no push is refused, so the send queue is modelled)."""
    from test_gpu_parity import scenario
    bw = np.where(np.arange(n) % 4 == 0, 1_000_000, 20_000_000).astype(np.uint64)
    args = scenario(n=n, V=50, bw=bw, fifo=256, stop_ns=280 * MS)
    args[3].hosts_per_wave = hosts_per_wave
    return args


PERIODIC_TARGETS = [S0 + k * 20 * MS for k in range(1, 11)]


def cold_world():
    """A 25 ms period against 500 kbit/s links at every fourth host: queues and held packets come
    and go, so hosts that had cold state earlier are idle (F_COLD clear, stale cold lines) later."""
    from test_gpu_parity import scenario
    bw = np.where(np.arange(200) % 4 == 0, 500_000, 20_000_000).astype(np.uint64)
    return scenario(n=200, V=50, bw=bw, period_ns=25 * MS, stop_ns=400 * MS)


COLD_TARGETS = [S0 + k * 5 * MS for k in range(1, 21)]


def tgen_world():
    """270 clients at 20 Mbit/s (a few at 3 Mbit/s) fetch 30-200 KB files from 30 servers at
    100 Mbit/s: trains stand in the clients' CoDel queues (hundreds of packets) and in the
    servers' send queues, few packets are dropped before 250 ms."""
    from test_gpu_parity import scenario
    n = 300
    bw = np.where(np.arange(n) % 10 == 0, 100_000_000, 20_000_000).astype(np.uint64)
    bw[7::37] = 3_000_000
    g, used, hosts, cfg, _ = scenario(n=n, V=30, kind=sgn.TRAFFIC_TGEN, stop_ns=1_000_000_000, bw=bw, tor=True)
    tr = sgn.make_traffic(sgn.TRAFFIC_TGEN, period_ns=100 * MS, period_jitter_ns=100 * MS, start_jitter_ns=20 * MS,
                          servers=np.arange(0, n, 10), file_bytes=(30 * 1024, 100 * 1024, 200 * 1024))
    return g, used, hosts, cfg, tr


TGEN_TARGETS = [S0 + k * 50 * MS for k in range(1, 6)]
EXT_STEP = 20 * MS


def oracle_sim(oracle, args):
    g, used, hosts, cfg, tr = args
    lat, loss = oracle.routes(g, used)
    return oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=True)


def expect_at(oracle, args, targets, full=False):
    """The model at the edges sgn_run_until(target) stops at: (oracle, [Expect]). full: the oracle
    runs on to the end afterwards (the payloads of queued packets are in later DELIVER records)."""
    o = oracle_sim(oracle, args)
    edges = oracle_edges(o, targets)
    if full:
        o.run()
    m = Model(o.trace(), args[2], args[3], args[4])
    return o, [m.at(e) for e in edges]


def submitted_by(dg, k, step=EXT_STEP, look=1_000_000):
    """Datagrams drive_ahead has submitted when step k's advance returns."""
    return int(np.searchsorted(dg[3], S0 + k * step + look, side="left"))
