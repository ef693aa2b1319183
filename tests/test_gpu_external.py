"""EXTERNAL traffic (CPU-resident applications: sgn_submit / sgn_drain) on the round kernels a
throughput-minded controller reaches (-m gpu): it submits ahead and runs many rounds per call
(external_common.drive_ahead), so the rounds run in the persistent kernel k_rounds<EXTERNAL, *>
(sgn_run_until / sgn_run), with the diagnostic stamps in k_rounds_diag<EXTERNAL, *>
(test_gpu_event_path.test_stamps_on_is_bit_exact[external]) and, on a local shard group, in
k_rounds_x<EXTERNAL> or in the per-round exchange with k_import.

Every comparison is bit for bit against the oracle driven by the same calls in the same order:
every field of every drain record, then the counters, the window and every host's digests
(assert_same_run). Every case also proves that the kernel it is about ran (a persistent grid,
launch counters, the exchange mode, big-slab pieces) and that the fates it claims occurred; the
worlds and seeds were chosen on the oracle alone (tests/test_external_oracle.py runs every case
below on the CPU and asserts the same statuses and counts)."""
import ctypes as C

import numpy as np
import pytest

import sgn
from external_common import (RUNAHEAD, advance_to, calendar_shape, datagrams, drive_ahead,
                             external_world)
from test_gpu_parity import assert_same_run, ctxf  # noqa: F401 (ctxf: fixture)

pytestmark = pytest.mark.gpu

S0 = sgn.SIMULATION_START
MS = 1_000_000
STEPS = (1 * MS, 7 * MS, 50 * MS)
ALL5 = (sgn.DRAIN_DELIVERED, sgn.DRAIN_LOCAL, sgn.DRAIN_LOSS, sgn.DRAIN_UNKNOWN, sgn.DRAIN_BLOCKED)
EOVERFLOW = -75
_CASES = {}


# ---- the cases: (world, datagrams, route latencies, drive_ahead arguments, statuses claimed) ----
def _merge(parts):
    """Datagram sets merged in send-time order, with fresh unique handles."""
    cat = [np.concatenate([p[i] for p in parts]) for i in range(6)]
    order = np.argsort(cat[3], kind="stable")
    src, dip, pay, t, _, wire = (a[order] for a in cat)
    handle = (np.arange(len(t), dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    return src, dip, pay, t, handle, wire


def _fan_in(hosts, lat, senders, dst, arrive_ns, gap_ns=500, payload=100):
    """One datagram from every sender to dst, sent so that all reach dst's node within
    len(senders) * gap_ns of S0 + arrive_ns: one calendar bucket of the receiver's host group."""
    node = np.asarray(hosts.node_id)
    senders = np.asarray(senders, dtype=np.uint32)
    t = np.array([S0 + arrive_ns - int(lat[node[s], node[dst]]) + i * gap_ns for i, s in enumerate(senders)],
                 dtype=np.uint64)
    k = len(senders)
    return (senders, np.full(k, hosts.ip[dst], np.uint32), np.full(k, payload, np.uint32), t,
            np.zeros(k, np.uint64), np.zeros(k, np.uint32))


def _fan_in_case(oracle, n, senders, dst, background):
    world = external_world(n=n, bw=1_000_000_000, fifo=64, stop_ns=3_000 * MS)
    hosts = world[2]
    lat, _ = oracle.routes(world[0], world[1])
    parts = [datagrams(hosts, k=background, span_ns=100 * MS)]
    for b in range(3):  # three bursts, 20 ms apart, each into one bucket 100 us after its start
        parts.append(_fan_in(hosts, lat, senders, dst, (70 + 20 * b) * MS + 100_000))
    return world, _merge(parts), lat


def build_case(oracle, name):
    """name -> dict(world, dg, lat, kw: drive_ahead's arguments, expect: statuses that occur)."""
    if name in _CASES:
        return _CASES[name]
    kw, expect = {}, ALL5
    if name == "default":  # external_common's world as test_external_oracle drives it
        world = external_world()
        dg = datagrams(world[2])
    elif name == "long":  # everything submitted before one run-until of 200 ms: > 128 rounds in it
        world = external_world()
        dg = datagrams(world[2], span_ns=100 * MS)
        kw = dict(step_ns=200 * MS)
    elif name == "fan-in":
        # 44 fast senders to host 50, three times, each burst into one bucket of host group 0
        senders = [h for h in range(60) if h % 7 and h != 50][:44]
        world, dg, lat = _fan_in_case(oracle, 60, senders, 50, 200)
        kw = dict(step_ns=7 * MS)
        expect = (sgn.DRAIN_DELIVERED, sgn.DRAIN_LOSS)
    elif name == "codel":
        # one CoDel page per host plus 64 to begin with (codel_cap = 1), and 4000 small datagrams
        # within 60 ms to the nine hosts behind 200 kbit/s down-links: about 0.5 s of standing queue
        world = external_world(codel_cap=1, fifo=64, stop_ns=3_000 * MS)
        hosts = world[2]
        rng = np.random.default_rng(17)
        k = 4000
        fast = np.array([h for h in range(hosts.n) if h % 7])
        extra = (rng.choice(fast, k).astype(np.uint32), hosts.ip[rng.choice(np.arange(0, hosts.n, 7), k)],
                 np.zeros(k, np.uint32), S0 + np.sort(rng.integers(0, 60 * MS, k)).astype(np.uint64),
                 np.zeros(k, np.uint64), np.zeros(k, np.uint32))
        dg = _merge([datagrams(hosts), extra])
        kw = dict(step_ns=7 * MS)
        expect = ALL5 + (sgn.DRAIN_CODEL,)
    elif name == "round-robin":
        world = external_world(qdisc=sgn.QDISC_ROUND_ROBIN)
        dg = datagrams(world[2])
        kw = dict(step_ns=7 * MS)
    elif name == "dynamic":
        # edge latencies of 1-10 ms keep the dynamic calendar (4 x the longest path) within the
        # 256 buckets persistent rounds need; a window is at most the longest path long
        world = external_world(lat_hi_us=10_000, dynamic=True)
        dg = datagrams(world[2])
        lat, _ = oracle.routes(world[0], world[1])
        kw = dict(step_ns=7 * MS, lookahead_ns=int(lat.max()))
    elif name == "gaps":
        # four bursts of 30 ms, 330 ms apart: the calendar (128 buckets of 1 ms) is idle for more
        # than its span between them, the controller moves the window to its next send
        # (sgn_set_window) and the rounds after it reach bucket indices the previous burst used
        world = external_world(stop_ns=2_000 * MS)
        parts = []
        for b in range(4):
            d = datagrams(world[2], k=150, seed=5 + b, span_ns=30 * MS)
            parts.append(d[:3] + (d[3] + np.uint64(b * 330 * MS),) + d[4:])
        dg = _merge(parts)
        kw = dict(step_ns=50 * MS)
    elif name == "horizon":
        # everything submitted before one run-until, the furthest datagrams 1 to 8 ns below the
        # horizon of the first window (the last bucket sgn_submit accepts)
        world = external_world()
        hosts = world[2]
        lat, _ = oracle.routes(world[0], world[1])
        nb, bw = calendar_shape(lat, world[3])
        far = S0 + np.uint64((nb - 2) * bw) - (1 + np.arange(8, dtype=np.uint64))
        edge = (np.arange(10, 18, dtype=np.uint32), hosts.ip[20:28], np.full(8, 300, np.uint32), far,
                np.zeros(8, np.uint64), np.zeros(8, np.uint32))
        dg = _merge([datagrams(hosts, span_ns=60 * MS), edge])
        kw = dict(step_ns=200 * MS)
    elif name.startswith("sweep-"):
        world, dg, kw, expect = _sweep_case(oracle, int(name[6:]))
    else:
        raise KeyError(name)
    lat, _ = oracle.routes(world[0], world[1])
    _CASES[name] = dict(world=world, dg=dg, lat=lat, kw=kw, expect=expect)
    return _CASES[name]


N_SWEEP = 12


def draw(case):
    """Sweep case -> the parameters of a world, its datagrams, the driver and the environment."""
    rng = np.random.default_rng(9000 + case)
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    return dict(
        n=int(rng.integers(20, 201)), V=int(rng.integers(5, 41)), graph_seed=int(rng.integers(1, 1000)),
        bw=pick((1_000_000, 2_000_000, 100_000_000)), slow_every=pick((3, 7, 1000)),  # bandwidth mix
        fifo=pick((2, 4, 64)), k=int(rng.integers(300, 801)), span_ns=int(rng.integers(40, 101)) * MS,
        dg_seed=int(rng.integers(1, 1000)), unknown=pick((0.0, 0.05, 0.3)), to_self=pick((0.0, 0.05, 0.3)),
        wire_kinds=pick(((0,), (1,), (2, 3), (0, 1, 2, 3))),
        step_frac=pick((0.0, 0.05, 0.2, 0.5, 0.9)),  # of the submit horizon (0: one runahead a step)
        persistent=bool(rng.integers(0, 2)), hpw=pick((None, "16", "32", "64")),
        host_order=pick((None, "id")), peer64=pick((None, "1")))


def sweep_env(p):
    env = {"SGN_HOSTS_PER_WAVE": p["hpw"], "SGN_HOST_ORDER": p["host_order"], "SGN_PEER64": p["peer64"],
           "SGN_PERSISTENT": None if p["persistent"] else "0"}
    return {k: v for k, v in env.items() if v is not None}


def _sweep_case(oracle, case):
    p = draw(case)
    world = external_world(n=p["n"], V=p["V"], seed=p["graph_seed"], bw=p["bw"], fifo=p["fifo"],
                           lat_hi_us=20_000, slow_every=p["slow_every"], stop_ns=5_000 * MS)
    dg = datagrams(world[2], k=p["k"], seed=p["dg_seed"], span_ns=p["span_ns"], unknown=p["unknown"],
                   to_self=p["to_self"], wire_kinds=p["wire_kinds"])
    lat, _ = oracle.routes(world[0], world[1])
    nb, bw = calendar_shape(lat, world[3])
    step = max(RUNAHEAD, int(p["step_frac"] * ((nb - 2) * bw - RUNAHEAD)) // 1000 * 1000)
    expect = [sgn.DRAIN_DELIVERED]
    if p["unknown"]:
        expect.append(sgn.DRAIN_UNKNOWN)
    if p["to_self"]:
        expect.append(sgn.DRAIN_LOCAL)
    return world, dg, dict(step_ns=step), tuple(expect)


# ---- helpers ----
def make_pair(ctxf, oracle, world, drain_cap=1 << 16, flags=0):
    g, used, hosts, cfg, tr = world
    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr)
    c = ctxf(flags=flags)
    c.routes_build(g, used)
    c.hosts_set(hosts)
    c.drain_enable(drain_cap)
    c.sim_init(cfg, tr)
    return o, c


def assert_records(do, dc, expect=()):
    assert len(do) == len(dc), (len(do), len(dc))
    for f in sgn.DRAIN_DTYPE.names:
        bad = np.nonzero(do[f] != dc[f])[0]
        assert len(bad) == 0, (f, do[bad[:3]], dc[bad[:3]])
    st = np.bincount(dc["status"], minlength=6)
    for s in expect:
        assert st[s] > 0, (s, st)
    return st


def assert_persistent(c, timed=False):
    info = c.engine_info()
    assert info["persistent_grid"] > 0 and info["persistent_fallbacks"] == 0, info
    if timed:
        assert c.kernel_times()["k_rounds"][0] > 0, c.kernel_times()
    else:
        assert c.kernel_launches_total()["k_rounds"] > 0, c.kernel_launches_total()
    return info


def run_case(ctxf, oracle, name, persistent=True, flags=0, **over):
    case = build_case(oracle, name)
    o, c = make_pair(ctxf, oracle, case["world"], flags=flags)
    log = {}
    kw = dict(case["kw"], **over)
    (do, dc), rounds = drive_ahead([o, c], case["dg"], log=log, **kw)
    assert len(dc) == len(case["dg"][3])  # one record per datagram: the simulation ran dry
    st = assert_records(do, dc, case["expect"])
    info = c.engine_info()
    if persistent:
        assert_persistent(c, timed=bool(flags & sgn.CREATE_TIME_KERNELS))
    else:
        assert info["persistent_grid"] == 0, info
    assert c.stats()["rounds"] == rounds > 0
    assert_same_run(o, c, case["world"][2].n, trace=False)
    return o, c, st, log


# ---- single shard ----
@pytest.mark.parametrize("step_ms,persistent", [(1, "1"), (7, "1"), (50, "1"), (50, "0")])
def test_submit_ahead_run_until(ctxf, oracle, monkeypatch, step_ms, persistent):
    """The default world in steps of 1, 7 and 50 ms: k_rounds<EXTERNAL, false> through
    sgn_run_until; the 50-ms case also on per-round launches through sgn_run_until
    (SGN_PERSISTENT=0: k_execute<false, EXTERNAL>, untraced)."""
    monkeypatch.setenv("SGN_PERSISTENT", persistent)
    _, _, _, log = run_case(ctxf, oracle, "default", persistent=persistent == "1", step_ns=step_ms * MS)
    assert max(log["rounds_per_step"]) > 1  # many rounds per call


def test_one_run_until_crosses_the_launch_limit(ctxf, oracle):
    """More than 128 rounds (kPersistRounds) inside one sgn_run_until: two persistent launches."""
    _, c, _, log = run_case(ctxf, oracle, "long")
    assert log["rounds_per_step"][0] > 128, log["rounds_per_step"]
    assert c.kernel_launches_total()["k_rounds"] >= 2


def test_fixed_round_counts_with_sgn_run(ctxf, oracle):
    """sgn_run(ctx, 29) in place of run-until, everything submitted before the first round; the
    oracle runs 29 rounds or stops at the end."""
    case = build_case(oracle, "long")
    o, c = make_pair(ctxf, oracle, case["world"])
    src, dip, pay, t, handle, wire = case["dg"]
    info = c.engine_info()
    assert int(t[-1]) < S0 + (info["calendar_buckets"] - 2) * info["bucket_width_ns"]
    rec = [[], []]
    for s in (o, c):
        s.submit(src, dip, pay, t, handle, wire_len=wire)
    calls = 0
    while c.window()[2]:
        assert o.run(29) == c.run(29)
        assert o.window() == c.window()
        calls += 1
        if calls % 2 == 0:
            assert o.rng_next_u64(1) == c.rng_next_u64(1)
            for i, s in enumerate((o, c)):
                rec[i].append(s.drain(0, 30))
                rec[i].append(s.drain(30, 1 << 31))
    assert calls >= 4 and not o.window()[2]
    for i, s in enumerate((o, c)):
        rec[i].append(s.drain())
    do, dc = (np.concatenate(r) for r in rec)
    assert len(dc) == len(t)
    assert_records(do, dc, case["expect"])
    assert_persistent(c)
    assert_same_run(o, c, case["world"][2].n, trace=False)


def test_big_slab_kernel(ctxf, oracle, monkeypatch):
    """k_rounds<EXTERNAL, true>: 16-run slabs that may grow to 32 (test hooks) and 44 senders whose
    datagrams reach one host inside one bucket: the slab spills, the calendar is re-laid out with
    extensions and the gathers order the hot slab in pieces."""
    monkeypatch.setenv("SGN_SLAB_CAP", "16")
    monkeypatch.setenv("SGN_SLAB_LIM", "32")
    _, c, st, _ = run_case(ctxf, oracle, "fan-in")
    info = c.engine_info()
    print({k: info[k] for k in ("slab_extensions", "big_slab_pieces", "calendar_spill_runs", "slab_capacity")})
    assert info["big_slab_pieces"] > 0 or info["slab_extensions"] > 0, info
    assert st[sgn.DRAIN_DELIVERED] > 3 * 33


def test_codel_pool_grows_inside_persistent_launches(ctxf, oracle):
    _, c, st, _ = run_case(ctxf, oracle, "codel")
    info = c.engine_info()
    print({k: info[k] for k in ("codel_pages", "codel_page_allocs", "codel_pool_grows")}, st)
    assert info["codel_pool_grows"] >= 1, info
    assert info["codel_pages_free"] + info["codel_pages_chained"] == info["codel_pages"], info
    assert st[sgn.DRAIN_CODEL] > 0 and c.stats()["codel_dropped"] == st[sgn.DRAIN_CODEL]


def test_idle_gaps_longer_than_the_calendar(ctxf, oracle):
    """Bursts of datagrams with idle gaps longer than the calendar's span between them: the
    controller moves the window over the gap and the persistent rounds after it reuse the
    bucket indices of the burst before."""
    case = build_case(oracle, "gaps")
    _, c, _, log = run_case(ctxf, oracle, "gaps")
    info = c.engine_info()
    assert info["calendar_buckets"] * info["bucket_width_ns"] < 300 * MS, info
    assert int(case["dg"][3][-1]) - S0 > 3 * 330 * MS and log["k"] > 20


def test_submit_up_to_the_horizon(ctxf, oracle):
    """Datagrams in the last nanoseconds sgn_submit accepts ahead of the window, submitted with
    everything else before one run-until of many rounds: the far bucket is reached by the
    calendar's wrap while a persistent launch runs, 66 ms after the traffic before it."""
    case = build_case(oracle, "horizon")
    o, c, _, log = run_case(ctxf, oracle, "horizon")
    info = c.engine_info()
    assert (info["calendar_buckets"], info["bucket_width_ns"]) == calendar_shape(case["lat"], case["world"][3])
    assert int(case["dg"][3][-1]) == S0 + (info["calendar_buckets"] - 2) * info["bucket_width_ns"] - 1
    assert log["rounds_per_step"][0] > 64


def test_round_robin_qdisc(ctxf, oracle):
    """SGN_QDISC_ROUND_ROBIN with the bursty senders of datagrams() (three hosts send a quarter of
    the datagrams within 15 ms: full send queues, BLOCKED fates)."""
    run_case(ctxf, oracle, "round-robin")


def test_dynamic_runahead(ctxf, oracle):
    """use_dynamic_runahead with EXTERNAL traffic. The oracle supports it: its round loop
    (oracle.cpp execute_round / advance / runahead_get) is the same for every traffic kind, a
    submitted datagram goes through send_packet, which lowers min_used like any other send, and
    ora_sim_set_window only bounds the caller's window. Windows then grow up to the longest path,
    so the driver looks that far ahead when it submits."""
    o, c, _, _ = run_case(ctxf, oracle, "dynamic")
    assert c.stats()["min_used_latency_ns"] == o.stats()["min_used_latency_ns"] != sgn.EMUTIME_INVALID


@pytest.mark.parametrize("env", [{"SGN_HOSTS_PER_WAVE": "16"}, {"SGN_HOSTS_PER_WAVE": "64"},
                                 {"SGN_HOST_ORDER": "id"}, {"SGN_PEER64": "1"}],
                         ids=lambda e: "-".join(f"{k[4:].lower()}={v}" for k, v in e.items()))
def test_layout_knobs(ctxf, oracle, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, c, _, _ = run_case(ctxf, oracle, "default", step_ns=7 * MS)
    if "SGN_HOSTS_PER_WAVE" in env:
        assert c.engine_info()["hosts_per_wave"] == int(env["SGN_HOSTS_PER_WAVE"])


@pytest.mark.parametrize("case", range(N_SWEEP))
def test_sweep(ctxf, oracle, monkeypatch, case):
    p = draw(case)
    for k, v in sweep_env(p).items():
        monkeypatch.setenv(k, v)
    run_case(ctxf, oracle, f"sweep-{case}", persistent=p["persistent"])


def test_snapshot_inside_a_submit_ahead_run(ctxf, oracle):
    """A save after step 4 of the 7-ms run — the last drain was at step 3, so records wait on the
    device, and step 4 drew from a host RNG on the CPU, so a CPU-held state is outstanding — then
    to the end, back to the save and the same steps again on libsgn alone."""
    case = build_case(oracle, "default")
    o, c = make_pair(ctxf, oracle, case["world"])
    dg, n = case["dg"], case["world"][2].n
    log = {}
    drive_ahead([o, c], dg, 7 * MS, stop_step=4, log=log)
    nxt = log["nxt"]
    assert 0 < nxt < len(dg[3]) and len(log["draws"][1]) == 2
    assert o.rng_next_u64(3) == c.rng_next_u64(3)
    at = (c.window(), c.stats(), c.digests(0, n))
    snap = c.snapshot_save()
    log1 = {}
    (do, dc), rounds = drive_ahead([o, c], dg, 7 * MS, k0=4, nxt0=nxt, log=log1)
    assert rounds > 50 and len(dc) > 0 and log1["draws"][0] == log1["draws"][1] and len(log1["draws"][1]) > 3
    assert_records(do, dc)
    more = (o.rng_next_u64(3), o.rng_next_u64(1))
    assert more == (c.rng_next_u64(3), c.rng_next_u64(1))
    assert_persistent(c)
    assert_same_run(o, c, n, trace=False)
    c.snapshot_restore(snap)
    back = (c.window(), c.stats(), c.digests(0, n))
    assert back[0] == at[0] and back[1] == at[1] and back[2].tobytes() == at[2].tobytes()
    log2 = {}
    (dc2,), rounds2 = drive_ahead([c], dg, 7 * MS, k0=4, nxt0=nxt, log=log2)
    assert rounds2 == rounds and log2["draws"][0] == log1["draws"][1]
    assert_records(dc, dc2)
    assert (c.rng_next_u64(3), c.rng_next_u64(1)) == more
    assert_same_run(o, c, n, trace=False)
    c.snapshot_free(snap)


def test_drain_buffer_exhaustion_is_a_status(ctxf, oracle):
    """Eight drain records of room and twenty fates in one window (datagrams to an unknown address:
    each is decided at its send; the window after the first, empty one, [S0, S0 + 1), holds them
    all): sgn_round returns SGN_EOVERFLOW and names the drain buffer; the device write is
    bounds-checked, nothing faults."""
    world = external_world(n=10, V=5)
    _, c = make_pair(ctxf, oracle, world, drain_cap=8)
    k = 20
    t = S0 + 1000 * (1 + np.arange(k, dtype=np.uint64))
    c.submit(np.arange(k) % 10, np.full(k, 0x0AFF0001), np.full(k, 100), t)
    c.round()
    assert c.window() == (S0 + 1000, S0 + 1000 + RUNAHEAD, True) and len(c.drain()) == 0
    with pytest.raises(sgn.SgnError, match="drain buffer") as e:
        c.round()
    assert e.value.rc == EOVERFLOW


# ---- local shard groups ----
def shard_ranges(c, n, k):
    out = []
    for r in range(k):
        lo, hi = C.c_uint32(), C.c_uint32()
        c.L.sgn_shard_range(n, r, k, C.byref(lo), C.byref(hi))
        out.append((lo.value, hi.value))
    return out


def make_group(world, k, drain_cap=1 << 16):
    g, used, hosts, cfg, tr = world
    shards = [sgn.Context(shard_rank=r, shard_count=k) for r in range(k)]
    arr = (C.c_void_p * k)(*[c.h.value for c in shards])
    for c in shards:
        c.routes_build(g, used)
        c.hosts_set(hosts)
        c.drain_enable(drain_cap)
    shards[0].check(shards[0].L.sgn_comm_init_local(arr, k, 1 << 14))
    for c in shards:
        c.sim_init(cfg, tr)
    return shards, arr


def submit_to_owners(shards, ranges, dg, sel):
    """Each datagram of dg[sel] to the shard that owns its source, one call per shard."""
    src = dg[0]
    for c, (lo, hi) in zip(shards, ranges):
        m = sel & (src >= lo) & (src < hi)
        if m.any():
            c.submit(dg[0][m], dg[1][m], dg[2][m], dg[3][m], dg[4][m], wire_len=dg[5][m])


def run_group(shards, arr):
    done = C.c_uint64()
    shards[0].check(shards[0].L.sgn_run_local_group(arr, len(shards), 1 << 40, C.byref(done)))
    return done.value


# np.lexsort: the last key is the primary one. (host, time, src_host, src_eid, status) alone can tie:
# a host behind a slow link sends two queued datagrams at one token-bucket refill, and LOCAL, LOSS and
# UNKNOWN fates carry no event id. Such records have one source, hence one submitting shard, and
# a shard numbers its submissions in the order the oracle numbers the same ones: the slot breaks
# the tie alike on both sides.
KEY = ("tag", "status", "src_eid", "src_host", "time", "host")
ADD = ("packets_sent", "packets_loss_dropped", "packets_unknown_dst", "packet_events_popped", "delivered",
       "codel_dropped", "local_events", "local_delivered", "app_blocked", "bytes_delivered", "host_executions")
DIGESTS = ("tx", "rx", "app", "rng", "next_event_id", "n_sent", "n_popped", "n_delivered", "n_codel_dropped")


def by_key(d):
    return d[np.lexsort([d[f] for f in KEY])]


def compare_group(o, shards, ranges, n, expect):
    """The shards' drains (each for its own host range) against the unsharded oracle's records:
    every field except the slot bits of `tag` (a shard numbers its own submissions) and `handle`
    (the submitted one where the draining shard owns the source, else 0). No per-host digest
    mixes in the slot or the tag (oracle.cpp deliver_to_app / send_packet and engine.hip fold
    times, hosts, event ids and payload lengths only), so every digest is compared exactly."""
    do = by_key(o.drain())
    parts = []
    for c, (lo, hi) in zip(shards, ranges):
        parts.append(c.drain(lo, hi))
        assert len(c.drain()) == 0  # nothing filed under a host of another shard
    dc = by_key(np.concatenate(parts))
    assert len(do) == len(dc)
    for f in ("time", "src_eid", "host", "src_host", "dst_host", "status", "payload_len"):
        bad = np.nonzero(do[f] != dc[f])[0]
        assert len(bad) == 0, (f, do[bad[:3]], dc[bad[:3]])
    slot = np.uint32(0x1FFFFFFF)  # SGN_TAG_SLOT_MASK
    assert np.array_equal(do["tag"] & ~slot, dc["tag"] & ~slot) and np.all(dc["tag"] & sgn.TAG_EXT)
    owner = lambda h: np.searchsorted([hi for _, hi in ranges], h, side="right")  # noqa: E731
    same = owner(dc["src_host"]) == owner(dc["host"])
    assert np.array_equal(dc["handle"], np.where(same, do["handle"], 0))
    assert same.any() and (~same).any() and np.all(do["handle"] != 0)
    st = np.bincount(dc["status"], minlength=6)
    for s in expect:
        assert st[s] > 0, (s, st)
    so = o.stats()
    tot = {key: 0 for key in ADD}
    for c, (lo, hi) in zip(shards, ranges):
        assert c.window() == o.window()
        sc = c.stats()
        assert sc["rounds"] == so["rounds"]
        for key in ADD:
            tot[key] += sc[key]
        d1, d2 = o.digests(lo, hi), c.digests(lo, hi)
        for f in DIGESTS:
            assert np.array_equal(d1[f], d2[f]), (lo, f)
    for key in ADD:
        assert tot[key] == so[key], (key, tot[key], so[key])


def shard_case(oracle):
    """The default world with every datagram below the horizon at t = 0 and no two at one time."""
    if "shards" not in _CASES:
        world = external_world()
        dg = _merge([datagrams(world[2], span_ns=100 * MS, unique_times=True)])  # (handles != 0)
        lat, _ = oracle.routes(world[0], world[1])
        _CASES["shards"] = dict(world=world, dg=dg, lat=lat, kw={}, expect=ALL5)
    return _CASES["shards"]


def oracle_of(oracle, case):
    g, used, hosts, cfg, tr = case["world"]
    lat, loss = oracle.routes(g, used)
    return oracle.Sim(used, lat, loss, hosts, cfg, tr)


def check_transport(shards, persist):
    info = shards[0].engine_info()
    if persist is None:
        assert info["exchange_mode"] == 2 and info["persistent_x_launches"] > 0, info
    else:
        assert info["exchange_mode"] == 1 and info["persistent_x_launches"] == 0, info
    return info


@pytest.mark.parametrize("persist", [None, "0"], ids=["k_rounds_x", "k_import"])
@pytest.mark.parametrize("k", [2, 3])
def test_shards_everything_submitted_ahead(oracle, monkeypatch, k, persist):
    """Every datagram submitted before the first round, each to the shard that owns its source,
    then sgn_run_local_group to the end: the persistent k_rounds_x<EXTERNAL> with its peer inboxes
    (default) and the per-round exchange with k_import (SGN_LOCAL_PERSIST=0)."""
    if persist is not None:
        monkeypatch.setenv("SGN_LOCAL_PERSIST", persist)
    case = shard_case(oracle)
    dg, n = case["dg"], case["world"][2].n
    shards, arr = make_group(case["world"], k)
    info = shards[0].engine_info()
    assert int(dg[3][-1]) < S0 + (info["calendar_buckets"] - 2) * info["bucket_width_ns"]
    ranges = shard_ranges(shards[0], n, k)
    submit_to_owners(shards, ranges, dg, np.ones(len(dg[3]), bool))
    o = oracle_of(oracle, case)
    o.submit(dg[0], dg[1], dg[2], dg[3], dg[4], wire_len=dg[5])
    assert run_group(shards, arr) == o.run() > 100
    check_transport(shards, persist)
    compare_group(o, shards, ranges, n, case["expect"])


@pytest.mark.parametrize("k", [2, 3])
def test_shards_two_halves_around_a_run_until(oracle, k):
    """The datagrams before S0 + 40 ms (and one runahead), sgn_shards_run_until(S0 + 40 ms), the
    rest, then to the end."""
    case = shard_case(oracle)
    dg, n = case["dg"], case["world"][2].n
    T = S0 + 40 * MS
    first = dg[3] < T + RUNAHEAD
    assert 100 < first.sum() < len(first) - 100
    shards, arr = make_group(case["world"], k)
    ranges = shard_ranges(shards[0], n, k)
    o = oracle_of(oracle, case)
    submit_to_owners(shards, ranges, dg, first)
    o.submit(*(a[first] for a in dg[:5]), wire_len=dg[5][first])
    assert sgn.shards_run_until(shards, T) == advance_to(o, T) > 10
    assert all(c.window() == o.window() for c in shards)
    info = shards[0].engine_info()
    assert int(dg[3][-1]) < o.window()[0] + (info["calendar_buckets"] - 2) * info["bucket_width_ns"]
    submit_to_owners(shards, ranges, dg, ~first)
    o.submit(*(a[~first] for a in dg[:5]), wire_len=dg[5][~first])
    assert run_group(shards, arr) == o.run() > 10
    check_transport(shards, None)
    compare_group(o, shards, ranges, n, case["expect"])


def run_bursts(o, shards, arr, ranges, dg, horizon_ns):
    """The datagrams in bursts (cut where more than 100 ms pass without one): each burst is
    submitted whole, to the oracle and to the owning shards, and run until the simulation is dry;
    before every burst but the first, sgn_set_window moves the window of the oracle and of EVERY
    shard to the burst's first send. Returns the rounds of each burst."""
    t = dg[3]
    cuts = [0] + (np.nonzero(np.diff(t.astype(np.int64)) > 100 * MS)[0] + 1).tolist() + [len(t)]
    rounds = []
    for b in range(len(cuts) - 1):
        sel = np.zeros(len(t), bool)
        sel[cuts[b]:cuts[b + 1]] = True
        start = int(t[cuts[b]])
        if b:
            assert not o.window()[2] or o.window()[0] >= start
            for s in [o] + list(shards):
                s.set_window(start, start + RUNAHEAD)
        assert all(c.window() == o.window() for c in shards)
        assert int(t[cuts[b + 1] - 1]) < o.window()[0] + horizon_ns
        submit_to_owners(shards, ranges, dg, sel)
        o.submit(*(a[sel] for a in dg[:5]), wire_len=dg[5][sel])
        r = o.run()
        if shards:
            assert run_group(shards, arr) == r
        rounds.append(r)
    return rounds


@pytest.mark.parametrize("persist", [None, "0"], ids=["k_rounds_x", "k_import"])
def test_shards_set_window_over_idle_gaps(oracle, monkeypatch, persist):
    """A controller of a shard group whose simulation runs dry between its sends: it moves the
    window with sgn_set_window on every shard (the same window), submits the next burst and runs
    the group again, four times, with gaps longer than the calendar's span."""
    if persist is not None:
        monkeypatch.setenv("SGN_LOCAL_PERSIST", persist)
    case = build_case(oracle, "gaps")
    dg, n = case["dg"], case["world"][2].n
    shards, arr = make_group(case["world"], 2)
    info = shards[0].engine_info()
    ranges = shard_ranges(shards[0], n, 2)
    o = oracle_of(oracle, case)
    rounds = run_bursts(o, shards, arr, ranges, dg, (info["calendar_buckets"] - 2) * info["bucket_width_ns"])
    assert len(rounds) == 4 and min(rounds) > 20
    check_transport(shards, persist)
    compare_group(o, shards, ranges, n, case["expect"])


def fan_in_shards_case(oracle):
    if "fan-in-x" not in _CASES:
        # 100 hosts on two shards: 44 fast senders of shard 0 (hosts 0-49) to host 71 of shard 1
        senders = [h for h in range(50) if h % 7][:44]
        world, dg, lat = _fan_in_case(oracle, 100, senders, 71, 200)
        t = dg[3].copy()
        i = np.arange(len(t), dtype=np.uint64)
        t = np.maximum.accumulate(t - i) + i  # no two at one time
        _CASES["fan-in-x"] = dict(world=world, dg=dg[:3] + (t,) + dg[4:], lat=lat, kw={},
                                  expect=(sgn.DRAIN_DELIVERED, sgn.DRAIN_LOSS))
    return _CASES["fan-in-x"]


def test_shards_hot_fan_in(oracle, monkeypatch):
    """Senders on shard 0, one receiver on shard 1, 16-run slabs: the imported runs pass their
    slab's capacity on the receiving shard (spill area, re-layout with extensions or pieces)."""
    monkeypatch.setenv("SGN_SLAB_CAP", "16")
    monkeypatch.setenv("SGN_SLAB_LIM", "32")
    case = fan_in_shards_case(oracle)
    dg, n = case["dg"], case["world"][2].n
    shards, arr = make_group(case["world"], 2)
    info = shards[0].engine_info()
    assert int(dg[3][-1]) < S0 + (info["calendar_buckets"] - 2) * info["bucket_width_ns"]
    ranges = shard_ranges(shards[0], n, 2)
    submit_to_owners(shards, ranges, dg, np.ones(len(dg[3]), bool))
    o = oracle_of(oracle, case)
    o.submit(dg[0], dg[1], dg[2], dg[3], dg[4], wire_len=dg[5])
    assert run_group(shards, arr) == o.run() > 50
    check_transport(shards, None)
    i1 = shards[1].engine_info()
    print({k: i1[k] for k in ("slab_extensions", "big_slab_pieces", "calendar_spill_runs", "slab_capacity")})
    assert i1["calendar_spill_runs"] > 0 or i1["big_slab_pieces"] > 0 or i1["slab_extensions"] > 0, i1
    compare_group(o, shards, ranges, n, case["expect"])
