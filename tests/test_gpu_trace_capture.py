"""A trace of chosen hosts, taken out in ordered pieces and streamed into captures (-m gpu):
sgn_trace_hosts, sgn_trace_take (trace_take.hip), their snapshot rules, two shards, and the
capture loop (sgn.Capture, sgn.run_captured).

Every comparison is against the oracle's ONE full trace of the scenario (module fixtures; never
modified): a restricted trace is that trace filtered by host, field by field — seq and rng_pos
included — and the takes of a run, concatenated and sorted, are that trace again. Each scenario's
simulation itself is compared with assert_same_run (window, counters, digests): neither the host
set nor the takes change it.
"""
import ctypes as C

import numpy as np
import pytest

import sgn
from external_common import datagrams, drive_ahead, external_world
from test_gpu_parity import assert_same_run, ctxf, scenario  # noqa: F401 (ctxf: a fixture)

pytestmark = pytest.mark.gpu

S0 = sgn.SIMULATION_START
EINVAL, ESTATE, EOVERFLOW = -22, -71, -75
FIELDS = ("kind", "host", "peer", "flags", "a", "b", "c", "seq", "rng_pos")
SET6 = [3, 63, 64, 65, 127, 199]  # both sides of a wave's and of a shard's boundary, first and last tile
EXT_STEP = 20_000_000


def srt(t):
    return t[np.lexsort((t["seq"], t["host"]))]


def only(t, hosts):
    return t[np.isin(t["host"], np.asarray(hosts, dtype=np.uint32))]


def same_records(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (what, f, got[bad[:3]], want[bad[:3]])


def check_take(recs, spans, hosts=None):
    """A take is sorted by (host, seq), every host's seq consecutive, and its spans tile it in
    ascending host order."""
    assert np.array_equal(spans["first"], np.concatenate([[0], np.cumsum(spans["count"])[:-1]]).astype(np.uint64))
    assert int(spans["count"].sum()) == len(recs) and np.all(spans["count"] > 0)
    assert np.all(np.diff(spans["host"].astype(np.int64)) > 0)
    assert np.array_equal(np.repeat(spans["host"], spans["count"].astype(np.int64)), recs["host"])
    if len(recs) > 1:
        same = recs["host"][1:] == recs["host"][:-1]
        assert np.all(np.diff(recs["seq"].astype(np.int64))[same] == 1)
    if hosts is not None:
        assert set(spans["host"].tolist()) <= set(hosts)


def make(ctxf, args, cap, hosts=None, drain=None, init=True, **kw):
    g, used, hst, cfg, tr = args
    c = ctxf(**kw)
    c.routes_build(g, used)
    c.hosts_set(hst)
    c.trace_enable(cap)
    if hosts is not None:
        c.trace_hosts(hosts)
    if drain:
        c.drain_enable(drain)
    if init:
        c.sim_init(cfg, tr)
    return c


def ref(oracle, args):
    g, used, hosts, cfg, tr = args
    lat, loss = oracle.routes(g, used)
    return oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=True)


# ---- the oracle, once per scenario ----
@pytest.fixture(scope="module")
def periodic(oracle):
    args = scenario()
    o = ref(oracle, args)
    o.run()
    return args, o, srt(o.trace())


@pytest.fixture(scope="module")
def periodic1100(oracle):
    args = scenario(n=1100, V=50, stop_ns=30_000_000)
    o = ref(oracle, args)
    o.run()
    return args, o, srt(o.trace())


@pytest.fixture(scope="module")
def tgen(oracle):
    bw = np.where(np.arange(300) % 10 == 0, 100_000_000, 4_000_000).astype(np.uint64)
    args = scenario(n=300, V=30, kind=sgn.TRAFFIC_TGEN, stop_ns=2_000_000_000, bw=bw, tor=True, tgen_think=200_000_000)
    o = ref(oracle, args)
    o.run()
    t = srt(o.trace())
    per = np.bincount(t["host"], minlength=300)
    servers = np.arange(0, 300, 10)
    clients = np.setdiff1d(np.arange(300), servers)
    server = int(servers[per[servers].argmax()])
    by = clients[np.argsort(per[clients])]
    return args, o, t, {"server": server, "clients": [int(by[-1]), int(by[-2])], "idle": int(by[0]), "per": per}


@pytest.fixture(scope="module")
def external(oracle):
    world = external_world()
    dg = datagrams(world[2])
    o = ref(oracle, world)
    drive_ahead([o], dg, EXT_STEP)
    return world, dg, o, srt(o.trace())


# ---- 1. the host filter ----
def _filter_case(ctxf, args, o, t, hosts, run):
    c = make(ctxf, args, 1 << 22, hosts, drain=(1 << 16) if args[4].kind == sgn.TRAFFIC_EXTERNAL else None)
    run(c)
    want = only(t, hosts)
    assert len(want) > 0
    same_records(srt(c.trace()), want, hosts)
    assert_same_run(o, c, args[2].n, trace=False)
    return c


@pytest.mark.parametrize("hosts", [[0], [199], SET6], ids=["h0", "h199", "six"])
def test_filter_periodic(ctxf, periodic, hosts):
    args, o, t = periodic
    _filter_case(ctxf, args, o, t, hosts, lambda c: c.run())


def test_filter_tgen(ctxf, tgen):
    args, o, t, who = tgen
    hosts = [who["server"]] + who["clients"] + [who["idle"]]
    per = who["per"]
    assert per[who["idle"]] * 10 < per[who["clients"][0]] and per[who["server"]] > 4096, per[hosts]
    _filter_case(ctxf, args, o, t, hosts, lambda c: c.run())


def test_filter_external(ctxf, external):
    world, dg, o, t = external
    hosts = [0, 1, 7, 30]  # (0, 7: slow links; 1: the CPU draws from its RNG between rounds)
    _filter_case(ctxf, world, o, t, hosts, lambda c: drive_ahead([c], dg, EXT_STEP))


# ---- 2. takes over many hosts, in a buffer a third of the trace ----
def test_take_many_hosts(ctxf, periodic1100):
    args, o, t = periodic1100
    n, stop = args[2].n, int(args[3].stop_time_ns)
    runahead = int(args[3].runahead_ns)
    cap = len(t) // 3
    points = [S0 + stop * i // 6 for i in range(1, 7)]
    # the reference alone shows that the capacity suffices: run_until(T) executes whole windows
    # that start below T, and a window is at most one runahead long
    lo = S0
    for T in points:
        held = int(((t["a"] >= lo - runahead) & (t["a"] < T + runahead)).sum())
        assert 0 < held <= cap, (T - S0, held, cap)
        lo = T
    assert len(np.unique(t["host"])) == n > 1024  # (the scan's tile is 1024 hosts)
    c = make(ctxf, args, cap)
    r0, s0 = c.trace_take()
    assert len(r0) == 0 and len(s0) == 0 and c.trace_pending() == 0
    takes = []
    for T in points:
        c.run_until(T)
        pend = c.trace_pending()
        recs, spans = c.trace_take()
        assert len(recs) == pend > 0
        check_take(recs, spans)
        again, sp2 = c.trace_take()  # directly after a take: nothing
        assert len(again) == 0 and len(sp2) == 0
        takes.append(recs)
    assert not c.window()[2]
    same_records(srt(np.concatenate(takes)), t, "takes")
    assert_same_run(o, c, n, trace=False)
    # the same run without takes does not fit that buffer
    d = make(ctxf, args, cap)
    with pytest.raises(sgn.SgnError, match="trace buffer") as e:
        d.run()
    assert e.value.rc == EOVERFLOW


# ---- 3. one hot host ----
def test_take_hot_host(ctxf, tgen):
    args, o, t, who = tgen
    hs, at = np.unique(t["host"], return_index=True)  # (t is sorted by (host, seq): a host's first record)
    first = dict(zip(hs.tolist(), t["a"][at].tolist()))
    servers = set(range(0, 300, 10))
    early = min((h for h in first if h not in servers), key=first.get)
    late = max((h for h in first if h not in servers), key=first.get)
    hosts = sorted([who["server"], early, late])
    c = make(ctxf, args, 1 << 20, hosts)
    bw = c.engine_info()["bucket_width_ns"]
    t_early = first[late] - 2 * bw
    assert first[early] + 2 * bw < t_early, (first[early], first[late], bw)
    c.run_until(t_early)
    r1, s1 = c.trace_take()
    check_take(r1, s1, hosts)
    assert early in s1["host"] and late not in s1["host"]  # a listed host without records yet
    c.run()
    pend = c.trace_pending()
    in_take = int(((t["host"] == who["server"]) & (t["seq"] >= (r1["host"] == who["server"]).sum())).sum())
    assert in_take > 4096
    with pytest.raises(sgn.SgnError) as e:  # too few records: nothing is taken
        c.trace_take(cap=pend - 1)
    assert e.value.rc == sgn.ERANGE and e.value.needed == (pend, 3)
    with pytest.raises(sgn.SgnError) as e:  # too few spans
        c.trace_take(cap=pend, span_cap=2)
    assert e.value.rc == sgn.ERANGE and e.value.needed == (pend, 3)
    assert c.trace_pending() == pend
    r2, s2 = c.trace_take()
    check_take(r2, s2, hosts)
    assert len(r2) == pend and int(s2["count"][s2["host"] == who["server"]][0]) == in_take
    same_records(srt(np.concatenate([r1, r2])), only(t, hosts), "hot")
    assert_same_run(o, c, args[2].n, trace=False)


# ---- 4. snapshots ----
def test_take_rewind(ctxf, periodic):
    """save at round 150, run, take, restore, run, take. The restore sets the records produced
    back to the save's count N and, the take having passed N, the records taken too: the second
    take holds what the re-run produced, the first take's records from N on — the first also held
    the records [0, N) that were pending at the save (read here with trace() before it). Then a
    snapshot saved AFTER a take: a restore keeps the records still pending at its save."""
    args, o, t = periodic
    c = make(ctxf, args, 1 << 20, SET6)
    c.run(150)
    pre = srt(c.trace())
    s0 = c.snapshot_save()
    assert len(pre) > 0 and c.trace_pending() == len(pre)
    c.run(100)
    a, sa = c.trace_take()
    check_take(a, sa, SET6)
    c.snapshot_restore(s0)
    assert c.trace_pending() == 0
    c.run(100)
    b, sb = c.trace_take()
    check_take(b, sb, SET6)
    assert len(b) > 0
    same_records(srt(np.concatenate([pre, b])), a, "rewind")
    # a snapshot saved after a take, with records pending
    c.run(50)
    p1 = srt(c.trace())
    s1 = c.snapshot_save()
    c.run(60)
    assert c.trace_pending() > len(p1) > 0
    c.snapshot_restore(s1)
    assert c.trace_pending() == len(p1)
    same_records(srt(c.trace()), p1, "pending kept")
    c.run()
    d, sd = c.trace_take()
    check_take(d, sd, SET6)
    same_records(srt(np.concatenate([a, d])), only(t, SET6), "all")
    assert_same_run(o, c, args[2].n, trace=False)


def test_take_snapshot_ahead_of_a_moved_cursor(ctxf, periodic, tmp_path):
    """A snapshot saved here keeps no records: the records [cursor, N) it stands for are in the
    buffer. Rewound behind it, they stay in place, and it restores with them pending — until the
    cursor moves: a take after the rewind starts the buffer anew, and what the buffer then holds at
    [cursor, N) is not those records (a restore used to hand them out as pending all the same, an
    export to write them: run-control sweep case 31 ends on such a restore). Both are refused, nothing
    changes; once the run has passed the snapshot's round again the records are there."""
    args, o, t = periodic
    c = make(ctxf, args, 1 << 20, SET6)
    c.run(100)
    n100 = c.trace_pending()
    sa = c.snapshot_save()
    c.run(100)
    n200 = c.trace_pending()
    sb = c.snapshot_save()
    assert n200 > n100 > 0
    c.snapshot_restore(sa)  # rewound, the cursor where it was: b's records are still in place
    assert c.trace_pending() == n100
    c.snapshot_restore(sb)
    assert c.trace_pending() == n200 and c.stats()["rounds"] == 200
    c.snapshot_restore(sa)
    first, sp = c.trace_take()  # the cursor moves to n100: the buffer starts anew
    check_take(first, sp, SET6)
    assert len(first) == n100
    path = tmp_path / "ahead.snap"
    for call in (lambda: c.snapshot_restore(sb), lambda: c.snapshot_export(sb, path)):
        with pytest.raises(sgn.SgnError, match="no longer in the trace buffer") as e:
            call()
        assert e.value.rc == ESTATE
    assert c.stats()["rounds"] == 100 and c.trace_pending() == 0 and not path.exists()
    c.run(150)  # past b's round: its records are produced again
    c.snapshot_restore(sb)
    assert c.stats()["rounds"] == 200 and c.trace_pending() == n200 - n100
    c.snapshot_export(sb, path)
    assert sgn.snapshot_file_info(path)["trace_records"] == n200 - n100
    mid, sm = c.trace_take()
    check_take(mid, sm, SET6)
    c.snapshot_restore(c.snapshot_import(path))  # the file's records [n100, n200) are pending again
    assert c.trace_pending() == n200 - n100
    again, sg = c.trace_take()
    same_records(again, mid, "the file's records")
    c.run()
    rest, sr = c.trace_take()
    check_take(rest, sr, SET6)
    same_records(srt(np.concatenate([first, mid, rest])), only(t, SET6), "every record once")
    assert_same_run(o, c, args[2].n, trace=False)


def _export(c, path):
    s = c.snapshot_save()
    c.snapshot_export(s, path)
    c.snapshot_free(s)
    return sgn.snapshot_file_info(path), {x["name"]: x for x in sgn.snapshot_file_sections(path)}


def test_take_snapshot_file(ctxf, periodic, tmp_path):
    args, o, t = periodic
    n = args[2].n
    t1, t2 = S0 + 100_000_000, S0 + 250_000_000
    c = make(ctxf, args, 1 << 20, SET6)
    c.run_until(t1)
    first, sp = c.trace_take()
    check_take(first, sp, SET6)
    c.run_until(t2)
    pend = c.trace_pending()
    assert len(first) > 0 and pend > 0
    info, secs = _export(c, tmp_path / "taken.snap")
    assert info["trace_records"] == pend and secs["trace"]["bytes"] == pend * 56  # N - b of N records
    # a fresh context with the same host set: the file's records are pending after the restore
    f = make(ctxf, args, 1 << 20, SET6)
    s = f.snapshot_import(tmp_path / "taken.snap")
    f.snapshot_restore(s)
    assert f.trace_pending() == pend
    f.run()
    rest, sr = f.trace_take()
    check_take(rest, sr, SET6)
    same_records(srt(np.concatenate([first, rest])), only(t, SET6), "from b on")
    assert_same_run(o, f, n, trace=False)
    # another host set is another simulation
    other = make(ctxf, args, 1 << 20, [0])
    with pytest.raises(sgn.SgnError, match="identity") as e:
        other.snapshot_import(tmp_path / "taken.snap")
    assert e.value.rc == EINVAL
    # without a take before it the file is the one a library without takes writes: every record
    # [0, N) in the trace section, the header's spare word 0 — and everything but the trace section
    # and that word is the same with and without the take (the record count N stays in ctrl)
    p = make(ctxf, args, 1 << 20, SET6)
    p.run_until(t2)
    total = p.trace_pending()
    assert total == len(first) + pend
    info2, secs2 = _export(p, tmp_path / "plain.snap")
    assert info2["trace_records"] == total and secs2["trace"]["bytes"] == total * 56
    assert info2["identity"] == info["identity"] and info2["rounds"] == info["rounds"]
    # (digests: of the sections whose bytes two runs of one simulation share. CoDel page numbers
    # come from an atomic counter and a slab keeps its runs in arrival order, so hrec / htile — the
    # queues' head and tail pages — the page pool and the packed calendar differ between any two
    # runs, with or without takes; their sizes do not)
    layout = {"hrec", "htile", "codel", "cq_next", "cq_free", "calendar"}
    for name in secs2:
        if name != "trace":
            assert secs2[name]["bytes"] == secs[name]["bytes"], name
            if name not in layout:
                assert secs2[name]["digest"] == secs[name]["digest"], name
    spare = slice(sgn.SNAPSHOT_HEADER_BYTES - 8, sgn.SNAPSHOT_HEADER_BYTES)
    assert int.from_bytes((tmp_path / "plain.snap").read_bytes()[spare], "little") == 0
    assert int.from_bytes((tmp_path / "taken.snap").read_bytes()[spare], "little") == len(first)
    # (its trace section is the records themselves, in the order the buffer holds them)
    raw = np.frombuffer((tmp_path / "plain.snap").read_bytes()[secs2["trace"]["offset"]:][: total * 56], dtype=sgn.TRACE_DTYPE)
    same_records(srt(raw), srt(p.trace()), "plain section")


# ---- 6. two shards on one GPU ----
def test_take_two_shards(ctxf, periodic):
    args, o, t = periodic
    g, used, hosts, cfg, tr = args
    n, stop = hosts.n, int(cfg.stop_time_ns)
    shards = [make(ctxf, args, 1 << 20, SET6, init=False, shard_rank=r, shard_count=2) for r in range(2)]
    arr = (C.c_void_p * 2)(*[c.h.value for c in shards])
    shards[0].check(shards[0].L.sgn_comm_init_local(arr, 2, 1 << 16))
    for c in shards:
        c.sim_init(cfg, tr)
    owned = []
    for r, c in enumerate(shards):
        lo, hi = C.c_uint32(), C.c_uint32()
        c.L.sgn_shard_range(n, r, 2, C.byref(lo), C.byref(hi))
        owned.append([h for h in SET6 if lo.value <= h < hi.value])
    assert all(len(x) >= 2 for x in owned)
    takes = []
    for k in range(1, 5):
        sgn.shards_run_until(shards, S0 + stop * k // 4)
        for r, c in enumerate(shards):
            recs, spans = c.trace_take()
            check_take(recs, spans, owned[r])
            assert len(recs) > 0
            takes.append(recs)
    assert not shards[0].window()[2]
    same_records(srt(np.concatenate(takes)), only(t, SET6), "shards")


# ---- 7. the capture loop ----
def _same_files(got, want):
    assert got.keys() == want.keys()
    for h in want:
        assert got[h][1] == want[h][1] > 0, h
        assert open(got[h][0], "rb").read() == open(want[h][0], "rb").read(), h


def test_run_captured_periodic(ctxf, periodic, tmp_path):
    args, o, t = periodic
    hosts, sizes = [3, 64], [65535, 96]
    names = sgn.host_names(args[2].n)
    want = {}
    for h, s in zip(hosts, sizes):
        want.update(sgn.write_pcaps(t, args[2].ip, tmp_path / "whole", names=names, hosts=[h], capture_len=s))
    c = make(ctxf, args, 1 << 10, hosts)  # (a buffer below the run's records of the two hosts)
    assert len(only(t, hosts)) > 3 * (1 << 10)
    cap = sgn.Capture(tmp_path / "stream", args[2].ip, hosts, sizes, names=names)
    rounds = sgn.run_captured(c, cap, 50_000_000)
    got = cap.close()
    assert rounds == o.stats()["rounds"] and not c.window()[2]
    _same_files(got, want)
    assert got[3][0].endswith(f"hosts/{names[3]}/eth0.pcap")
    assert_same_run(o, c, args[2].n, trace=False)


class _Captured:
    """A Context whose run_until is the capture loop (drive_ahead advances with it)."""

    def __init__(self, c, cap, step_ns):
        self.c, self.cap, self.step_ns = c, cap, step_ns

    def run_until(self, t):
        return sgn.run_captured(self.c, self.cap, self.step_ns, until=t)

    def __getattr__(self, name):
        return getattr(self.c, name)


def test_run_captured_external(ctxf, external, tmp_path):
    world, dg, o, t = external
    hosts = [1, 7]
    names = sgn.host_names(world[2].n)
    want = sgn.write_pcaps(t, world[2].ip, tmp_path / "whole", names=names, hosts=hosts)
    c = make(ctxf, world, 1 << 16, hosts, drain=1 << 16)
    cap = sgn.Capture(tmp_path / "stream", world[2].ip, hosts, names=names)
    drive_ahead([_Captured(c, cap, EXT_STEP // 4)], dg, EXT_STEP)
    cap.feed(*c.trace_take())
    _same_files(cap.close(), want)
    assert_same_run(o, c, world[2].n, trace=False)


# ---- errors ----
def test_trace_hosts_errors(ctxf, periodic):
    args = periodic[0]
    g, used, hosts, cfg, tr = args
    c = ctxf()
    c.routes_build(g, used)
    c.hosts_set(hosts)
    with pytest.raises(sgn.SgnError, match="sgn_trace_enable") as e:  # no trace enabled
        c.trace_hosts([1])
    assert e.value.rc == ESTATE
    c.trace_enable(1 << 16)
    with pytest.raises(sgn.SgnError, match="twice") as e:
        c.trace_hosts([5, 9, 5])
    assert e.value.rc == EINVAL
    c.trace_hosts([5, hosts.n])  # an id past the hosts: refused when the simulation is made
    with pytest.raises(sgn.SgnError, match="not in the simulation") as e:
        c.sim_init(cfg, tr)
    assert e.value.rc == EINVAL
    c.trace_hosts([])  # the set removed: every host is traced
    c.sim_init(cfg, tr)
    with pytest.raises(sgn.SgnError, match="precede") as e:
        c.trace_hosts([1])
    assert e.value.rc == ESTATE
    c.run(20)
    assert len(np.unique(c.trace()["host"])) > 6
    u = ctxf()  # a simulation without a trace: nothing pending, nothing to take
    u.routes_build(g, used)
    u.hosts_set(hosts)
    u.sim_init(cfg, tr)
    assert u.trace_pending() == 0
    with pytest.raises(sgn.SgnError, match="no trace") as e:
        u.trace_take(cap=0)
    assert e.value.rc == ESTATE
