"""CPU-resident applications (SGN_TRAFFIC_EXTERNAL) and the device-held host RNG, on the
oracle alone: the contract's invariants (every submitted datagram's fate is drained exactly
once, with its handle; delivery times respect the routes; window rules), and the RNG
byte/double encodings against rand_core 0.9's fill_bytes_via_next restated in Python."""
import numpy as np
import pytest

import sgn
from external_common import (RUNAHEAD, advance_to, calendar_shape, datagrams, drive, drive_ahead,
                             external_world)


def make_oracle(oracle, world):
    g, used, hosts, cfg, tr = world
    lat, loss = oracle.routes(g, used)
    return oracle.Sim(used, lat, loss, hosts, cfg, tr), lat, loss


def test_every_datagram_fate_drained_once(oracle):
    world = external_world()
    o, lat, _ = make_oracle(oracle, world)
    hosts = world[2]
    dg = datagrams(hosts)
    recs, rounds = drive([o], dg)
    d = recs[0]
    src, dip, pay, t, handle, wire = dg
    # one record per submitted datagram (the simulation ran dry: nothing in flight)
    slots = d["tag"] & 0x1FFFFFFF
    kinds = (d["tag"] >> 29) & 3  # header kind: 0 UDP, 1 TCP, 2 TCP + window scale
    assert np.all(d["tag"] & sgn.TAG_EXT)
    assert len(d) == len(t) and len(np.unique(slots)) == len(t)
    # the handle and the payload travel with the datagram
    order = np.argsort(slots)
    assert np.array_equal(d["handle"][order], handle)
    assert np.array_equal(d["payload_len"][order], pay)
    hdr = np.array([28, 40, 44])[kinds[order]]
    assert np.array_equal(np.where(wire == 0, pay + 28, wire), pay + hdr)
    assert set(np.unique(kinds).tolist()) == {0, 1, 2}
    st = np.bincount(d["status"], minlength=6)
    for s in (sgn.DRAIN_DELIVERED, sgn.DRAIN_LOCAL, sgn.DRAIN_LOSS, sgn.DRAIN_UNKNOWN,
              sgn.DRAIN_BLOCKED):
        assert st[s] > 0, (s, st)
    # a delivery happens no earlier than send time + path latency, at the destination
    ip2h = {int(ip): i for i, ip in enumerate(hosts.ip)}
    node = np.asarray(hosts.node_id)
    dl = d[order]
    for i in range(len(t)):
        r = dl[i]
        if r["status"] == sgn.DRAIN_DELIVERED:
            dh = ip2h[int(dip[i])]
            assert r["host"] == dh and r["src_host"] == src[i]
            assert r["time"] >= t[i] + lat[node[src[i]], node[dh]]
        elif r["status"] == sgn.DRAIN_UNKNOWN:
            assert int(dip[i]) not in ip2h and r["host"] == src[i]
        elif r["status"] == sgn.DRAIN_LOCAL:
            assert int(dip[i]) == int(hosts.ip[src[i]]) and r["time"] >= t[i]
    stt = o.stats()
    assert stt["app_blocked"] == st[sgn.DRAIN_BLOCKED]
    assert stt["packets_loss_dropped"] == st[sgn.DRAIN_LOSS]
    assert stt["delivered"] == st[sgn.DRAIN_DELIVERED]


def test_drain_filters_by_host_and_keeps_the_rest(oracle):
    world = external_world(n=20, V=8)
    o, _, _ = make_oracle(oracle, world)
    hosts = world[2]
    dg = datagrams(hosts, k=80, span_ns=20_000_000)
    recs, _ = drive([o], dg)
    d = recs[0]
    # drive() drained [0,30) then [30,..) every 5 rounds: the union is all records, each
    # slice ordered by (host, time, src, src eid, tag, status)
    assert len(d) == 80
    assert o.drain().size == 0


def test_set_window_rules(oracle):
    world = external_world(n=10, V=5)
    o, _, _ = make_oracle(oracle, world)
    S = sgn.SIMULATION_START
    o.round()  # [S, S+1): nothing to do; the simulation has no events
    assert o.window()[2] is False
    with pytest.raises(sgn.SgnError):
        o.set_window(S, S)  # empty
    o.set_window(S + 5_000_000, S + 5_000_000 + RUNAHEAD)
    with pytest.raises(sgn.SgnError):  # before the window start
        o.submit([0], [world[2].ip[1]], [100], [S + 4_000_000])
    o.submit([0], [world[2].ip[1]], [100], [S + 5_500_000])
    o.round()
    ws, we, active = o.window()
    assert active and ws > S + 5_500_000
    with pytest.raises(sgn.SgnError):  # after the next event
        o.set_window(ws + 1, ws + 2)
    with pytest.raises(sgn.SgnError):  # before the last window's end
        o.set_window(S + 5_000_000, S + 5_000_001)


def _fill_bytes_py(next_u64, n):
    out = bytearray()
    while n - len(out) >= 8:
        out += next_u64().to_bytes(8, "little")
    r = n - len(out)
    if r > 4:
        out += next_u64().to_bytes(8, "little")[:r]
    elif r > 0:
        out += (next_u64() >> 32).to_bytes(4, "little")[:r]
    return bytes(out)


@pytest.mark.parametrize("nbytes", [0, 1, 3, 4, 5, 7, 8, 9, 12, 13, 16, 31])
def test_host_rng_fill_bytes_and_double(oracle, nbytes):
    world = external_world(n=4, V=3)
    o, _, _ = make_oracle(oracle, world)
    L = oracle.load()
    st = np.zeros(4, dtype=np.uint64)
    L.ora_xoshiro_seed_from_u64(int(world[2].seed[2]), sgn.ptr(st, sgn.C.c_uint64))

    def nxt():
        return int(L.ora_xoshiro_next_u64(sgn.ptr(st, sgn.C.c_uint64)))

    assert o.rng_fill_bytes(2, nbytes) == _fill_bytes_py(nxt, nbytes)
    x = nxt()
    assert o.rng_double(2) == (x >> 11) * 2.0 ** -53
    assert o.rng_next_u64(2) == nxt()


def test_tcp_segments_take_their_wire_length_through_token_buckets(oracle):
    """Packet::len (network/packet.rs:388-390, :617-635): a TCP segment is payload + 40 B on
    the wire (+ 44 with window scale) and the relays' token buckets charge that length, so the
    same payloads drain later from a slow link as TCP than as UDP."""
    finish = {}
    for hdr in (28, 44):
        world = external_world(n=4, V=3, bw=400_000, fifo=1000, stop_ns=3_000_000_000)
        o, _, _ = make_oracle(oracle, world)
        ip = world[2].ip
        k = 60
        t = sgn.SIMULATION_START + 1_000_000 + np.arange(k, dtype=np.uint64)
        o.submit(np.zeros(k), np.full(k, ip[1]), np.full(k, 500), t, wire_len=np.full(k, 500 + hdr))
        while o.window()[2]:
            o.round()
        d = o.drain()
        assert len(d) == k and np.all(d["status"] == sgn.DRAIN_DELIVERED)
        finish[hdr] = int(d["time"].max())
    assert finish[44] > finish[28]
    with pytest.raises(sgn.SgnError):
        o.submit([0], [ip[1]], [500], [o.window()[0]], wire_len=[530])


# ---- the submit-ahead driver (external_common.drive_ahead) on the oracle alone ----
_DRIVE_REF = {}


def _canon(d):
    return np.sort(d, order=list(sgn.DRAIN_DTYPE.names))


def _idle_rng_case(oracle):
    """The default world and datagrams() without the sends of hosts 58 and 59: the two drivers
    make their CPU-side RNG draws at different moments, and a draw from a host that also sends
    would move that host's loss draws; these two hosts only receive."""
    if not _DRIVE_REF:
        world = external_world()
        dg = datagrams(world[2], k=640)
        keep = ~np.isin(dg[0], (58, 59))
        dg = tuple(a[keep] for a in dg)
        o, lat, _ = make_oracle(oracle, world)
        (d,), rounds = drive([o], dg, rng_hosts=(58, 59))
        _DRIVE_REF.update(world=world, dg=dg, lat=lat, recs=_canon(d), rounds=rounds, stats=o.stats(),
                          window=o.window(), digests=o.digests())
    return _DRIVE_REF


@pytest.mark.parametrize("step_ms", [1, 7, 50])
def test_drive_ahead_yields_the_records_of_drive(oracle, step_ms):
    """Submitting ahead changes no window and no fate: the same drain records, counters, window
    and digests as drive(), which submits a window at a time and steps with round(). (The RNG
    state of the two hosts the drivers draw from is left out: they draw different amounts.)"""
    ref = _idle_rng_case(oracle)
    world, dg = ref["world"], ref["dg"]
    o, lat, _ = make_oracle(oracle, world)
    log = {}
    (d,), rounds = drive_ahead([o], dg, step_ms * 1_000_000, rng_hosts=(58, 59),
                               calendar=calendar_shape(lat, world[3]), log=log)
    assert rounds == ref["rounds"] and len(d) == len(dg[3]) > 600
    assert np.array_equal(_canon(d), ref["recs"])
    assert o.stats() == ref["stats"] and o.window() == ref["window"]
    d0, d1 = ref["digests"], o.digests()
    for f in d0.dtype.names:
        sel = np.arange(len(d0)) < 58 if f == "rng" else slice(None)
        assert np.array_equal(d0[f][sel], d1[f][sel]), f
    assert len(log["draws"][0]) > 0 and max(log["rounds_per_step"]) > 1


def _gpu_case_names():
    import test_gpu_external as gx
    named = ["default", "long", "fan-in", "codel", "round-robin", "dynamic", "gaps", "horizon"]
    return named + [f"sweep-{i}" for i in range(gx.N_SWEEP)]


@pytest.mark.parametrize("name", _gpu_case_names())
def test_gpu_cases_on_the_oracle(oracle, name):
    """Every world of tests/test_gpu_external.py under drive_ahead on the oracle: one record per
    datagram with its handle, the statuses the GPU test asserts, a calendar short enough for
    persistent rounds (256 buckets) and every submit below its horizon."""
    import test_gpu_external as gx
    case = gx.build_case(oracle, name)
    world, dg = case["world"], case["dg"]
    cal = calendar_shape(case["lat"], world[3])
    assert cal[0] <= 256, cal
    steps = gx.STEPS if name == "default" else (case["kw"]["step_ns"],)
    for step in steps:
        o, _, _ = make_oracle(oracle, world)
        log = {}
        (d,), rounds = drive_ahead([o], dg, calendar=cal, log=log, **dict(case["kw"], step_ns=step))
        slots = d["tag"] & 0x1FFFFFFF
        assert len(d) == len(dg[3]) and len(np.unique(slots)) == len(d) and rounds > 20
        order = np.argsort(slots)
        assert np.array_equal(d["handle"][order], dg[4]) and np.array_equal(d["payload_len"][order], dg[2])
        st = np.bincount(d["status"], minlength=6)
        for s in case["expect"]:
            assert st[s] > 0, (name, s, st)
        assert max(log["rounds_per_step"]) > 1, (name, step)
    if name == "long":
        assert log["rounds_per_step"][0] > 128  # (and sgn_run(ctx, 29) at least four times)
        assert int(dg[3][-1]) < sgn.SIMULATION_START + (cal[0] - 2) * cal[1]
    if name == "horizon":
        assert int(dg[3][-1]) == sgn.SIMULATION_START + (cal[0] - 2) * cal[1] - 1 and log["rounds_per_step"][0] > 64
    if name == "gaps":
        gaps = np.diff(dg[3].astype(np.int64))
        assert np.sum(gaps > cal[0] * cal[1]) == 3 and log["k"] > 20  # idle for longer than the calendar's span
    if name == "fan-in":
        hot = d[(d["host"] == 50) & (d["status"] == sgn.DRAIN_DELIVERED)]
        per_bucket = np.bincount(((hot["time"] - sgn.SIMULATION_START) // cal[1]).astype(np.int64))
        assert np.sum(per_bucket >= 33) >= 3, per_bucket  # three bursts, each inside one bucket
        assert st[sgn.DRAIN_DELIVERED] > 3 * 33
    if name == "codel":
        assert st[sgn.DRAIN_CODEL] > 0 and o.stats()["codel_dropped"] == st[sgn.DRAIN_CODEL]
        assert o.stats()["max_codel_len"] > 124 * 16 // 9  # the nine slow hosts' queues: pages beyond the first 124
    if name == "dynamic":
        assert o.stats()["min_used_latency_ns"] != sgn.EMUTIME_INVALID
        assert world[3].use_dynamic_runahead == 1


@pytest.mark.parametrize("which", ["shards", "fan-in-x"])
def test_sharded_gpu_cases_on_the_oracle(oracle, which):
    """The datagram sets the shard-group tests submit before the first round: all below the
    horizon at t = 0, an unambiguous ordering key, every claimed status, and (fan-in) three bursts
    of more than 32 deliveries to host 71 inside one bucket each, all from hosts of shard 0."""
    import test_gpu_external as gx
    case = gx.shard_case(oracle) if which == "shards" else gx.fan_in_shards_case(oracle)
    world, dg = case["world"], case["dg"]
    cal = calendar_shape(case["lat"], world[3])
    assert cal[0] <= 256 and int(dg[3][-1]) < sgn.SIMULATION_START + (cal[0] - 2) * cal[1]
    assert len(np.unique(dg[3])) == len(dg[3]) and len(np.unique(dg[4])) == len(dg[4]) and np.all(dg[4] != 0)
    o, _, _ = make_oracle(oracle, world)
    o.submit(dg[0], dg[1], dg[2], dg[3], dg[4], wire_len=dg[5])
    if which == "shards":
        T = sgn.SIMULATION_START + 40_000_000
        assert advance_to(o, T) > 10
        ws = o.window()[0]
        assert ws <= int(dg[3][dg[3] >= T + RUNAHEAD][0])  # the second half is still ahead of the window
    assert o.run() > 50
    d = gx.by_key(o.drain())
    assert len(d) == len(dg[3])
    st = np.bincount(d["status"], minlength=6)
    for s in case["expect"]:
        assert st[s] > 0, (s, st)
    n = world[2].n
    half = d["src_host"] < n // 2
    assert (half != (d["host"] < n // 2)).any()  # fates drained on a shard that did not submit them
    if which == "fan-in-x":
        hot = d[(d["host"] == 71) & (d["status"] == sgn.DRAIN_DELIVERED)]
        assert np.all(hot["src_host"][hot["payload_len"] == 100] < 50)
        per_bucket = np.bincount(((hot["time"] - sgn.SIMULATION_START) // cal[1]).astype(np.int64))
        assert np.sum(per_bucket >= 33) >= 3, per_bucket


def test_drain_overflow_case_on_the_oracle(oracle):
    """The twenty datagrams of test_drain_buffer_exhaustion_is_a_status: twenty fates in the
    window after the first, empty one."""
    world = external_world(n=10, V=5)
    o, _, _ = make_oracle(oracle, world)
    k = 20
    t = sgn.SIMULATION_START + 1000 * (1 + np.arange(k, dtype=np.uint64))
    o.submit(np.arange(k) % 10, np.full(k, 0x0AFF0001), np.full(k, 100), t)
    o.round()  # [S, S + 1)
    assert o.window() == (int(t[0]), int(t[0]) + RUNAHEAD, True) and len(o.drain()) == 0
    o.round()
    d = o.drain()
    assert len(d) == k and np.all(d["status"] == sgn.DRAIN_UNKNOWN)


def test_burst_controller_on_the_oracle(oracle):
    """test_shards_set_window_over_idle_gaps' controller on the oracle alone: four bursts, the
    window moved to each burst's first send, every burst below the horizon of its window, every
    fate drained."""
    import test_gpu_external as gx
    case = gx.build_case(oracle, "gaps")
    cal = calendar_shape(case["lat"], case["world"][3])
    o, _, _ = make_oracle(oracle, case["world"])
    rounds = gx.run_bursts(o, [], None, [], case["dg"], (cal[0] - 2) * cal[1])
    assert len(rounds) == 4 and min(rounds) > 20
    d = o.drain()
    st = np.bincount(d["status"], minlength=6)
    assert len(d) == len(case["dg"][3]) and all(st[s] > 0 for s in case["expect"])
    low = d["src_host"] < 30  # (senders on both shards of two, and fates that cross)
    assert low.any() and (~low).any() and (low != (d["host"] < 30)).any()
