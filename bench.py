"""Headline benchmark: simulated packet events/s (whole node) at 100k hosts + APSP build time.

Workload (BASELINE.json configs[2], "config C", the one the metric is quoted on: it fits a
single MI355X): 100k synthetic hosts per GPU on a Tor-like 1000-node complete graph
(latency 1 ms + 5..150 ms distance term, loss 0..0.5 %), Zipf(1.0) host placement,
bandwidth classes 10M/100M/1G, 10 % servers; clients fetch 50 KiB / 1 MiB / 5 MiB files as
1500 B UDP trains paced only by token buckets and CoDel (no TCP congestion control: the
TCP stack is outside the GPU core). Synthetic data, seeded.

A step = ROUNDS_PER_STEP simulation rounds (Shadow scheduling windows). A packet event =
one send_packet call past the DNS check (sent or loss-dropped) or one packet event popped
at its destination. value = all ranks' packet events / max-rank wall time.

Launch: python bench.py [--gpus N --steps K --warmup W] [--full] [--dump-outputs DIR]; a plain
run sets up, warms up, times the K steps and prints the result line; --full adds the CPU
baselines and the parity checks (main's --help). For N > 1 under
torch.distributed.run (one rank per GPU, hosts sharded, RCCL exchange inside libsgn).
Scaling is STRONG by default: the workload's hosts (C: 100k) are sharded over the N GPUs,
as BASELINE.json names config C ("100k synthetic hosts ... sharded over 8 GPUs");
--weak gives every GPU --hosts hosts instead.
"""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT / "shadow-gen_amd"))
import sgn  # noqa: E402

METRIC = "simulated packet events/sec (whole node) at 100k hosts; APSP build time"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md chip table (spec)
L2_PEAK_GBS = 34500.0  # MI355X_MICROARCH.md L2 section: 4 MiB per XCD, ~34.5 TB/s aggregate
# 32-bit integer VALU (min / add have no packed form): 256 CUs x 64 lanes per clock x 2.4 GHz
# (MI355X_MICROARCH.md: the 157.3 TF f32 vector peak counts packed FMA, 2 lanes x 2 flops)
VALU_PEAK_TOPS = 39.3


def build_workload(n_hosts, V, seed=1):
    g = sgn.tor_graph(V, seed=42)
    used = np.arange(V, dtype=np.uint32)
    names = sgn.host_names(n_hosts)
    seeds = sgn.derive_seeds(seed, names)
    node = sgn.zipf_nodes(n_hosts, V, seed=5)
    bw = sgn.bandwidth_classes(n_hosts, seed=3)
    hosts = sgn.HostArrays(sgn.assign_ips(n_hosts), node, bw, bw, seeds)
    rng = np.random.default_rng(11)
    servers = np.sort(rng.choice(n_hosts, size=max(1, n_hosts // 10), replace=False)).astype(np.uint32)
    if os.environ.get("SGN_BENCH_SORTED"):  # experiment: hosts of one kind in consecutive HostIds
        ns = len(servers)
        servers = np.arange(ns, dtype=np.uint32)
        bw = np.concatenate([np.sort(bw[:ns]), np.sort(bw[ns:])])
        hosts = sgn.HostArrays(hosts.ip, hosts.node_id, bw, bw, hosts.seed)
    # first fetch uniform over one mean think time: the fetch process is stationary from t=0
    tr = sgn.make_traffic(sgn.TRAFFIC_TGEN, flow_seed=7, start_ns=0, start_jitter_ns=3_000_000_000,
                          period_ns=2_000_000_000, period_jitter_ns=2_000_000_000,
                          req_payload=64, servers=servers,
                          file_bytes=(50 * 1024, 1024 * 1024, 5 * 1024 * 1024))
    cfg = sgn.make_config(3600 * 1_000_000_000, runahead_ns=1_000_000, out_fifo_cap=64,
                          codel_cap=64, event_capacity=1 << 24)
    return g, used, hosts, cfg, tr


def build_workload_b(n_hosts, V, seed=1):
    """Config B (BASELINE.json configs[1]): 10k hosts on a 1000-node random graph (mean degree
    6, 20 % lossy edges), every host sends 1024 B UDP every 10 ms to a seeded random peer
    (1 permille to addresses outside the simulation), 100 Mbit, 10 simulated seconds."""
    g = sgn.random_graph(V, seed=42)
    used = np.arange(V, dtype=np.uint32)
    seeds = sgn.derive_seeds(seed, sgn.host_names(n_hosts))
    bw = np.full(n_hosts, 100_000_000, dtype=np.uint64)
    hosts = sgn.HostArrays(sgn.assign_ips(n_hosts), (np.arange(n_hosts) % V).astype(np.uint32), bw, bw, seeds)
    tr = sgn.make_traffic(sgn.TRAFFIC_PERIODIC, flow_seed=7, period_ns=10_000_000,
                          start_jitter_ns=10_000_000, payload_len=1024, unknown_dst_permille=1)
    cfg = sgn.make_config(10_000_000_000, runahead_ns=1_000_000, out_fifo_cap=64, codel_cap=64,
                          event_capacity=1 << 22)
    # 16 hosts per execute wave: B's 10k hosts are 157 waves at 64, one per CU on 157 of the
    # 256 CUs; 625 waves of 16 spread the (per-lane serial) host work (same-box A/B: 2827 ->
    # 2770 us per 100-round launch; 8 and 4 hosts per wave were slower). A performance knob:
    # results do not depend on it (tests/test_gpu_fuzz.py mixes it).
    cfg.hosts_per_wave = 16
    return g, used, hosts, cfg, tr


def build_workload_d(n_hosts, V, seed=1, stop_ns=1_000_000_000):
    """Config D (BASELINE.json configs[3]): the config-B graph (1000-node random GML, mean
    degree 6, 20 % lossy edges, 100 Mbit), every host sends a 64 B datagram to a uniform
    random peer every 1 ms (dense all-to-all). The bench sets stop_ns so that every timed
    step has its full rounds (1 ms each)."""
    g = sgn.random_graph(V, seed=42)
    used = np.arange(V, dtype=np.uint32)
    seeds = sgn.derive_seeds(seed, sgn.host_names(n_hosts))
    bw = np.full(n_hosts, 100_000_000, dtype=np.uint64)
    hosts = sgn.HostArrays(sgn.assign_ips(n_hosts), (np.arange(n_hosts) % V).astype(np.uint32), bw, bw, seeds)
    tr = sgn.make_traffic(sgn.TRAFFIC_PERIODIC, flow_seed=7, start_ns=0, start_jitter_ns=1_000_000,
                          period_ns=1_000_000, payload_len=64, unknown_dst_permille=0)
    cfg = sgn.make_config(stop_ns, runahead_ns=1_000_000, out_fifo_cap=16, codel_cap=64,
                          event_capacity=0)
    return g, used, hosts, cfg, tr


def build_workload_h(n_hosts, V, seed=1):
    """Hot-spot fan-in (a test workload, not a BASELINE config): 8 TGEN servers (the first
    HostIds: shard 0) and every other host a client that first fetches a one-packet
    file from one of them at the same instant, then every ~50 ms. Thousands of request runs land
    in the servers' (bucket, host group) slabs each round — the fan-in the reference's unbounded
    per-host EventQueue takes (core/work/event_queue.rs:12,57-66) — and with N > 1 most of them
    arrive through the round exchange (k_import)."""
    g = sgn.tor_graph(V, seed=42)
    used = np.arange(V, dtype=np.uint32)
    seeds = sgn.derive_seeds(seed, sgn.host_names(n_hosts))
    bw = np.full(n_hosts, 1_000_000_000, dtype=np.uint64)
    hosts = sgn.HostArrays(sgn.assign_ips(n_hosts), (np.arange(n_hosts) % V).astype(np.uint32), bw, bw, seeds)
    servers = np.arange(8, dtype=np.uint32)
    tr = sgn.make_traffic(sgn.TRAFFIC_TGEN, flow_seed=7, start_ns=0, start_jitter_ns=0,
                          period_ns=50_000_000, period_jitter_ns=50_000_000, req_payload=64,
                          servers=servers, file_bytes=(1000, 1400, 1400))
    cfg = sgn.make_config(3600 * 1_000_000_000, runahead_ns=1_000_000, out_fifo_cap=64,
                          codel_cap=64, event_capacity=1 << 22)
    return g, used, hosts, cfg, tr


def events_of(st):
    return st["packets_sent"] + st["packets_loss_dropped"] + st["packet_events_popped"]


def cpu_share():
    """Host cores this process may use: the cgroup CPU quota when one is set (the GPU box
    grants a share of a larger machine), else the affinity mask; plus what the OS shows."""
    visible = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    share = visible
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            share = max(1, min(visible, -(-int(q) // int(per))))
    except (OSError, ValueError):
        pass
    if os.environ.get("OMP_NUM_THREADS", "").isdigit():  # the box pins pools to its share
        share = max(1, min(share, int(os.environ["OMP_NUM_THREADS"])))
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return share, visible, model


STAT_KEYS = ("rounds", "packets_sent", "packets_loss_dropped", "packets_unknown_dst", "packet_events_popped",
             "codel_dropped", "delivered", "local_delivered", "app_blocked", "local_events", "bytes_delivered",
             "min_used_latency_ns", "max_codel_len", "host_executions")
DIGEST_KEYS = ("tx", "rx", "app", "rng", "next_event_id", "n_sent", "n_popped", "n_delivered", "n_codel_dropped")


def shard_check(ctx, dist, rank, world, n_hosts, rounds_done, build_unsharded):
    """N > 1: the sharded run (RCCL exchange) against ONE unsharded run of all N x hosts on
    rank 0's GPU for the same rounds (build_unsharded() -> a context after sim_init) — bit for
    bit: every host's digests, the summed counters, the window. (The unsharded path is the one
    checked against the oracle at N = 1.) Collective over gloo; frees the shard's context
    first. Returns rank 0's verdict dict (None on other ranks)."""
    import torch
    lo, hi = sgn.C.c_uint32(), sgn.C.c_uint32()
    rc = sgn.load().sgn_shard_range(n_hosts, rank, world, sgn.C.byref(lo), sgn.C.byref(hi))
    assert rc == 0
    lo, hi = lo.value, hi.value
    d = ctx.digests(lo, hi)
    st = ctx.stats()
    ws, we, act = ctx.window()
    if hasattr(ctx, "close"):
        ctx.close()
    width = sgn.DIGEST_DTYPE.itemsize // 8
    per = -(-n_hosts // world) + 1
    buf = np.zeros((per, width), dtype=np.uint64)
    buf[: hi - lo] = d.view(np.uint64).reshape(-1, width)
    meta = np.array([lo, hi, ws, we, int(act)] + [st[k] for k in STAT_KEYS], dtype=np.uint64)
    tb, tm = torch.from_numpy(buf.view(np.int64)), torch.from_numpy(meta.view(np.int64))
    gb = [torch.zeros_like(tb) for _ in range(world)] if rank == 0 else None
    gm = [torch.zeros_like(tm) for _ in range(world)] if rank == 0 else None
    dist.gather(tb, gb, dst=0)
    dist.gather(tm, gm, dst=0)
    out = None
    if rank == 0:
        c1 = build_unsharded()
        assert c1.run(rounds_done) == rounds_done
        so = c1.stats()
        d1 = c1.digests(0, n_hosts).view(np.uint64).reshape(-1, width)
        w1 = c1.window()
        if hasattr(c1, "close"):
            c1.close()
        mism = []
        metas = [m.numpy().view(np.uint64) for m in gm]
        for r in range(world):
            a, b = int(metas[r][0]), int(metas[r][1])
            got = gb[r].numpy().view(np.uint64)[: b - a]
            bad = np.nonzero((got != d1[a:b]).any(axis=1))[0]
            if len(bad):
                mism.append(f"rank {r}: {len(bad)} host digests differ (first HostId {a + int(bad[0])})")
            if tuple(int(x) for x in metas[r][2:5]) != (w1[0], w1[1], int(w1[2])):
                mism.append(f"rank {r}: window {metas[r][2:5].tolist()} vs {list(w1)}")
        add_keys = [k for k in STAT_KEYS if k not in ("rounds", "min_used_latency_ns", "max_codel_len")]
        for i, k in enumerate(STAT_KEYS):
            vals = [int(m[5 + i]) for m in metas]
            want = so[k]
            got = sum(vals) if k in add_keys else (min(vals) if k == "min_used_latency_ns" else max(vals))
            if got != want:
                mism.append(f"{k}: shards {got} vs unsharded {want}")
        out = {"ok": not mism, "mismatches": mism[:10], "rounds_compared": int(rounds_done),
               "hosts_compared": int(n_hosts),
               "reference": "one unsharded libsgn run of all hosts on rank 0's GPU (the path checked "
                            "against the oracle at N=1)"}
    dist.barrier()
    return out


DUMP_MAX_BYTES = 48 << 20  # --dump-outputs: the files of all ranks together stay below this
HASH_FIELDS = ("tx", "rx", "app", "rng")  # 64-bit hashes: no float64 holds one, so two halves


def _f64(a, split):
    """u64 values as float64, exactly: hashes as (high 32 bits, low 32 bits) in a trailing
    axis of 2, counters and times (below 2^53) as they are."""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if split:
        return np.stack([a >> np.uint64(32), a & np.uint64(0xFFFFFFFF)], axis=-1).astype(np.float64)
    assert not len(a) or int(a.max()) < 1 << 53
    return a.astype(np.float64)


def dump_outputs(path, ctx, n_hosts, rank, world):
    """--dump-outputs: what a caller of the timed path (ctx.run) holds after the last timed
    step, as DIR/<name>.npy in float64: `stats` (the counters, STAT_KEYS order), `window`
    (start ns, end ns, active), both as high and low 32-bit halves, and per host of this
    rank's shard `digest_<field>` (DIGEST_KEYS; the hashes tx/rx/app/rng as halves, the
    counters as they are) with `host_ids` naming the rows. A shard whose digests would pass
    its share of DUMP_MAX_BYTES (1 / N of it, so all ranks together stay below 64 MB) writes
    a fixed seeded sample of its hosts. The workload is seeded and the engine bit-reproducible,
    so two builds given the same arguments can be compared file for file. With N > 1 every
    rank writes its shard as <name>.rank<r>.npy."""
    d = pathlib.Path(path)
    d.mkdir(parents=True, exist_ok=True)
    sfx = f".rank{rank}" if world > 1 else ""
    lo, hi = sgn.C.c_uint32(0), sgn.C.c_uint32(n_hosts)
    if world > 1:
        assert sgn.load().sgn_shard_range(n_hosts, rank, world, sgn.C.byref(lo), sgn.C.byref(hi)) == 0
    lo, hi = lo.value, hi.value
    st = ctx.stats()
    ws, we, act = ctx.window()
    dg = ctx.digests(lo, hi)
    rows = np.arange(hi - lo)
    keep = DUMP_MAX_BYTES // world // (2 * sgn.DIGEST_DTYPE.itemsize + 8)
    if len(rows) > keep:
        rows = np.sort(np.random.default_rng(20240).choice(len(rows), size=keep, replace=False))
    arrays = {"stats": _f64([st[k] for k in STAT_KEYS], True),
              "window": _f64([ws, we, int(act)], True),
              "host_ids": _f64(rows + lo, False)}
    for f in DIGEST_KEYS:
        arrays[f"digest_{f}"] = _f64(dg[f][rows], f in HASH_FIELDS)
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    for name, a in arrays.items():
        np.save(d / f"{name}{sfx}.npy", a)


def cpu_baseline(g, used, hosts, cfg, tr, args, gpu):
    """The CPU restatement of the reference's hot path (oracle/, a C++ port: the Rust
    reference cannot be built here), timed on this box's host cores, and the parity check of
    the GPU run.

    1. Parity: the oracle (CPU-optimised data structures, all cores) runs the same workload
       through exactly the rounds the GPU ran (warm-up untimed, then the GPU's timed rounds,
       timed); its stats, final window and every host's digests must equal the GPU's.
    2. Then, on the next rounds of the same simulation, each of {reference-faithful,
       CPU-optimised} x {all cores, 1 core} for a bounded sample (SURVEY.md §8(d),
       BASELINE.md). Faithful = the reference's hash-map lookups per packet, the global
       packet-counter write lock (worker.rs:379, graph/mod.rs:450-458), heap packet copies
       and a lock per queue operation; a persistent worker pool with a rendezvous per round
       either way.
    3. APSP: compute_shortest_paths restated both ways, at all cores (rayon) and 1 core."""
    sys.path.insert(0, str(ROOT / "oracle"))
    import oracle_py

    cores, visible, model = cpu_share()
    last = [time.perf_counter()]

    def progress(msg):  # long CPU phases keep writing (a silent GPU-box command is taken as hung)
        if time.perf_counter() - last[0] > 15:
            print(f"bench: cpu baseline: {msg}", file=sys.stderr, flush=True)
            last[0] = time.perf_counter()

    def run_rounds(sim, n, what):
        done = 0
        while done < n:
            k = sim.run(min(25, n - done))
            done += k
            progress(f"{what} {done}/{n} rounds")
            if k == 0:
                break
        return done

    apsp = {}
    for faithful in (True, False):
        for th in (cores, 1):
            t0 = time.perf_counter()
            lat, loss = oracle_py.routes(g, used, faithful=faithful, threads=th)
            apsp[f"{'faithful' if faithful else 'optimised'}_{th}c_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            progress(f"APSP faithful={faithful} threads={th}")
    sim = oracle_py.Sim(used, lat, loss, hosts, cfg, tr, threads=cores)
    warm = args.warmup * args.rounds_per_step
    assert run_rounds(sim, warm, "parity warm-up") == warm
    st0 = sim.stats()
    t0 = time.perf_counter()
    timed_rounds = run_rounds(sim, gpu["rounds_timed"], "parity replay of the timed rounds")
    el = time.perf_counter() - t0
    ev = events_of(sim.stats()) - events_of(st0)
    # parity with the GPU run: same rounds, same counters, same window, same digests
    so = sim.stats()
    mism = [k for k in STAT_KEYS if so[k] != gpu["stats"][k]]
    if sim.window() != gpu["window"]:
        mism.append("window")
    do = sim.digests(0, hosts.n)
    for f in DIGEST_KEYS:
        bad = np.nonzero(do[f] != gpu["digests"][f])[0] if do[f].ndim == 1 else \
            np.nonzero((do[f] != gpu["digests"][f]).any(1))[0]
        if len(bad):
            mism.append(f"digest {f}: {len(bad)} hosts (first {bad[:3].tolist()})")
    parity = {"ok": not mism and timed_rounds == gpu["rounds_timed"], "mismatches": mism[:8],
              "rounds_compared": warm + timed_rounds, "hosts_compared": int(hosts.n),
              "fields": list(STAT_KEYS) + ["window"] + [f"digest.{f}" for f in DIGEST_KEYS]}
    modes = {"optimised_all": {"value": ev / el, "cores": cores, "rounds": timed_rounds, "events": ev,
                               "wall_s": round(el, 2), "sample": "the GPU's timed rounds"}}

    def sample(name, faithful, th, budget):
        sim.set_faithful(faithful)
        sim.set_threads(th)
        s0 = events_of(sim.stats())
        t1 = time.perf_counter()
        r = 0
        # (rounds per call: config D's 1M hosts take ~1 s a round in the single-core faithful
        # mode, so its samples step 2 rounds at a time to stay near the budget)
        step = 20 if hosts.n <= 200_000 else 2
        while time.perf_counter() - t1 < budget and sim.window()[2]:
            r += sim.run(step)
            progress(f"{name} sample")
        e1 = time.perf_counter() - t1
        e = events_of(sim.stats()) - s0
        modes[name] = {"value": e / e1, "cores": th, "rounds": r, "events": e, "wall_s": round(e1, 2),
                       "sample": "the next rounds of the same simulation"}

    b = args.cpu_budget_s
    sample("faithful_all", True, cores, b / 4)
    sample("faithful_1", True, 1, b / 4)
    sample("optimised_1", False, 1, b / 4)
    # the headline is the stronger CPU baseline: the CPU-optimised restatement on every core of
    # the box's share (the faithful mode keeps the reference's global packet-counter lock,
    # which serialises it; it is reported in `modes`)
    o, f = modes["optimised_all"], modes["faithful_all"]
    return {
        "value": o["value"],
        "unit": "packet events/s",
        "cores": cores,
        "kind": "port",
        "sample": f"CPU-optimised C++ restatement (oracle/) of the round loop on {cores} worker threads over "
                  f"exactly the GPU's {o['rounds']} timed rounds of the same {hosts.n}-host workload "
                  f"({o['events']} packet events, {o['wall_s']} s); the reference-faithful restatement "
                  f"(global packet-counter lock, hash-map lookups) reached {f['value'] / 1e6:.2f} M/s on "
                  f"{f['rounds']} later rounds",
        "cpu_model": model, "cpus_visible": visible,
        "modes": {k: {kk: (round(vv, 1) if isinstance(vv, float) else vv) for kk, vv in m.items()}
                  for k, m in modes.items()},
        "apsp_ms": apsp,
        "apsp_sample": "compute_shortest_paths restated (per-source Dijkstra over the same graph): "
                       "faithful = hash-map scores, O(U) contains filter, hashed U^2 output + to_ids "
                       "re-collect; optimised = dense arrays; sources over N threads like rayon",
    }, parity


def apsp_roofline(apsp, V, U):
    """SURVEY.md §8(d) per phase, algorithmic bytes of the form that ran:
    latency — u64 blocked Floyd-Warshall: the V x V u64 matrix read+written per k-block,
    16 V^3 / T; u32 min-plus squaring: per pass every T x T tile reads its row and column
    panels, 8 V^3 / T; per-source relaxation (sparse graphs): every sweep reads the arc list
    (12 B per arc) for every used source, 12 U E sweeps.
    loss — multi-source sweep (kS sources per arc load): 8 B per arc per source group plus
    the rows, 8 E ceil(U / kS) + 4 U V; its dense form (loss_dense: a lane per head, the tails'
    negated latencies from a V x V matrix, kS sources per workgroup): 4 B per (tail, head) per
    source group plus the rows, 4 V^2 ceil(U / kS) + 4 U V; one-source pass: 12 B per arc per
    source, 12 U E.
    The arc list is re-read from L2 / MALL, so these are traffic above HBM, not HBM bytes."""
    T = apsp["tile"] or 64
    E = apsp["n_tight_edges"]
    if apsp.get("latency_bf"):
        b_lat = 12.0 * U * E * max(1, apsp["latency_passes"])
    elif apsp.get("latency_u64", 1):
        b_lat = 16.0 * V ** 3 / T
    else:
        b_lat = max(1, apsp["latency_passes"]) * 8.0 * V ** 3 / T
    k = apsp.get("loss_multi", 0)
    dense = bool(apsp.get("loss_dense", 0))
    fused = bool(apsp.get("loss_fused", 0))  # the tight sweep ran inside the latency phase
    if not k:
        b_loss = 12.0 * U * E
    elif dense:
        b_loss = 4.0 * V * V * -(-U // k) + 4.0 * U * V
    else:
        b_loss = 8.0 * E * -(-U // k) + 4.0 * U * V
    # Each phase's `frac` is the fraction of the bound it meets (`bound`): 32-bit integer VALU
    # issue for the squaring passes and the multi-source sweep, HBM for the other forms. The
    # HBM fraction is always given as `hbm_frac` (against HBM_PEAK_GBS) and the loss phase's
    # L2 traffic as `l2_frac` (against L2_PEAK_GBS): L2 bytes are never quoted against the HBM
    # peak.
    out = {}
    for name, b, ms in (("latency_phase", b_lat, apsp["latency_ms"]), ("loss_phase", b_loss, apsp["loss_ms"])):
        gbs = b / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        out[name] = {"bound": "hbm", "alg_bytes": int(b), "ms": round(ms, 3), "achieved": round(gbs, 2),
                     "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 5),
                     "hbm_frac": round(gbs / HBM_PEAK_GBS, 5)}
    # the loss phase against each level it reads: its compulsory HBM bytes — the
    # arc list once (8 B per arc), the used sources' u32 distance rows, the tight lists written
    # and read back (~one arc per node and source, 4 B each way), the f32 loss rows written — and
    # the re-read model above, whose arc re-reads are served by the L2s (MI355X_MICROARCH.md:
    # 4 MiB per XCD, ~34.5 TB/s aggregate), not by HBM
    ms = apsp["loss_ms"]
    if ms > 0 and k:
        hbm = 8.0 * E + 4.0 * U * V + 2 * 4.0 * U * V + 4.0 * U * V
        lp = out["loss_phase"]
        lp["hbm_bytes"] = int(hbm)
        lp["hbm_GBps"] = round(hbm / (ms * 1e-3) / 1e9, 2)
        lp["hbm_frac"] = round(hbm / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5)
        lp["l2_bytes"] = int(b_loss)
        lp["l2_GBps"] = round(b_loss / (ms * 1e-3) / 1e9, 2)
        lp["l2_peak_GBps"] = L2_PEAK_GBS
        lp["l2_frac"] = round(b_loss / (ms * 1e-3) / 1e9 / L2_PEAK_GBS, 5)
        # (alg_bytes / achieved above are the L2-served re-read model; the HBM figure is hbm_GBps)
    # the bound these two forms actually meet: 32-bit integer VALU work. Squaring: per pass every
    # (i, k, j) relaxation is one saturating add and half a v_min3 (1.5 lane-ops, V^3 per pass,
    # the padded V); the multi-source sweep: every (source, arc) pair is one v_add3 and half a
    # v_min3 (1.5 lane-ops, U x E pairs; the dense form also tests the absent arcs of its V x V
    # matrix, which are not counted: the work priced is the same U x E pairs)
    Vp = -(-V // 64) * 64

    def valu_bound(ph, ops, ms_):
        tops = ops / (ms_ * 1e-3) / 1e12
        ph["valu"] = {"lane_ops": int(ops), "achieved_Tops": round(tops, 2), "peak_Tops": VALU_PEAK_TOPS,
                      "frac": round(tops / VALU_PEAK_TOPS, 4)}
        ph.update({"bound": "valu", "achieved": round(tops, 2), "peak": VALU_PEAK_TOPS, "unit": "Tops (int32 lane-ops)",
                   "frac": round(tops / VALU_PEAK_TOPS, 4)})

    if fused and apsp["latency_ms"] > 0:
        # the fused form: the tight sweep over the direct arcs was the squaring's only pass (it
        # found nothing to shorten), so the latency phase's work is that sweep, 1.5 lane-ops per
        # (source, arc) pair; the loss phase is the fold alone (its tight-list bytes: HBM)
        lp, lms = out["latency_phase"], apsp["latency_ms"]
        b_f = 4.0 * V * V * -(-U // k) + 4.0 * U * V
        lp.update({"alg_bytes": int(b_f), "l2_bytes": int(b_f),
                   "l2_frac": round(b_f / (lms * 1e-3) / 1e9 / L2_PEAK_GBS, 5)})
        valu_bound(lp, 1.5 * U * E, lms)
        fl = out["loss_phase"]
        hbm_f = 2 * 4.0 * U * V + 4.0 * U * V
        fl.update({"alg_bytes": int(hbm_f), "hbm_bytes": int(hbm_f),
                   "achieved": round(hbm_f / (ms * 1e-3) / 1e9, 2) if ms > 0 else 0.0,
                   "frac": round(hbm_f / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if ms > 0 else 0.0,
                   "hbm_frac": round(hbm_f / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5) if ms > 0 else 0.0})
        for key in ("l2_bytes", "l2_GBps", "l2_peak_GBps", "l2_frac", "hbm_GBps"):
            fl.pop(key, None)
        fl["bound"] = "hbm"
        fl["unit"] = "GB/s"
        fl["peak"] = HBM_PEAK_GBS
    elif not apsp.get("latency_bf") and not apsp.get("latency_u64", 1) and apsp["latency_ms"] > 0:
        lp, lms = out["latency_phase"], apsp["latency_ms"]
        # compulsory HBM bytes: the u32 matrix read and written once per pass; the panel re-reads
        # of the model above (alg_bytes) are L2-served
        hbm = 8.0 * V * V * max(1, apsp["latency_passes"])
        lp.update({"hbm_bytes": int(hbm), "hbm_GBps": round(hbm / (lms * 1e-3) / 1e9, 2),
                   "hbm_frac": round(hbm / (lms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5), "l2_bytes": int(b_lat),
                   "l2_frac": round(b_lat / (lms * 1e-3) / 1e9 / L2_PEAK_GBS, 5)})
        valu_bound(lp, 1.5 * Vp ** 3 * max(1, apsp["latency_passes"]), lms)
    if apsp.get("latency_bf") and apsp["latency_ms"] > 0:
        # per-source relaxation (sparse graphs): its arc re-reads (the model above) are served by
        # the L2s — every (source, arc, sweep) is one add and one min (1.5 lane-ops with the
        # v_min3 fold), the compulsory HBM bytes are the arc list once and the u64 rows written
        lp, lms = out["latency_phase"], apsp["latency_ms"]
        hbm = 12.0 * E + 8.0 * U * V
        lp.update({"hbm_bytes": int(hbm), "hbm_GBps": round(hbm / (lms * 1e-3) / 1e9, 2),
                   "hbm_frac": round(hbm / (lms * 1e-3) / 1e9 / HBM_PEAK_GBS, 5), "l2_bytes": int(b_lat),
                   "l2_frac": round(b_lat / (lms * 1e-3) / 1e9 / L2_PEAK_GBS, 5)})
        valu_bound(lp, 1.5 * U * E * max(1, apsp["latency_passes"]), lms)
    if k and ms > 0 and not fused:
        valu_bound(out["loss_phase"], 1.5 * U * E, ms)
    out["form"] = {"latency": ("fused tight sweep over the direct arcs = the squaring's one pass (nothing to "
                               "shorten), then sq_run returns at once") if fused else
                              "per-source relaxation" if apsp.get("latency_bf") else
                   ("u64 Floyd-Warshall" if apsp.get("latency_u64", 1) else
                    "u32 min-plus squaring, all passes in one launch (sq_run)"),
                   "loss": (f"dense {k}-source sweep (a lane per head, negated latency matrix, scalar -d[s][u], "
                            "add3/min3 filter; a source's own out-arcs apart) + LDS fold") if k and dense else
                           (f"{k}-source sweep (tail-ordered arcs, branch-free add3/min3 filter) + LDS fold" if k
                            else "one-source arc sweep + LDS fold")}
    out["note"] = ("frac is the fraction of each phase's bound: the squaring passes, the per-source "
                   "relaxation and the multi-source sweep are bound by 32-bit integer VALU issue (lane-ops over the phase's time, each "
                   "phase timed whole including its launches and barrier); hbm_frac (HBM bytes / 8 TB/s) "
                   "and l2_frac (L2-served bytes / 34.5 TB/s) are reported beside it")
    return out


def launch_ranks(n, argv):
    """Runs `python -m torch.distributed.run --nproc-per-node n bench.py <argv>` as a child (the
    driver's own launch line: one node, 127.0.0.1, a free port) and returns its exit status.
    SGN_BENCH_LAUNCH_DRY=1 prints the command as JSON instead (tests/test_bench_launch.py)."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(ROOT / "bench.py")] + list(argv)
    if os.environ.get("SGN_BENCH_LAUNCH_DRY"):
        print(json.dumps(cmd), flush=True)
        return 0
    return subprocess.call(cmd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", choices=("B", "C", "D", "H"), default="C",
                    help="C: the headline 100k-host Tor-like tgen workload; B: 10k hosts, UDP every 10 ms "
                         "on a random graph; D: 1M hosts, dense all-to-all; H: hot-spot fan-in (a test "
                         "workload: 8 servers, every client fetches at once)")
    ap.add_argument("--hosts", type=int, default=None,
                    help="hosts in the simulation (B: 10k, C: 100k, D: 1M), sharded over the GPUs; "
                         "with --weak: hosts per GPU")
    ap.add_argument("--weak", action="store_true",
                    help="weak scaling: --hosts hosts on every GPU (the default is strong scaling: "
                         "--hosts in total, sharded over the GPUs)")
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--rounds-per-step", type=int, default=100)
    ap.add_argument("--cpu-budget-s", type=float, default=12.0,
                    help="wall budget of the CPU mode samples after the parity run")
    ap.add_argument("--full", action="store_true",
                    help="also everything beside the headline figure: at N = 1 the CPU baselines and the "
                         "parity check against the oracle; at N > 1 the other form of the APSP build and "
                         "the unsharded re-run that checks the sharded results (a plain run sets up, warms "
                         "up, times the steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step left (counters, window, per-host "
                         "digests) as DIR/<name>.npy; see dump_outputs")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full at N = 1: skip the CPU baselines and the parity check")
    ap.add_argument("--codel-cap", type=int, default=None,
                    help="CoDel run slots per host on average (the shared page pool's size)")
    ap.add_argument("--one-gpu", action="store_true",
                    help="rehearsal of the N > 1 path on a one-GPU machine: every rank on device 0, each "
                         "with its own NCCL_HOSTID, so RCCL accepts the ranks (as if on different hosts) "
                         "and moves the exchange over its socket transport; correctness only, not a "
                         "scaling measurement")
    ap.add_argument("--exchange-slot", type=int, default=None,
                    help="N > 1: per-peer exchange slot in runs (it grows when a round needs more)")
    ap.add_argument("--no-shard-check", action="store_true",
                    help="with --full at N > 1: skip the unsharded re-run on rank 0 that checks the sharded results")
    args = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `bench.py --gpus N` without a launcher: start the N ranks (one per GPU) under
        # torch.distributed.run as a CHILD process — before anything in this process touches a
        # GPU — and exit with its status (--gpus was ignored, and N > 1 ran one GPU)
        sys.exit(launch_ranks(args.gpus, sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"bench: --gpus {args.gpus} but WORLD_SIZE={world} (one rank per GPU)", file=sys.stderr, flush=True)
        sys.exit(2)
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.one_gpu:
        local = 0
        os.environ["NCCL_HOSTID"] = f"sgn-one-gpu-rank{rank}"
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        os.environ.setdefault("NCCL_IB_DISABLE", "1")
    dist = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method="env://")
    if args.hosts is None:
        args.hosts = {"B": 10_000, "C": 100_000, "D": 1_000_000, "H": 20_000}[args.workload]
    n_total = args.hosts * world if args.weak else args.hosts
    n_shard = -(-n_total // world)  # hosts per GPU (the last shard may hold fewer)
    if args.workload == "C":
        g, used, hosts, cfg, tr = build_workload(n_total, args.nodes)
    elif args.workload == "B":
        g, used, hosts, cfg, tr = build_workload_b(n_total, args.nodes)
    elif args.workload == "H":
        g, used, hosts, cfg, tr = build_workload_h(n_total, args.nodes)
    else:
        stop = max(1_000_000_000, (args.warmup + args.steps + 1) * args.rounds_per_step * 1_000_000)
        g, used, hosts, cfg, tr = build_workload_d(n_total, args.nodes, stop_ns=stop)
        # calendar slabs of 128 runs per host group and bucket: ~64 due on average, 108 at most
        # measured (a 128-run slab keeps the round kernel at 8 workgroups per CU; a fuller slab
        # spills and the calendar is re-laid out with larger slabs, never silently)
        groups = -(-n_shard // 64)
        cfg.event_capacity = 257 * groups * 128
    if cfg.event_capacity and world > 1 and not args.weak and args.workload != "D":
        # the calendar is sized per shard: the same slabs per host group as the one-GPU run
        cfg.event_capacity = -(-cfg.event_capacity // world)

    if args.codel_cap:
        cfg.codel_cap = args.codel_cap
    ctx = sgn.Context(device=local, shard_rank=rank, shard_count=world,
                      flags=2)  # SGN_CREATE_TIME_EXECUTE: HIP events around the round kernel
    if world > 1:
        import torch
        idb = (sgn.C.c_uint8 * 128)()
        if rank == 0:
            ctx.check(ctx.L.sgn_comm_get_unique_id(idb))
        t = torch.tensor(list(bytes(idb)), dtype=torch.uint8)
        dist.broadcast(t, 0)
        idb = (sgn.C.c_uint8 * 128)(*t.tolist())
        # per-peer exchange slot: capacity 8192 event runs per round; a round moves only the
        # high-water size (2x the largest per-peer count seen), ~700-1800 runs per
        # peer at 100k hosts per GPU (overflow of the slot is detected and reported)
        # D (every host sends every 1 ms, 7/8 of it to other shards): ~1e6 x 7/8 / 7 runs per
        # peer per round at 1M hosts per GPU, so its slot holds 2^18 runs (8 MB per peer)
        slot = args.exchange_slot or (1 << 18 if args.workload == "D" else 1 << 13)
        ctx.check(ctx.L.sgn_comm_init(ctx.h, idb, slot))
    # with the communicator set, large graphs (>= 2048 used nodes) build the APSP sharded: each
    # GPU computes its block of used sources and the blocks are exchanged over RCCL
    # (DESIGN.md §5); smaller ones build it whole on every GPU (~1 ms)
    ctx.routes_build(g, used)
    apsp_first = ctx.routes_timing()  # includes loading the APSP kernels' code object
    ctx.routes_build(g, used)         # steady state: the build time proper
    apsp = ctx.routes_timing()
    apsp_shard = None
    if world > 1 and args.full:
        # the other form, timed the same way (second build), bit for bit against the first
        lat_a, loss_a = ctx.routes_copy()
        other = "SGN_APSP_REPLICATED" if apsp["shards"] > 1 else "SGN_APSP_SHARDED"
        os.environ[other] = "1"
        ctx.routes_build(g, used)
        ctx.routes_build(g, used)
        alt = ctx.routes_timing()
        lat_b, loss_b = ctx.routes_copy()
        del os.environ[other]
        same = bool(np.array_equal(lat_a, lat_b) and np.array_equal(loss_a.view(np.uint32), loss_b.view(np.uint32)))
        import torch
        f = torch.tensor([0 if same else 1], dtype=torch.int64)
        dist.all_reduce(f, op=dist.ReduceOp.SUM)
        sh, rep = (apsp, alt) if apsp["shards"] > 1 else (alt, apsp)
        apsp_shard = {"shards": sh["shards"], "equal_on_all_ranks": int(f.item()) == 0,
                      "default_form": "sharded" if apsp["shards"] > 1 else "replicated",
                      "replicated_ms": round(rep["total_ms"], 3), "sharded_ms": round(sh["total_ms"], 3)}
    ctx.hosts_set(hosts)
    ctx.sim_init(cfg, tr)

    def barrier():
        if dist:
            dist.barrier()

    for _ in range(args.warmup):
        ctx.run(args.rounds_per_step)
    st0 = ctx.stats()
    # the round kernel: k_rounds (one shard, persistent: many rounds per launch), k_rounds_x
    # (N > 1, persistent: peer inboxes), or k_execute (per-round launches)
    kts = ctx.kernel_times()
    rk = next(k for k in ("k_rounds", "k_rounds_x", "k_execute") if k in kts)
    kt0 = ctx.kernel_times()[rk]
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ctx.run(args.rounds_per_step)
    barrier()
    el = time.perf_counter() - t0
    st1 = ctx.stats()
    kt1 = ctx.kernel_times()[rk]
    ev = events_of(st1) - events_of(st0)
    if dist:
        import torch
        m = torch.tensor([el], dtype=torch.float64)
        dist.all_reduce(m, op=dist.ReduceOp.MAX)
        el = float(m.item())
        e = torch.tensor([ev], dtype=torch.float64)
        dist.all_reduce(e, op=dist.ReduceOp.SUM)
        ev = int(e.item())
    d = {k: st1[k] - st0[k] for k in st1}
    rounds = d["rounds"]
    # roofline of the dominant kernel (k_rounds on one shard, k_execute multi-shard): algorithmic bytes per launch
    # = SURVEY.md §8(d)'s packet-path model, 128 B per packet (send record, DNS, node
    # indices, route entry, event record write, sort/merge, pop read) + 96 B per active
    # host-round (RNG state, event-id counter, queue head), over the units one launch
    # processes, / the launch's average duration (HIP events on the engine stream).
    # Every persistent launch (k_rounds, 100 rounds) is timed; per-round launches (k_execute)
    # are timed one in eight (an event pair around every launch cost ~20 % of the rounds), so
    # their average duration comes from the sample and the launch count is the round count.
    timed = kt1[0] - kt0[0]
    persistent = rk in ("k_rounds", "k_rounds_x")
    launches = timed if persistent else rounds
    exec_ms = kt1[1] - kt0[1]
    n_pkt = d["packets_sent"] + d["packets_loss_dropped"]
    host_exec = d["host_executions"]
    alg_bytes = 128 * n_pkt + 96 * host_exec
    roof = None
    if timed and launches and exec_ms > 0:
        avg_s = exec_ms / timed / 1e3
        achieved = alg_bytes / launches / avg_s / 1e9
        rpl = rounds / launches
        roof = {"bound": "hbm", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": None,
                "kernel": rk, "avg_launch_us": round(avg_s * 1e6, 2), "timed_launches": timed,
                "alg_bytes_per_launch": int(alg_bytes / launches),
                "units_per_launch": {"packets": round(n_pkt / launches, 1),
                                     "active_host_rounds": round(host_exec / launches, 1),
                                     "rounds": round(rpl, 2)},
                "latency_bound": {
                    "round_us": round(avg_s * 1e6 / rpl, 2),
                    "note": "the round is a chain: per-host serial event loops (RNG stream and event "
                            "ids force in-order work inside a host) with dependent memory round trips, "
                            "then a grid-wide barrier; HBM bytes are not what bounds it"}}
        # HBM bytes per launch measured by PMC (tools/pmc_traffic.sh: FETCH_SIZE x2 +
        # WRITE_SIZE, separate passes) over the timed launches of THIS invocation: the entry
        # keyed by workload, hosts, rounds per launch, GPUs, steps and warmup (null otherwise)
        tf = ROOT / "profiles" / "round_kernel_traffic.json"
        if tf.exists():
            want = {"name": args.workload, "hosts_per_gpu": n_shard, "graph_nodes": args.nodes,
                    "rounds_per_launch": round(rpl), "n_gpus": world, "steps": args.steps, "warmup": args.warmup}
            build = sgn.build_id()
            roof["traffic_note"] = f"no PMC entry for this invocation on this libsgn build ({build})"
            for t in json.loads(tf.read_text()).get("entries", []):
                if t.get("workload") == want and t.get("kernel") == rk and t.get("build") == build:
                    roof["traffic_note"] = f"measured on this libsgn build ({build})"
                    roof["traffic"] = t["traffic_bytes_per_launch"]
                    roof["traffic_unit"] = "bytes/launch (PMC, profiles/round_kernel_traffic.json)"
                    roof["traffic_provenance"] = t.get("bench_args")
                    roof["traffic_uncorrected"] = t.get("traffic_bytes_per_launch_uncorrected")
                    roof["traffic_GBps"] = round(t["traffic_bytes_per_launch"] / avg_s / 1e9, 2)
    info = ctx.engine_info()
    if roof is not None:
        # why the kernel sits far below the HBM roof: a latency chain on a partly filled chip.
        # Workgroups are one wave; k_rounds keeps its grid resident (each workgroup serves
        # groups g, g + grid, ...), k_execute launches one workgroup per group every round.
        grid = {"k_rounds": info["persistent_grid"], "k_rounds_x": info["persistent_x_grid"]}.get(rk, info["host_groups"])
        wave_rounds = info["host_groups"] * max(1, rounds)
        roof["occupancy"] = {
            "compute_units": info["compute_units"],
            "resident_waves_per_cu": round(min(grid, 8 * info["compute_units"]) / max(1, info["compute_units"]), 2),
            "lanes_per_wave": 64, "hosts_per_wave": info["hosts_per_wave"],
            "busy_lanes_per_wave_round": round(host_exec / wave_rounds, 2),
            "note": "a host runs in its own lane; busy lanes = hosts with an event due in the window, "
                    "averaged over every (group, round); the slowest wave of a round sets its length"}
    out = {
        "metric": METRIC,
        "value": ev / el,
        "unit": "packet events/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": el * 1e3 / args.steps,
        "higher_is_better": True,
        "scaling": "weak" if args.weak else "strong",
        "vs_baseline": None,
        "dtype": "u64",
        "data": "synthetic",
        "config": {
            "workload": {"C": "C: Tor-like 1000-node complete graph, tgen-style UDP trains",
                         "B": "B: 1000-node random graph (20 % lossy edges), 1024 B UDP every 10 ms to random peers",
                         "D": "D: 1000-node random graph, every host sends 64 B to a uniform random peer every 1 ms",
                         "H": "H (test workload): hot-spot fan-in, every client fetches from one of 8 servers",
                         }[args.workload],
            "hosts_per_gpu": n_shard, "hosts_total": n_total, "graph_nodes": args.nodes,
            "rounds_per_step": args.rounds_per_step, "runahead_ms": 1,
            "parallelism": f"host-shard x{world}" + (" (one-GPU rehearsal: all ranks on device 0, RCCL socket transport)" if args.one_gpu else ""),
        },
        "apsp_build_ms": round(apsp["total_ms"], 3),
        "apsp": {k: (round(v, 3) if isinstance(v, float) else v) for k, v in apsp.items()},
        "apsp_first_build_ms": round(apsp_first["total_ms"], 3),
        "apsp_roofline": apsp_roofline(apsp, args.nodes, len(used)),
        "apsp_sharded": apsp_shard,
        "sim_ms_per_step": None,
        "rounds_timed": rounds,
        "packet_events_timed": ev,
        "roofline": roof,
        "cpu_baseline": None,
        "parity": None,
        "max_slab_fill": st1["max_pending_events"],
        "hbm_footprint_bytes": info["device_bytes"],
        "engine": {k: info[k] for k in ("calendar_buckets", "bucket_width_ns", "host_groups", "slab_capacity",
                                        "persistent_grid", "persistent_fallbacks", "codel_pages",
                                        "codel_page_allocs", "bucket_min_lds", "codel_pool_grows",
                                        "calendar_grows", "exchange_slot_grows", "rounds_held",
                                        "slab_extensions", "big_slab_pieces", "calendar_spill_runs")},
    }
    if world > 1:
        # the round exchange: per-peer slot, runs per peer a round moves now
        # (2x the largest per-peer count seen, a power of two), rounds held and completed with
        # the whole slot, and bytes this rank sent to peers per round since sim_init
        out["exchange"] = {"slot_runs": info["exchange_slot_runs"], "send_runs": info["exchange_send_runs"],
                           "hwm_runs": info["exchange_hwm_runs"], "spills": info["exchange_spills"],
                           "bytes_per_round": round(info["exchange_bytes"] / max(1, st1["rounds"])),
                           # 2: persistent rounds (k_rounds_x: peer inboxes over xGMI), 1: per-round
                           # launches with the RCCL exchange
                           "mode": info["exchange_mode"], "persistent_launches": info["persistent_x_launches"],
                           "inbox_slot_runs": info["inbox_slot_runs"], "inbox_grows": info["inbox_grows"],
                           "inbox_overflow_rounds": info["inbox_overflow_rounds"]}
    ws, we, act = ctx.window()
    out["sim_time_reached_ms"] = (ws - sgn.SIMULATION_START) / 1e6
    out["sim_ms_per_step"] = out["sim_time_reached_ms"] / (args.steps + args.warmup)
    ok = apsp_shard is None or apsp_shard["equal_on_all_ranks"]
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, ctx, hosts.n, rank, world)
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        gpu = {"rounds_timed": rounds, "stats": st1, "window": (ws, we, act),
               "digests": ctx.digests(0, hosts.n)}
        out["cpu_baseline"], par = cpu_baseline(g, used, hosts, cfg, tr, args, gpu)
        out["parity"] = par["ok"]
        out["parity_detail"] = par
        ok = ok and par["ok"]
    if world > 1 and args.full and not args.no_shard_check:
        def unsharded():
            c1 = sgn.Context(device=local)
            c1.routes_build(g, used)
            c1.hosts_set(hosts)
            cfg1 = type(cfg).from_buffer_copy(cfg)
            if cfg1.event_capacity:  # calendar sized per host group: N x the groups
                cfg1.event_capacity *= world
            c1.sim_init(cfg1, tr)
            return c1

        par = shard_check(ctx, dist, rank, world, hosts.n, int(st1["rounds"]), unsharded)
        if rank == 0:
            out["parity"] = par["ok"]
            out["parity_detail"] = par
            ok = ok and par["ok"]
    if rank == 0:
        print(json.dumps(out), flush=True)
    ctx.close()
    if dist:
        dist.destroy_process_group()
    if not ok:
        print("bench: GPU results differ from the oracle (parity false)", file=sys.stderr, flush=True)
        sys.exit(3)


if __name__ == "__main__":
    main()
