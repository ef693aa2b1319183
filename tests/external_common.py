"""Shared driver for the CPU-resident-application path (SGN_TRAFFIC_EXTERNAL): a CPU
controller that submits datagrams, moves the window to its own next send when that comes
first (sgn_set_window) and drains the datagrams' fates. Used against the oracle alone (CPU
tests) and against libsgn + the oracle in lockstep (GPU tests)."""
import numpy as np

import sgn

RUNAHEAD = 1_000_000


def external_world(n=60, V=20, seed=3, bw=2_000_000, fifo=4, stop_ns=400_000_000, *, lat_hi_us=50000,
                   codel_cap=4096, qdisc=0, dynamic=False, slow_every=7):
    g = sgn.random_graph(V, mean_degree=min(6, V - 1), seed=seed, lat_hi_us=lat_hi_us, loss_frac=0.5,
                         loss_hi=0.05)
    used = np.arange(V)
    names = sgn.host_names(n)
    seeds = sgn.derive_seeds(11, names)
    bwv = np.full(n, bw, dtype=np.uint64)
    bwv[::slow_every] = 200_000  # slow links: standing CoDel queues and drops
    hosts = sgn.HostArrays(sgn.assign_ips(n), (np.arange(n) * 5) % V, bwv, bwv, seeds)
    cfg = sgn.make_config(stop_ns, runahead_ns=RUNAHEAD, out_fifo_cap=fifo, codel_cap=codel_cap,
                          event_capacity=1 << 18, qdisc=qdisc, dynamic=dynamic)
    tr = sgn.make_traffic(sgn.TRAFFIC_EXTERNAL)
    return g, used, hosts, cfg, tr


def datagrams(hosts, k=600, seed=5, span_ns=150_000_000, *, unknown=0.05, to_self=0.05, wire_kinds=(0, 1, 2, 3),
              unique_times=False):
    """k datagrams: random peers, some to unknown addresses or to the sender itself, bursts
    from a few hosts (send-queue blocking), times over [0, span). wire_kinds: the wire-length
    forms in use (0: implied, 1: UDP, 2: TCP, 3: TCP with window scale); unique_times: no two
    datagrams share a send time (and all lie below span + k ns)."""
    rng = np.random.default_rng(seed)
    n = hosts.n
    src = rng.integers(0, n, k).astype(np.uint32)
    src[: k // 4] = rng.integers(0, 3, k // 4)  # bursty senders
    dst = rng.integers(0, n, k)
    dip = hosts.ip[dst].astype(np.uint32)
    unk = rng.random(k) < unknown
    dip[unk] = 0x0AFF0000 + rng.integers(1, 1000, unk.sum())  # 10.255/16: not registered
    me = rng.random(k) < to_self
    dip[me] = hosts.ip[src[me]]
    pay = rng.integers(0, 1473, k).astype(np.uint32)
    pay[rng.random(k) < 0.1] = 0
    t = sgn.SIMULATION_START + np.sort(rng.integers(0, span_ns, k)).astype(np.uint64)
    t[: k // 4] = sgn.SIMULATION_START + np.sort(rng.integers(0, span_ns // 10, k // 4)).astype(np.uint64)
    order = np.argsort(t, kind="stable")
    if unique_times:  # strictly increasing in sorted order
        i = np.arange(k, dtype=np.uint64)
        t[order] = np.maximum.accumulate(t[order] - i) + i
    handle = (np.arange(k, dtype=np.uint64) * 0x9E3779B97F4A7C15) & np.uint64(0xFFFFFFFFFFFFFFFF)
    # wire lengths: UDP (0 = implied, or payload + 28) and TCP segments from the CPU TCP stack
    # (payload + 40, + 44 with the window-scale option: network/packet.rs:617-635)
    kind = np.asarray(wire_kinds)[rng.integers(0, 4, k) % len(wire_kinds)]
    wire = np.where(kind == 0, 0, pay + np.array([0, 28, 40, 44])[kind]).astype(np.uint32)
    return src[order], dip[order], pay[order], t[order], handle[order], wire[order]


def drive(sims, dg, rng_hosts=(1, 2), max_rounds=100_000, on_round=None):
    """Runs every sim in lockstep as a CPU controller would; returns the drain records of
    each (list of arrays) and the number of rounds."""
    src, dip, pay, t, handle, wire = dg
    nxt = 0
    drains = [[] for _ in sims]
    rounds = 0
    while rounds < max_rounds:
        wins = [s.window() for s in sims]
        assert all(w == wins[0] for w in wins), wins
        ws, we, active = wins[0]
        if nxt < len(t) and (not active or int(t[nxt]) < ws):
            ws, we = int(t[nxt]), int(t[nxt]) + RUNAHEAD
            for s in sims:
                s.set_window(ws, we)
            we = sims[0].window()[1]
        elif not active:
            break
        j = nxt
        while j < len(t) and int(t[j]) < we:
            j += 1
        if j > nxt:
            for s in sims:
                s.submit(src[nxt:j], dip[nxt:j], pay[nxt:j], t[nxt:j], handle[nxt:j], wire_len=wire[nxt:j])
            nxt = j
        mins = [s.round() for s in sims]
        assert all(m == mins[0] for m in mins), mins
        rounds += 1
        if rounds % 7 == 0:
            # CPU-side draws from the device-held host RNG (host_rngDouble / NextNBytes)
            h = rng_hosts[rounds % len(rng_hosts)]
            vals = [(s.rng_next_u64(h), s.rng_double(h), s.rng_fill_bytes(h, rounds % 13)) for s in sims]
            assert all(v == vals[0] for v in vals), vals
        if rounds % 5 == 0:
            half = 30
            for i, s in enumerate(sims):
                drains[i].append(s.drain(0, half))
                drains[i].append(s.drain(half, 1 << 32 - 1))
        if on_round:
            on_round(rounds)
    for i, s in enumerate(sims):
        drains[i].append(s.drain())
    return [np.concatenate(d) if d else np.zeros(0, sgn.DRAIN_DTYPE) for d in drains], rounds


def calendar_shape(lat, cfg):
    """(buckets, bucket width in ns) of the event calendar as sgn_sim_init sizes it from the route
    latencies and the runahead (engine_info() reports the same two numbers on the device); the
    CPU tests choose datagram spans below the submit horizon with it."""
    lo, hi = int(np.min(lat)), int(np.max(lat))
    bw = max(1, lo, int(cfg.runahead_ns))
    wmax = max(bw, hi, int(cfg.runahead_ns)) if cfg.use_dynamic_runahead else bw
    nb = (3 * wmax + hi) // bw + 8
    while nb & (nb - 1):
        nb += nb & -nb
    return nb, bw


def advance_to(s, t_emulated):
    """Whole windows until the next one would start at or after t_emulated (or the end): libsgn's
    sgn_run_until, and the same rule a round at a time on the oracle. Returns the rounds run."""
    if hasattr(s, "run_until"):
        return s.run_until(t_emulated)
    k = 0
    while True:
        ws, _, active = s.window()
        if not active or ws >= t_emulated:
            return k
        s.round()
        k += 1


def drive_ahead(sims, dg, step_ns, rng_hosts=(1, 2), rng_every=2, drain_every=3, window_ns=RUNAHEAD,
                lookahead_ns=None, calendar=None, k0=0, nxt0=0, stop_step=None, max_steps=100_000,
                on_step=None, log=None):
    """A CPU controller that submits ahead and runs many rounds per call: for the targets
    T_k = SIMULATION_START + k * step_ns it submits (one call per sim) every datagram with
    t < T_k + lookahead_ns not yet submitted, then advances every sim to T_k (advance_to). The
    last window of such a run starts below T_k and ends at most a window length past it, hence
    the lookahead: window_ns with a static runahead; the longest possible window with a dynamic
    one. Windows are compared at every step; every rng_every steps the CPU-side RNG draws and
    every drain_every steps the split drain of drive(). The furthest datagram of a submit must
    lie below the calendar's horizon (from the first sim with engine_info(), else from
    `calendar` = calendar_shape(); unchecked without either).

    k0 / nxt0 / stop_step resume and interrupt a run (log["nxt"] after the call is the position to
    resume from); on_step(k) runs after step k's draws and drains. Returns the drain records of
    each sim and the number of rounds, as drive() does; log["draws"] gets the RNG draws per sim and
    log["rounds_per_step"] the rounds each step's advance ran."""
    src, dip, pay, t, handle, wire = dg
    look = window_ns if lookahead_ns is None else lookahead_ns
    if calendar is None:
        info = next((s.engine_info() for s in sims if hasattr(s, "engine_info")), None)
        calendar = (info["calendar_buckets"], info["bucket_width_ns"]) if info else None
    nxt, k, rounds = nxt0, k0, 0
    drains = [[] for _ in sims]
    draws = [[] for _ in sims]
    per_step = []
    finished = False
    while k - k0 < max_steps and (stop_step is None or k < stop_step):
        k += 1
        T = sgn.SIMULATION_START + k * step_ns
        wins = [s.window() for s in sims]
        assert all(w == wins[0] for w in wins), (k, wins)
        ws, we, active = wins[0]
        if nxt < len(t) and (not active or int(t[nxt]) < ws):
            ws = int(t[nxt])
            for s in sims:
                s.set_window(ws, ws + window_ns)
        elif nxt == len(t) and not active:
            finished = True
            break
        j = max(nxt, int(np.searchsorted(t, T + look, side="left")))
        if j > nxt:
            if calendar is not None:
                horizon = ws + (calendar[0] - 2) * calendar[1]
                assert int(t[j - 1]) < horizon, (k, int(t[j - 1]) - ws, horizon - ws)
            for s in sims:
                s.submit(src[nxt:j], dip[nxt:j], pay[nxt:j], t[nxt:j], handle[nxt:j], wire_len=wire[nxt:j])
            nxt = j
        ran = [advance_to(s, T) for s in sims]
        assert all(r == ran[0] for r in ran), (k, ran)
        rounds += ran[0]
        per_step.append(ran[0])
        wins = [s.window() for s in sims]
        assert all(w == wins[0] for w in wins), (k, wins)
        if k % rng_every == 0:
            h = rng_hosts[k % len(rng_hosts)]
            vals = [(s.rng_next_u64(h), s.rng_double(h), s.rng_fill_bytes(h, k % 13)) for s in sims]
            assert all(v == vals[0] for v in vals), (k, vals)
            for i, v in enumerate(vals):
                draws[i].append(v)
        if k % drain_every == 0:
            half = 30
            for i, s in enumerate(sims):
                drains[i].append(s.drain(0, half))
                drains[i].append(s.drain(half, 1 << 31))
        if on_step:
            on_step(k)
    assert finished or stop_step is not None, "drive_ahead: the simulation did not run dry"
    if finished:
        for i, s in enumerate(sims):
            drains[i].append(s.drain())
    if log is not None:
        log.update(nxt=nxt, k=k, draws=draws, finished=finished, rounds_per_step=per_step)
    return [np.concatenate(d) if d else np.zeros(0, sgn.DRAIN_DTYPE) for d in drains], rounds
