#!/usr/bin/env python3
"""What the router delay report costs (one GPU): sgn_delay_fold against the parent commit's way to
the same numbers.

Scenario: config C's graph and hosts (100 k hosts) with EXTERNAL traffic; `--datagrams` (1 M)
datagrams from random hosts to `--traced` (300) chosen hosts — fan-in — over `--seconds` (3) of
simulated time; only the chosen hosts are traced. A snapshot is saved before the first round.
`--repeats` times, in rotating order, each leg from a restore of that snapshot, the run in intervals
of `--interval-ms` (100), each interval's datagrams submitted before it:
  fold  sgn_delay_fold at every interval's end (sgn_delay_enable after the restore), then
        sgn_delay_get                                   — and the HIP-event split of the folds;
  join  sgn_trace_take into arrays allocated once and touched beforehand, then the key join on the
        host in numpy: pops and exits of the take and the carried pops sorted together by (host,
        peer, c, pop-before-exit), so every exit stands right behind its pop; delays, per-host sums
        and both histograms from there                  — the code of the parent commit: the baseline.
Only the fold / take + join calls are timed, not the rounds between them. The two legs' totals,
maxima and histograms are compared (the same integers).

Skewed case: the report's kernels alone (sgn_selftest_delay_fold) on `--datagrams` records with one
host holding `--skew` (200 k) of them, so the workgroup walker runs at scale; the result is checked
against delays computed here by rank.

The kernels' time is set against the HBM peak (8 TB/s, the figure bench.py's roofline uses): the
count reads every record's line once, the match once more (56 B each), a walked span's pops write
and its exits read an 8-byte index, and the carry is read and written once (24 B an entry).
One JSON line per repeat and summary lines, appended to --out when given.

usage: python tools/delay_timing.py [--hosts 100000] [--datagrams 1000000] [--repeats 5] [--out FILE]
"""
import argparse
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "shadow-gen_amd"))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402

import bench  # noqa: E402
import sgn  # noqa: E402
from sample_timing import HBM_PEAK_BYTES_PER_S, median  # noqa: E402

REC, ENT = 56, 24
MS = 1_000_000
EDGES = np.array([1 << k for k in range(sgn.DELAY_BINS - 1)], dtype=np.uint64)  # bin = edges <= delay


def kernel_bytes(t):
    big = t["largest_span"] if t["spans_by_class"][1] else 0  # (a lower bound when several spans are walked)
    return 2 * REC * t["records"] + 16 * big + 2 * ENT * t["carry_entries"]


def hbm_share(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 5) if ms > 0 else None


class Join:
    """The baseline's state: the pops not yet exited (host, peer, c, a), and the accumulators."""

    def __init__(self, n_hosts):
        self.carry = np.zeros(0, dtype=sgn.TRACE_DTYPE)
        self.hist = np.zeros((2, sgn.DELAY_BINS), np.uint64)
        self.count = np.zeros((2, n_hosts), np.uint64)
        self.sum = np.zeros((2, n_hosts), np.uint64)
        self.max = np.zeros(n_hosts, np.uint64)

    def fold(self, recs):
        k = recs["kind"]
        pops = np.concatenate([self.carry, recs[k == sgn.TRACE_POP]])
        exits = recs[(k == sgn.TRACE_DELIVER) | (k == sgn.TRACE_CODEL_DROP)]
        both = np.concatenate([pops, exits])
        is_exit = np.concatenate([np.zeros(len(pops), np.uint8), np.ones(len(exits), np.uint8)])
        order = np.lexsort((is_exit, both["c"], both["peer"], both["host"]))
        both, is_exit = both[order], is_exit[order]
        x = np.nonzero(is_exit)[0]
        p = x - 1
        assert len(x) == 0 or (p[0] >= 0 and not is_exit[p].any())
        assert np.array_equal(both["host"][p], both["host"][x]) and np.array_equal(both["c"][p], both["c"][x])
        d = both["a"][x] - both["a"][p]
        drop = (both["kind"][x] == sgn.TRACE_CODEL_DROP).astype(np.int64)
        h = both["host"][x].astype(np.int64)
        np.add.at(self.hist, (drop, np.searchsorted(EDGES, d, side="right")), np.uint64(1))
        np.add.at(self.count, (drop, h), np.uint64(1))
        np.add.at(self.sum, (drop, h), d)
        np.maximum.at(self.max, h, d)
        left = np.ones(len(both), bool)
        left[x] = False
        left[p] = False
        self.carry = both[left]

    def totals(self):
        return [int(self.count[0].sum()), int(self.count[1].sum()), int(self.sum[0].sum()), int(self.sum[1].sum()),
                len(self.carry), 0]


def simulation(a, emit):
    g, used, hst, cfg, _ = bench.build_workload(a.hosts, a.nodes)
    tr = sgn.make_traffic(sgn.TRAFFIC_EXTERNAL)
    rng = np.random.default_rng(1)
    traced = np.sort(rng.choice(a.hosts, a.traced, replace=False)).astype(np.uint32)
    k = a.datagrams
    ctxs, snaps = {}, {}
    for leg in ("fold", "join"):  # a context each: the report, once enabled, folds every take of its context
        c = sgn.Context(device=0)
        c.routes_build(g, used)
        c.hosts_set(hst)
        c.trace_enable(4 * k)
        c.trace_hosts(traced)
        c.drain_enable(max(1 << 20, 2 * k))
        c.sim_init(cfg, tr)
        ctxs[leg], snaps[leg] = c, c.snapshot_save()
    info = c.engine_info()
    step = a.interval_ms * MS
    assert step + 2 * MS < (info["calendar_buckets"] - 2) * info["bucket_width_ns"], "an interval must fit the calendar's horizon"
    src = rng.integers(0, a.hosts, k).astype(np.uint32)
    dst = hst.ip[rng.choice(traced, k)].astype(np.uint32)
    t = sgn.SIMULATION_START + np.sort(rng.integers(0, a.seconds * 1000 * MS, k)).astype(np.uint64)
    pay = np.full(k, 100, np.uint32)
    handle = np.arange(1, k + 1, dtype=np.uint64)
    n_steps = a.seconds * 1000 // a.interval_ms + 5  # (the last packets leave the routers after the last send)
    buf = np.ones(4 * k, dtype=sgn.TRACE_DTYPE)  # (pages touched)
    spans = np.ones(a.hosts, dtype=sgn.SPAN_DTYPE)
    out = {}

    def run(leg):
        import ctypes as C
        c = ctxs[leg]
        c.snapshot_restore(snaps[leg])
        c.drain()  # (nothing of an earlier leg)
        if leg == "fold":
            c.delay_enable()
        join = Join(a.hosts)
        spent, nxt, records, split = 0.0, 0, 0, []
        got, n_spans = C.c_uint64(), C.c_uint64()
        for s in range(1, n_steps + 1):
            T = sgn.SIMULATION_START + s * step
            j = int(np.searchsorted(t, T + MS, side="left"))
            if j > nxt:
                ws, _, active = c.window()
                if not active or int(t[nxt]) < ws:  # (a CPU controller's rule: the window comes back to its own next send)
                    c.set_window(int(t[nxt]), int(t[nxt]) + MS)
                c.submit(src[nxt:j], dst[nxt:j], pay[nxt:j], t[nxt:j], handle[nxt:j])
                nxt = j
            c.run_until(T)
            c.drain()
            t0 = time.perf_counter()
            if leg == "fold":
                c.check(c.L.sgn_delay_fold(c.h, None))
            else:
                c.check(c.L.sgn_trace_take(c.h, buf.ctypes.data_as(C.POINTER(sgn.TraceRec)), len(buf), C.byref(got),
                                           spans.ctypes.data_as(C.POINTER(sgn.TraceSpan)), len(spans), C.byref(n_spans)))
                join.fold(buf[: got.value])
                records += got.value
            spent += time.perf_counter() - t0
            if leg == "fold":
                split.append(c.delay_timing())
        t0 = time.perf_counter()
        if leg == "fold":
            d = c.delay()
            out[leg] = dict(total=d.info["total"], hist=[d.info["hist_delivered"], d.info["hist_dropped"]], max=d.info["delay_max"],
                            records=d.info["records"], folds=d.info["folds"], split=split)
        else:
            out[leg] = dict(total=join.totals(), hist=join.hist.tolist(), max=int(join.max.max()), records=records, folds=n_steps)
        return (spent + time.perf_counter() - t0) * 1e3

    legs = ("fold", "join")
    for leg in legs:  # (nobody's first run is reported: code objects are loaded, scratch is allocated)
        run(leg)
    assert out["fold"]["total"][:5] == out["join"]["total"][:5] and out["fold"]["hist"] == out["join"]["hist"], (out["fold"]["total"], out["join"]["total"])
    assert out["fold"]["max"] == out["join"]["max"] and out["fold"]["records"] == out["join"]["records"]
    per = []
    for rep in range(a.repeats):
        res = {}
        for leg in legs[rep % 2:] + legs[: rep % 2]:
            res[leg + "_wall_ms"] = round(run(leg), 3)
        sp = out["fold"]["split"]
        res.update(case="repeat", rep=rep, records=out["fold"]["records"], folds=out["fold"]["folds"], traced=a.traced,
                   matched=out["fold"]["total"][0] + out["fold"]["total"][1], delay_max_ns=out["fold"]["max"],
                   order_ms=[round(sum(x["order_ms"][i] for x in sp), 4) for i in range(3)],
                   kernel_ms=[round(sum(x["kernel_ms"][i] for x in sp), 4) for i in range(5)],
                   kernel_bytes=sum(kernel_bytes(x) for x in sp))
        res["kernel_hbm_share"] = hbm_share(res["kernel_bytes"], sum(res["kernel_ms"]))
        emit(res)
        per.append(res)
    med = lambda key: median([r[key] for r in per])  # noqa: E731
    rng_ = lambda key: [min(r[key] for r in per), max(r[key] for r in per)]  # noqa: E731
    emit({"case": "summary", "hosts": a.hosts, "traced": a.traced, "records": per[-1]["records"], "folds": per[-1]["folds"],
          "matched": per[-1]["matched"], "repeats": a.repeats,
          "fold_wall_ms_median": med("fold_wall_ms"), "fold_wall_ms_range": rng_("fold_wall_ms"),
          "join_wall_ms_median": med("join_wall_ms"), "join_wall_ms_range": rng_("join_wall_ms"),
          "order_ms_median": [round(median([r["order_ms"][i] for r in per]), 4) for i in range(3)],
          "kernel_ms_median": [round(median([r["kernel_ms"][i] for r in per]), 4) for i in range(5)],
          "kernel_hbm_share_median": median([r["kernel_hbm_share"] for r in per if r["kernel_hbm_share"] is not None] or [None])})
    for leg, c in ctxs.items():
        c.snapshot_free(snaps[leg])
        c.close()


def skewed_records(a):
    """n records: one host with a long FIFO history (a reflected random walk: an exit that would find
    the router empty is another kind of record), the others pop-then-exit pairs. Returns the records
    (shuffled) and the expected (delivered, dropped, sum of all delays, largest delay)."""
    n, big = a.datagrams, min(a.skew, a.datagrams)
    rng = np.random.default_rng(2)
    r = np.zeros(n, dtype=sgn.TRACE_DTYPE)
    hot = a.hosts // 3
    small = rng.integers(0, a.hosts - 1, n - big).astype(np.uint32)
    small[small >= hot] += 1
    small.sort()
    r["host"][:big] = hot
    r["host"][big:] = small
    r["a"] = np.cumsum(rng.integers(0, 2000, n).astype(np.uint64))
    # the hot host
    s = np.where(rng.random(big) < 0.52, 1, -1)
    S = np.cumsum(s)
    low = np.minimum.accumulate(np.minimum(S, 0))
    idle = (s < 0) & (S == low) & (S < 0)  # an exit at a new minimum: the router was empty
    kind = np.where(idle, sgn.TRACE_SEND, np.where(s > 0, sgn.TRACE_POP, sgn.TRACE_DELIVER)).astype(np.uint32)
    kind[(kind == sgn.TRACE_DELIVER) & (rng.random(big) < 0.2)] = sgn.TRACE_CODEL_DROP
    r["kind"][:big] = kind
    r["seq"][:big] = np.arange(big)
    pops = np.nonzero(kind == sgn.TRACE_POP)[0]
    exits = np.nonzero((kind == sgn.TRACE_DELIVER) | (kind == sgn.TRACE_CODEL_DROP))[0]
    r["c"][pops] = np.arange(len(pops)) + (1 << 33)
    r["peer"][pops] = np.arange(len(pops)) % 977
    r["c"][exits] = r["c"][pops[: len(exits)]]
    r["peer"][exits] = r["peer"][pops[: len(exits)]]
    delays = [r["a"][exits] - r["a"][pops[: len(exits)]]]
    drops = int((kind == sgn.TRACE_CODEL_DROP).sum())
    # the others: rank inside the host; even ranks pop, odd ranks deliver the pop before them
    h = r["host"][big:]
    first = np.concatenate([[0], np.nonzero(np.diff(h))[0] + 1])
    rank = np.arange(len(h)) - np.repeat(first, np.diff(np.concatenate([first, [len(h)]])))
    r["seq"][big:] = rank
    r["kind"][big:] = np.where(rank % 2 == 0, sgn.TRACE_POP, sgn.TRACE_DELIVER)
    r["c"][big:] = (rank // 2) + (1 << 20)
    r["peer"][big:] = 5
    odd = big + np.nonzero(rank % 2 == 1)[0]
    delays.append(r["a"][odd] - r["a"][odd - 1])
    d = np.concatenate(delays)
    expect = (len(exits) - drops + len(odd), drops, int(d.sum(dtype=np.uint64)), int(d.max()))
    return r[rng.permutation(n)], expect


def skewed(a, emit):
    recs, expect = skewed_records(a)
    c = sgn.Context(device=0)
    per = []
    for rep in range(a.repeats + 1):
        t0 = time.perf_counter()
        d = sgn.selftest_delay_fold(c, recs, [len(recs)], 0, a.hosts)
        wall = (time.perf_counter() - t0) * 1e3
        got = (d.info["total"][0], d.info["total"][1], d.info["total"][2] + d.info["total"][3], d.info["delay_max"])
        assert got == expect, (got, expect)
        if rep == 0:
            continue  # (the first call allocates the scratch)
        tt = c.delay_timing()
        res = dict(case="skewed", rep=rep - 1, records=len(recs), hosts_with_records=tt["hosts"], wall_ms=round(wall, 3),
                   order_ms=[round(x, 4) for x in tt["order_ms"]], kernel_ms=[round(x, 4) for x in tt["kernel_ms"]],
                   spans_by_class=tt["spans_by_class"], largest_span=tt["largest_span"], carry_entries=tt["carry_entries"],
                   kernel_bytes=kernel_bytes(tt), kernel_hbm_share=hbm_share(kernel_bytes(tt), sum(tt["kernel_ms"])))
        emit(res)
        per.append(res)
    emit({"case": "skewed-summary", "records": len(recs), "largest_span": per[-1]["largest_span"],
          "spans_by_class": per[-1]["spans_by_class"],
          "order_ms_median": [round(median([r["order_ms"][i] for r in per]), 4) for i in range(3)],
          "kernel_ms_median": [round(median([r["kernel_ms"][i] for r in per]), 4) for i in range(5)],
          "kernel_ms_range": [[min(r["kernel_ms"][i] for r in per), max(r["kernel_ms"][i] for r in per)] for i in range(5)],
          "kernel_hbm_share_median": median([r["kernel_hbm_share"] for r in per if r["kernel_hbm_share"] is not None] or [None])})
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=100_000)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--datagrams", type=int, default=1_000_000)
    ap.add_argument("--traced", type=int, default=300)
    ap.add_argument("--seconds", type=int, default=3)
    ap.add_argument("--interval-ms", type=int, default=100)
    ap.add_argument("--skew", type=int, default=200_000, help="records of the one large host of the skewed case")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-simulation", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(d):
        d = {"tool": "delay_timing", "build_id": sgn.build_id(), **d}
        print(json.dumps(d), flush=True)
        lines.append(d)

    def flush():
        if a.out:
            with open(a.out, "a", encoding="utf-8") as f:
                for d in lines:
                    f.write(json.dumps(d) + "\n")
            lines.clear()

    skewed(a, emit)
    flush()
    if not a.skip_simulation:
        simulation(a, emit)
        flush()


if __name__ == "__main__":
    main()
