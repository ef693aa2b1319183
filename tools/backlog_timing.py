#!/usr/bin/env python3
"""What a backlog report of a running simulation costs (one GPU), at config C (100 k hosts, TGEN)
and config D (1 M hosts, PERIODIC), at mid-run round edges.

After a warm-up, `--repeats` times: run `--rounds` rounds, then on the same context, in alternating
order,
  totals  sgn_backlog(NULL, 0, ...) — the totals-only form; wall clock around the call and the
          HIP-event split of sgn_backlog_timing_get (calendar pass, count, scan, scatter);
  rows    sgn_backlog into an array allocated once and touched beforehand; wall clock, the split
          again, and the device-to-host copy of the rows;
  old     sgn_host_digests(0, n) + sgn_stats_get — the nearest substitute there was (the per-host
          popped / delivered / dropped counters give the router backlog, the stats the packets in
          flight; nothing gave the send queue or the ages): wall clock around the two calls.
The report does not change the simulation and the old way changes nothing either, so the order
within a repeat changes nobody's work.

The calendar pass's algorithmic bytes: 32 B per run read plus the fill words it looks at (4 B per
(bucket, group) slab, 4 B per bucket's slab id per group), set against its HIP-event time as a share
of the HBM peak (8 TB/s, MI355X: the figure bench.py's roofline uses).
One JSON line per repeat and one summary line per config, appended to --out when given.

usage: python tools/backlog_timing.py [--configs C,D] [--repeats 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "shadow-gen_amd"))

import numpy as np  # noqa: E402

import sgn  # noqa: E402
from sample_timing import HBM_PEAK_BYTES_PER_S, median, world_of  # noqa: E402


def measure(config, a, emit):
    hosts = a.hosts or {"C": 100_000, "D": 1_000_000}[config]
    warmup = a.warmup or {"C": 300, "D": 50}[config]
    rounds = a.rounds or {"C": 100, "D": 10}[config]
    g, used, hst, cfg, tr = world_of(config, hosts, a.nodes, warmup, rounds, a.repeats)
    c = sgn.Context(device=0)
    c.routes_build(g, used)
    c.hosts_set(hst)
    c.sim_init(cfg, tr)
    c.run(warmup)
    L = c.L
    d = np.zeros(hosts, dtype=sgn.DIGEST_DTYPE)
    row_buf = np.zeros(hosts, dtype=sgn.BACKLOG_ROW_DTYPE)
    d["tx"] = 1
    row_buf["host"] = 1  # (the caller's pages are touched: see tools/sample_timing.py)
    stats, info, info_t = sgn.Stats(), sgn.BacklogInfo(), sgn.BacklogInfo()
    n_rows, n_tot = C.c_uint64(), C.c_uint64()
    split = {}

    def old():
        c.check(L.sgn_host_digests(c.h, 0, hosts, d.ctypes.data_as(C.POINTER(sgn.HostDigest))))
        c.check(L.sgn_stats_get(c.h, C.byref(stats)))

    def totals():
        c.check(L.sgn_backlog(c.h, None, 0, C.byref(n_tot), C.byref(info_t)))
        split["totals"] = c.backlog_timing()

    def rows():
        c.check(L.sgn_backlog(c.h, row_buf.ctypes.data_as(C.POINTER(sgn.BacklogRow)), hosts, C.byref(n_rows), C.byref(info)))
        split["rows"] = c.backlog_timing()

    sides = {"old": old, "totals": totals, "rows": rows}
    for f in sides.values():  # (nobody's first call is reported: code objects are loaded, scratch is allocated)
        f()
    ei = c.engine_info()
    G, NB = int(ei["host_groups"]), int(ei["calendar_buckets"])
    per = []
    for rep in range(a.repeats):
        assert c.run(rounds) == rounds, "the simulation ended inside the timed part: fewer --repeats or --rounds"
        res = {}
        order = list(sides)
        order = order[rep % 3:] + order[: rep % 3]
        for side in order:
            t0 = time.perf_counter()
            sides[side]()
            res[side + "_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
        st = stats.as_dict()
        tt, tr_ = split["totals"], split["rows"]
        assert n_tot.value == n_rows.value == int(info.rows) and list(info.total) == list(info_t.total)
        assert int(info.rounds) == st["rounds"] and int(info.total[6]) == st["packets_sent"] - st["packet_events_popped"]
        got = row_buf[: n_rows.value]
        held = int((got["flags"] & sgn.BACKLOG_ROUTER_HELD != 0).sum())
        assert int(got["router_packets"].sum()) + held == int((d["n_popped"] - d["n_delivered"] - d["n_codel_dropped"]).sum())
        cal_bytes = 32 * tt["calendar_runs"] + 4 * NB * G * 2
        res.update(case="repeat", config=config, rep=rep, rows=int(n_rows.value), rounds=st["rounds"],
                   calendar_runs=tt["calendar_runs"], inflight_packets=int(info.total[6]),
                   router_packets=int(info.total[0]), send_packets=int(info.total[3]),
                   max_router_packets=int(info.max_router_packets), max_sojourn_ms=round(int(info.max_sojourn_ns) / 1e6, 3),
                   totals_kernel_ms=[round(x, 4) for x in tt["kernel_ms"]], rows_kernel_ms=[round(x, 4) for x in tr_["kernel_ms"]],
                   rows_copy_ms=round(tr_["copy_ms"], 4), calendar_bytes=cal_bytes,
                   calendar_hbm_share=round(cal_bytes / (tt["kernel_ms"][0] * 1e-3) / HBM_PEAK_BYTES_PER_S, 4)
                   if tt["kernel_ms"][0] > 0 else None)
        emit(res)
        per.append(res)
    med = lambda k: median([r[k] for r in per])  # noqa: E731
    emit({"case": "summary", "config": config, "hosts": hosts, "repeats": a.repeats, "rounds_between": rounds,
          "host_groups": G, "calendar_buckets": NB,
          "totals_wall_ms_median": med("totals_wall_ms"), "rows_wall_ms_median": med("rows_wall_ms"),
          "old_wall_ms_median": med("old_wall_ms"),
          "totals_kernel_ms_median": [round(median([r["totals_kernel_ms"][k] for r in per]), 4) for k in range(4)],
          "rows_kernel_ms_median": [round(median([r["rows_kernel_ms"][k] for r in per]), 4) for k in range(4)],
          "rows_copy_ms_median": med("rows_copy_ms"), "rows_median": med("rows"), "calendar_runs_median": med("calendar_runs"),
          "calendar_bytes_median": med("calendar_bytes"),
          "calendar_hbm_share_median": median([r["calendar_hbm_share"] for r in per if r["calendar_hbm_share"] is not None] or [None]),
          "old_over_totals_median": round(median([r["old_wall_ms"] / r["totals_wall_ms"] for r in per]), 2)})
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C,D")
    ap.add_argument("--hosts", type=int, default=0, help="override the config's host count (a rehearsal)")
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=0, help="rounds before the first timed repeat (default: C 300, D 50)")
    ap.add_argument("--rounds", type=int, default=0, help="rounds between repeats (default: C 100, D 10)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(d):
        d = {"tool": "backlog_timing", "build_id": sgn.build_id(), **d}
        print(json.dumps(d), flush=True)
        lines.append(d)

    for config in a.configs.split(","):
        measure(config, a, emit)
    if a.out:
        with open(a.out, "a", encoding="utf-8") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
