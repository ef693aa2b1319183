#!/usr/bin/env python3
"""What a per-host sample of a running simulation costs (one GPU), the old way and the new one, at
config C (100 k hosts, TGEN) and config D (1 M hosts, PERIODIC).

After a warm-up, `--repeats` times: run `--rounds` rounds (so that counters move), then on the same
context, alternating which comes first,
  old  sgn_host_digests(0, n) + sgn_stats_get — every host record to the CPU and a CPU fold, the
       only per-host reading there was; wall clock around the two calls (they end synchronised);
  new  sgn_sample + sgn_sample_take — wall clock around the two calls, and the HIP-event split of
       sgn_sample_timing_get (count, scan, scatter kernels; the take's device-to-host copy).
Both sides are called through the C ABI with arrays allocated once and touched beforehand.
The old way does not move the sampler's baseline and the new one does not change the simulation,
so the order within a repeat changes neither's work.

A sample's algorithmic bytes are computed here from the host count and the layout: both passes
(count, scatter) read per owned host its slot id (4 B), its seven counters (56 B) and its seven
baseline words (56 B); the scatter writes per changed host a row (64 B) and the baseline (56 B).
They are set against the three kernels' time as a share of the HBM peak (8 TB/s, MI355X).
One JSON line per repeat and one summary line per config, appended to --out when given.

usage: python tools/sample_timing.py [--configs C,D] [--repeats 5] [--out FILE]
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

import bench  # noqa: E402
import sgn  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12
PASS_BYTES_PER_HOST = 4 + 56 + 56  # slot id, counters, baseline: read by the count and by the scatter
ROW_BYTES = 64 + 56                # a changed host: its row and its baseline, written by the scatter


def world_of(config, hosts, nodes, warmup, rounds, repeats):
    if config == "C":
        return bench.build_workload(hosts, nodes)
    stop = max(1_000_000_000, (warmup + (rounds + 1) * (repeats + 2)) * 1_000_000)  # (1 ms per round)
    g, used, hst, cfg, tr = bench.build_workload_d(hosts, nodes, stop_ns=stop)
    cfg.event_capacity = 257 * -(-hosts // 64) * 128  # (the benchmark's calendar for D)
    return g, used, hst, cfg, tr


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def measure(config, a, emit):
    hosts = a.hosts or {"C": 100_000, "D": 1_000_000}[config]
    warmup = a.warmup or {"C": 300, "D": 50}[config]
    rounds = a.rounds or {"C": 100, "D": 10}[config]
    g, used, hst, cfg, tr = world_of(config, hosts, a.nodes, warmup, rounds, a.repeats)
    c = sgn.Context(device=0)
    c.routes_build(g, used)
    c.hosts_set(hst)
    c.sim_init(cfg, tr)
    c.sample_enable(hosts)
    c.run(warmup)
    # The caller's arrays are allocated once and their pages touched: a device-to-host copy into
    # fresh pageable memory pays the page faults (64 MB of rows: 200 ms against 5 ms), which is the
    # caller's allocation and not the call. Both sides go through the C ABI directly.
    L = c.L
    d = np.zeros(hosts, dtype=sgn.DIGEST_DTYPE)
    row_buf = np.zeros(hosts, dtype=sgn.SAMPLE_ROW_DTYPE)
    d["tx"] = 1
    row_buf["sent"] = 1
    stats, info, infos = sgn.Stats(), sgn.SampleInfo(), (sgn.SampleInfo * 4)()
    n_rows, n_infos = C.c_uint64(), C.c_uint64()

    def old():
        c.check(L.sgn_host_digests(c.h, 0, hosts, d.ctypes.data_as(C.POINTER(sgn.HostDigest))))
        c.check(L.sgn_stats_get(c.h, C.byref(stats)))

    def new():
        c.check(L.sgn_sample(c.h, C.byref(info)))
        c.check(L.sgn_sample_take(c.h, row_buf.ctypes.data_as(C.POINTER(sgn.SampleRow)), hosts, C.byref(n_rows), infos, 4,
                                  C.byref(n_infos)))

    old()  # (neither side's first call is reported: code objects are loaded)
    new()
    per = []
    for rep in range(a.repeats):
        assert c.run(rounds) == rounds, "the simulation ended inside the timed part: fewer --repeats or --rounds"
        res = {}
        for side in (("old", "new") if rep % 2 == 0 else ("new", "old")):
            t0 = time.perf_counter()
            (old if side == "old" else new)()
            res[side + "_wall_ms"] = (time.perf_counter() - t0) * 1e3
        t = c.sample_timing()
        st = stats.as_dict()
        rows = row_buf[: n_rows.value]
        info_rows, info_rounds = int(info.rows), int(info.rounds)
        assert len(rows) == info_rows == t["rows"] and t["hosts"] == hosts and n_infos.value == 1
        # (both readings are of the same round edge: the growth the rows report ends at the digests' totals)
        assert info_rounds == st["rounds"] and int(d["n_sent"].sum()) == st["packets_sent"]
        kernel_ms = sum(t["kernel_ms"])
        nbytes = 2 * PASS_BYTES_PER_HOST * hosts + ROW_BYTES * len(rows)
        res.update(case="repeat", config=config, rep=rep, rows=len(rows), rounds=st["rounds"],
                   sample_call_ms=round(t["total_ms"], 4), kernel_ms=[round(x, 4) for x in t["kernel_ms"]],
                   take_copy_ms=round(t["copy_ms"], 4), algorithmic_bytes=nbytes,
                   hbm_share=round(nbytes / (kernel_ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 4) if kernel_ms > 0 else None,
                   old_wall_ms=round(res["old_wall_ms"], 3), new_wall_ms=round(res["new_wall_ms"], 3))
        emit(res)
        per.append(res)
    emit({"case": "summary", "config": config, "hosts": hosts, "repeats": a.repeats, "rounds_between": rounds,
          "old_wall_ms_median": median([r["old_wall_ms"] for r in per]), "old_wall_ms_min": min(r["old_wall_ms"] for r in per),
          "new_wall_ms_median": median([r["new_wall_ms"] for r in per]), "new_wall_ms_max": max(r["new_wall_ms"] for r in per),
          "kernel_ms_median": round(median([sum(r["kernel_ms"]) for r in per]), 4),
          "take_copy_ms_median": median([r["take_copy_ms"] for r in per]),
          "rows_median": median([r["rows"] for r in per]),
          "hbm_share_median": median([r["hbm_share"] for r in per if r["hbm_share"] is not None] or [None]),
          "old_over_new_median": round(median([r["old_wall_ms"] / r["new_wall_ms"] for r in per]), 2)})
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
        d = {"tool": "sample_timing", "build_id": sgn.build_id(), **d}
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
