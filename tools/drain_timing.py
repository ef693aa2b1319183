#!/usr/bin/env python3
"""What taking the drain records of a paused EXTERNAL simulation costs (one GPU): sgn_drain_take
against the two ways sgn_drain is used.

Scenario: config C's graph and hosts (100 k hosts) with EXTERNAL traffic; `--datagrams` (1 M)
datagrams to unregistered addresses, spread over all hosts, are submitted and run until every one is
decided (each yields one UNKNOWN record at its sender), then a snapshot is saved. `--repeats` times,
in rotating order, each leg from a restore of that snapshot:
  single  sgn_drain(0, all hosts)                       — the range form, once;
  ranges  16 x sgn_drain over 16 equal host ranges      — the worker-thread pattern;
  take    sgn_drain_take with spans                      — and its HIP-event split.
All three write into arrays allocated once and touched beforehand, through the C ABI. The legs'
outputs are compared (the same bytes). sgn_drain is the code of the parent commit: the baseline.

Skewed case: the ordering kernels alone (sgn_selftest_drain_order) on as many records with one
host holding `--skew` (200 k) of them, so the tile-and-merge path runs at scale.

The order stage is set against the HBM peak (8 TB/s, the figure bench.py's roofline uses): every
record is read and written once by its class's kernel, and once more per merge pass for the
records of the large segments (48 B each way).
One JSON line per repeat and summary lines, appended to --out when given.

usage: python tools/drain_timing.py [--hosts 100000] [--datagrams 1000000] [--repeats 5] [--out FILE]
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
from sample_timing import HBM_PEAK_BYTES_PER_S, median  # noqa: E402

REC = 48


def order_bytes(t):
    """Bytes the order stage moves for the timing dict t (an upper bound for the merge passes: every
    large segment is charged the passes of the largest)."""
    passes, w = 0, t["tile"]
    while w < t["largest_span"]:
        passes, w = passes + 1, w * 2
    passes += passes & 1
    return 2 * REC * t["records"], passes


def hbm_share(nbytes, ms):
    return round(nbytes / (ms * 1e-3) / HBM_PEAK_BYTES_PER_S, 4) if ms > 0 else None


def simulation(a, emit):
    g, used, hst, cfg, _ = bench.build_workload(a.hosts, a.nodes)
    tr = sgn.make_traffic(sgn.TRAFFIC_EXTERNAL)
    c = sgn.Context(device=0)
    c.routes_build(g, used)
    c.hosts_set(hst)
    k = a.datagrams
    c.drain_enable(max(1 << 20, 2 * k))
    c.sim_init(cfg, tr)
    info = c.engine_info()
    horizon = (info["calendar_buckets"] - 2) * info["bucket_width_ns"]
    rng = np.random.default_rng(1)
    src = rng.integers(0, a.hosts, k).astype(np.uint32)
    t = sgn.SIMULATION_START + np.sort(rng.integers(0, min(50_000_000, horizon // 2), k)).astype(np.uint64)
    c.submit(src, np.full(k, 0x0AFF0001, np.uint32), np.full(k, 100, np.uint32), t, np.arange(1, k + 1, dtype=np.uint64))
    rounds = c.run()
    n = c.drain_pending()
    assert n == k, (n, k)
    snap = c.snapshot_save()
    L = c.L
    bufs = {s: np.ones(n + 16, dtype=sgn.DRAIN_DTYPE) for s in ("single", "ranges", "take")}  # (pages touched)
    spans = np.ones(a.hosts, dtype=sgn.SPAN_DTYPE)
    got, n_spans = C.c_uint64(), C.c_uint64()
    ptr = lambda b, off=0: C.cast(b.ctypes.data + off * REC, C.POINTER(sgn.DrainRec))  # noqa: E731
    split = {}

    def single():
        c.check(L.sgn_drain(c.h, 0, a.hosts, ptr(bufs["single"]), n, C.byref(got)))
        assert got.value == n

    def ranges():
        at = 0
        for r in range(16):
            lo, hi = a.hosts * r // 16, a.hosts * (r + 1) // 16
            c.check(L.sgn_drain(c.h, lo, hi, ptr(bufs["ranges"], at), n - at, C.byref(got)))
            at += got.value
        assert at == n

    def take():
        c.check(L.sgn_drain_take(c.h, ptr(bufs["take"]), n, C.byref(got), spans.ctypes.data_as(C.POINTER(sgn.TraceSpan)),
                                 a.hosts, C.byref(n_spans)))
        assert got.value == n
        split["take"] = c.drain_take_timing()

    legs = {"single": single, "ranges": ranges, "take": take}
    for f in legs.values():  # (nobody's first call is reported: code objects are loaded, scratch is allocated)
        c.snapshot_restore(snap)
        f()
    assert bufs["single"][:n].tobytes() == bufs["ranges"][:n].tobytes() == bufs["take"][:n].tobytes()
    per = []
    for rep in range(a.repeats):
        res = {}
        order = list(legs)
        order = order[rep % 3:] + order[: rep % 3]
        for leg in order:
            c.snapshot_restore(snap)
            t0 = time.perf_counter()
            legs[leg]()
            res[leg + "_wall_ms"] = round((time.perf_counter() - t0) * 1e3, 4)
        tt = split["take"]
        nbytes, passes = order_bytes(tt)
        res.update(case="repeat", rep=rep, records=n, hosts_with_records=int(n_spans.value), rounds=rounds,
                   take_kernel_ms=[round(x, 4) for x in tt["kernel_ms"]], take_copy_ms=round(tt["copy_ms"], 4),
                   spans_by_class=tt["spans_by_class"], largest_span=tt["largest_span"], order_bytes=nbytes,
                   order_hbm_share=hbm_share(nbytes, tt["kernel_ms"][3]))
        emit(res)
        per.append(res)
    med = lambda key: median([r[key] for r in per])  # noqa: E731
    rng_ = lambda key: [min(r[key] for r in per), max(r[key] for r in per)]  # noqa: E731
    emit({"case": "summary", "hosts": a.hosts, "records": n, "repeats": a.repeats,
          "single_wall_ms_median": med("single_wall_ms"), "single_wall_ms_range": rng_("single_wall_ms"),
          "ranges_wall_ms_median": med("ranges_wall_ms"), "ranges_wall_ms_range": rng_("ranges_wall_ms"),
          "take_wall_ms_median": med("take_wall_ms"), "take_wall_ms_range": rng_("take_wall_ms"),
          "take_kernel_ms_median": [round(median([r["take_kernel_ms"][i] for r in per]), 4) for i in range(4)],
          "take_copy_ms_median": med("take_copy_ms"), "spans_by_class": per[-1]["spans_by_class"],
          "largest_span": per[-1]["largest_span"],
          "order_hbm_share_median": median([r["order_hbm_share"] for r in per if r["order_hbm_share"] is not None] or [None])})
    c.snapshot_free(snap)
    c.close()


def skewed(a, emit):
    n, big = a.datagrams, min(a.skew, a.datagrams)
    rng = np.random.default_rng(2)
    recs = np.zeros(n, dtype=sgn.DRAIN_DTYPE)
    host = rng.integers(0, a.hosts, n).astype(np.uint32)
    host[rng.choice(n, big, replace=False)] = a.hosts // 3
    recs["host"] = host
    recs["time"] = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    recs["src_host"] = rng.integers(0, a.hosts, n)
    recs["src_eid"] = rng.permutation(n)
    recs["tag"] = rng.integers(0, 1 << 29, n)
    recs["handle"] = np.arange(n)
    exp = recs[np.lexsort([recs[f] for f in ("status", "tag", "src_eid", "src_host", "time", "host")])]
    c = sgn.Context(device=0)
    per = []
    for rep in range(a.repeats + 1):
        t0 = time.perf_counter()
        out, spans = sgn.selftest_drain_order(c, recs, 0, a.hosts)
        wall = (time.perf_counter() - t0) * 1e3
        assert out.tobytes() == exp.tobytes()
        if rep == 0:
            continue  # (the first call allocates the scratch)
        tt = c.drain_take_timing()
        nbytes, passes = order_bytes(tt)
        nbytes += 2 * REC * tt["largest_span"] * passes
        res = dict(case="skewed", rep=rep - 1, records=n, hosts_with_records=len(spans), wall_ms=round(wall, 4),
                   kernel_ms=[round(x, 4) for x in tt["kernel_ms"]], copy_ms=round(tt["copy_ms"], 4),
                   spans_by_class=tt["spans_by_class"], largest_span=tt["largest_span"], merge_passes=passes,
                   order_bytes=nbytes, order_hbm_share=hbm_share(nbytes, tt["kernel_ms"][3]))
        emit(res)
        per.append(res)
    emit({"case": "skewed-summary", "records": n, "largest_span": per[-1]["largest_span"], "merge_passes": per[-1]["merge_passes"],
          "spans_by_class": per[-1]["spans_by_class"],
          "kernel_ms_median": [round(median([r["kernel_ms"][i] for r in per]), 4) for i in range(4)],
          "copy_ms_median": median([r["copy_ms"] for r in per]),
          "order_hbm_share_median": median([r["order_hbm_share"] for r in per if r["order_hbm_share"] is not None] or [None])})
    c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=100_000)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--datagrams", type=int, default=1_000_000)
    ap.add_argument("--skew", type=int, default=200_000, help="records of the one large host of the skewed case")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(d):
        d = {"tool": "drain_timing", "build_id": sgn.build_id(), **d}
        print(json.dumps(d), flush=True)
        lines.append(d)

    simulation(a, emit)
    skewed(a, emit)
    if a.out:
        with open(a.out, "a", encoding="utf-8") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
