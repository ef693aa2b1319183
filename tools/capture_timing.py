#!/usr/bin/env python3
"""What a capture costs (one GPU): config C's workload at a size whose full trace fits a buffer.

1. Rounds per second of the same rounds run four ways: untraced with one launch per round
   (SGN_PERSISTENT=0: what a traced run is compared with, traced runs execute round by round), with
   a full trace, with a trace of 8 hosts (sgn_trace_hosts), and — with --parent-lib, a libsgn.so
   built from the parent commit — the parent's full trace.
   Every run warms up first, then times `--rounds` rounds `--repeats` times (wall clock around
   sgn_run, which ends in a stream synchronise); the traced runs take the trace between the timed
   windows, outside them.
2. sgn_trace_take of about `--take-records` pending records of the full trace: the HIP-event times
   of its three kernels, its device-to-host copies and the wall time of the call, beside
   sgn_trace_read of the same records (a plain device-to-host copy: what reading the trace cost
   before takes, without the sort the caller then does).
One JSON line per result, appended to --out when given.

usage: python tools/capture_timing.py [--hosts 20000] [--rounds 200] [--warmup 200] [--repeats 5]
                                      [--take-records 1000000] [--parent-lib PATH] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "shadow-gen_amd"))

import numpy as np  # noqa: E402

import bench  # noqa: E402
import sgn  # noqa: E402


def context(world, trace_cap=0, hosts=None, lib=None):
    g, used, hst, cfg, tr = world
    c = sgn.Context(device=0, lib=lib)
    c.routes_build(g, used)
    c.hosts_set(hst)
    if trace_cap:
        c.trace_enable(trace_cap)
    if hosts is not None:
        c.trace_hosts(hosts)
    c.sim_init(cfg, tr)
    return c


def rounds_per_s(c, warmup, rounds, repeats, traced):
    """Timed windows of `rounds` rounds; a traced run's buffer is emptied between them."""
    c.run(warmup)
    if traced:
        c.trace_take()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        done = c.run(rounds)
        dt = time.perf_counter() - t0
        assert done == rounds, done
        out.append(rounds / dt)
        if traced:
            c.trace_take()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hosts", type=int, default=20_000)
    ap.add_argument("--nodes", type=int, default=1000)
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--trace-cap", type=int, default=1 << 25)
    ap.add_argument("--take-records", type=int, default=1_000_000)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    world = bench.build_workload(a.hosts, a.nodes)
    lines = []

    def emit(d):
        d = {"tool": "capture_timing", "build_id": sgn.build_id(), "hosts": a.hosts, **d}
        print(json.dumps(d), flush=True)
        lines.append(d)

    def stats(v):
        v = sorted(v)
        return {"rounds_per_s_median": round(v[len(v) // 2], 1), "rounds_per_s_min": round(v[0], 1),
                "rounds_per_s_max": round(v[-1], 1)}

    eight = np.linspace(0, a.hosts - 1, 8).astype(np.uint32)
    os.environ["SGN_PERSISTENT"] = "0"
    for name, cap, hosts in [("untraced_per_round", 0, None), ("full_trace", a.trace_cap, None),
                             ("trace_8_hosts", a.trace_cap, eight)]:
        c = context(world, cap, hosts)
        v = rounds_per_s(c, a.warmup, a.rounds, a.repeats, traced=cap > 0)
        emit({"case": name, "rounds": a.rounds, "repeats": a.repeats, **stats(v)})
        c.close()
    if a.parent_lib:
        # The parent has no takes: one timed window per context, the buffer sized for warm-up and
        # window together — and this build measured the same way, the two alternating.
        cur = sgn.load()
        par = C.CDLL(a.parent_lib)
        for fn in ("sgn_create", "sgn_destroy", "sgn_last_error", "sgn_routes_build", "sgn_hosts_set", "sgn_trace_enable",
                   "sgn_sim_init", "sgn_run", "sgn_trace_read"):
            getattr(par, fn).restype = getattr(cur, fn).restype
            getattr(par, fn).argtypes = getattr(cur, fn).argtypes
        v = {"parent_full_trace": [], "full_trace_one_window": []}
        for _ in range(a.repeats):
            for name, lib in (("parent_full_trace", par), ("full_trace_one_window", cur)):
                c = context(world, a.trace_cap, None, lib)
                c.run(a.warmup)
                t0 = time.perf_counter()
                done = c.run(a.rounds)
                v[name].append(done / (time.perf_counter() - t0))
                c.close()
        for name, x in v.items():
            emit({"case": name, "rounds": a.rounds, "repeats": a.repeats, **stats(x)})

    # ---- the take ----
    c = context(world, a.trace_cap)
    c.run(a.warmup)
    c.trace_take()
    for rep in range(a.repeats + 1):  # (the first take allocates its scratch: not reported)
        while c.trace_pending() < a.take_records and c.window()[2]:
            c.run(4)
        n = c.trace_pending()
        buf = np.zeros(n, dtype=sgn.TRACE_DTYPE)
        tot = C.c_uint64()
        read_ms = []
        for _ in range(2):  # (the second read: the array's pages are touched)
            t0 = time.perf_counter()
            c.check(c.L.sgn_trace_read(c.h, buf.ctypes.data_as(C.POINTER(sgn.TraceRec)), n, C.byref(tot)))
            read_ms.append((time.perf_counter() - t0) * 1e3)
        recs = np.zeros(n, dtype=sgn.TRACE_DTYPE)
        spans = np.zeros(a.hosts, dtype=sgn.SPAN_DTYPE)
        recs["seq"] = 1  # (pages touched, like the read's array)
        spans["count"] = 1
        got, ns = C.c_uint64(), C.c_uint64()
        t0 = time.perf_counter()
        c.check(c.L.sgn_trace_take(c.h, recs.ctypes.data_as(C.POINTER(sgn.TraceRec)), n, C.byref(got),
                                   spans.ctypes.data_as(C.POINTER(sgn.TraceSpan)), a.hosts, C.byref(ns)))
        wall_ms = (time.perf_counter() - t0) * 1e3
        t = c.trace_take_timing()
        assert got.value == n and t["records"] == n and ns.value == t["hosts"]
        srt = buf[np.lexsort((buf["seq"], buf["host"]))]
        assert srt.tobytes() == recs.tobytes()  # (the take is the read, sorted)
        if rep == 0:
            continue
        emit({"case": "take", "records": n, "bytes": n * 56, "hosts_with_records": t["hosts"],
              "kernel_ms": [round(x, 4) for x in t["kernel_ms"]], "copy_ms": round(t["copy_ms"], 3),
              "take_call_ms": round(t["total_ms"], 3), "take_wall_ms_python": round(wall_ms, 3),
              "trace_read_ms": round(read_ms[1], 3)})
    c.close()
    if a.out:
        with open(a.out, "a", encoding="utf-8") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
