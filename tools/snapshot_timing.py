#!/usr/bin/env python3
"""What a snapshot costs at bench.py's default sizes (one GPU): for configs C and D, one JSON
line each with the save and restore times, the snapshot's size, the packed-copy rate of the
calendar, the time a raw device-to-device copy of the unpacked calendar takes in the same process
(what a snapshot without packing would pay for the calendar alone), and the only way back there
was before snapshots: sgn_sim_init + sgn_run to the same round.

usage: python tools/snapshot_timing.py [--workload C D] [--rounds 1500] [--shards N] [--out FILE]
                                       [--export DIR]
The save is taken after bench.py's warm-up + steps worth of rounds (5 + 10 steps of 100).
--shards N: the same hosts as N shards of one local group on this GPU, saved and restored with
the collective calls (sgn_shards_snapshot_*): per-shard save times (their maximum and their sum:
the shards save one after the other) and the wall time of the group's save and restore.
--export DIR: snapshot files instead. The snapshot goes to DIR/<workload>.snap (the second export is
timed: the staging chunks are pinned by then) and into a FRESH context of the same simulation
(import, then restore): wall times, the digest kernel's time and rate over the device sections at
export and at import, and in the same process a device-to-device copy and the pinned-host
transfers of the same bytes. The lines are appended to profiles/snapshot_timing.jsonl."""
import argparse
import ctypes as C
import json
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "shadow-gen_amd"))

import torch  # noqa: E402

import bench  # noqa: E402
import sgn  # noqa: E402


def workload(name, rounds):
    if name == "C":
        return bench.build_workload(100_000, 1000)
    n = 1_000_000
    g, used, hosts, cfg, tr = bench.build_workload_d(n, 1000, stop_ns=max(1_000_000_000, (rounds + 100) * 1_000_000))
    cfg.event_capacity = 257 * (-(-n // 64)) * 128  # bench.py's slabs for D
    return g, used, hosts, cfg, tr


def raw_copy_ms(nbytes):
    """A device-to-device copy of nbytes (the second of two: the first touches the pages)."""
    a = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    b = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    a.zero_()
    b.copy_(a)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1)
    del a, b
    torch.cuda.empty_cache()
    return ms


def measure(name, rounds):
    g, used, hosts, cfg, tr = workload(name, rounds)
    c = sgn.Context(device=0)
    c.routes_build(g, used)
    c.hosts_set(hosts)
    c.sim_init(cfg, tr)
    done = c.run(rounds)
    w = c.window()
    snap = c.snapshot_save()
    c.snapshot_free(snap)
    snap = c.snapshot_save()  # (the second save: allocations and code objects warm)
    info = c.snapshot_info(snap)
    c.run(200)
    t0 = time.perf_counter()
    c.snapshot_restore(snap)  # (synchronises its stream before it returns)
    restore_ms = (time.perf_counter() - t0) * 1e3
    assert c.window() == w and c.stats()["rounds"] == done
    eng = c.engine_info()
    c.snapshot_free(snap)
    raw_ms = raw_copy_ms(info["calendar_pool_bytes"])
    t0 = time.perf_counter()
    c.sim_init(cfg, tr)
    init_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    c.run(done)
    assert c.window() == w
    rerun_ms = (time.perf_counter() - t0) * 1e3
    c.close()
    return {
        "tool": "snapshot_timing", "build_id": sgn.build_id(), "workload": name, "hosts": hosts.n,
        "rounds_at_save": done, "save_ms": round(info["save_ms"], 3), "pack_ms": round(info["pack_ms"], 3),
        "restore_wall_ms": round(restore_ms, 3), "device_bytes": info["device_bytes"],
        "host_bytes": info["host_bytes"], "calendar_runs": info["calendar_runs"],
        "calendar_bytes": info["calendar_bytes"], "calendar_pool_bytes": info["calendar_pool_bytes"],
        "pack_gb_per_s": round(info["calendar_bytes"] / max(info["pack_ms"], 1e-6) / 1e6, 2),
        "raw_pool_copy_ms": round(raw_ms, 3),
        "raw_pool_copy_gb_per_s": round(info["calendar_pool_bytes"] / max(raw_ms, 1e-6) / 1e6, 2),
        "reinit_ms": round(init_ms, 1), "rerun_ms": round(rerun_ms, 1),
        "slab_capacity": eng["slab_capacity"], "sim_device_bytes": eng["device_bytes"],
    }


def pinned_copy_ms(nbytes, to_host):
    """nbytes between the device and pinned host memory, in pieces of a 256 MiB pinned buffer (the
    second pass is timed)."""
    piece = min(nbytes, 256 << 20)
    dev = torch.empty(piece, dtype=torch.uint8, device="cuda").zero_()
    host = torch.empty(piece, dtype=torch.uint8).pin_memory()
    ms = 0.0
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        left = nbytes
        while left > 0:
            k = min(left, piece)
            if to_host:
                host[:k].copy_(dev[:k], non_blocking=True)
            else:
                dev[:k].copy_(host[:k], non_blocking=True)
            left -= k
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
    del dev, host
    torch.cuda.empty_cache()
    return ms


def measure_export(name, rounds, out_dir):
    g, used, hosts, cfg, tr = workload(name, rounds)

    def fresh():
        c = sgn.Context(device=0)
        c.routes_build(g, used)
        c.hosts_set(hosts)
        c.sim_init(cfg, tr)
        return c

    c = fresh()
    done = c.run(rounds)
    w = c.window()
    snap = c.snapshot_save()
    info = c.snapshot_info(snap)
    path = pathlib.Path(out_dir) / f"{name}.snap"
    c.snapshot_export(snap, path)  # (the first export pins the staging chunks)
    path.unlink()  # (or the timed export's rename pays for freeing this file's pages)
    t0 = time.perf_counter()
    nbytes = c.snapshot_export(snap, path)
    export_ms = (time.perf_counter() - t0) * 1e3
    te = c.snapshot_file_timing()
    c.close()
    c = fresh()  # never ran a round: its pools stand at their initial sizes
    s0 = c.snapshot_import(path)
    c.snapshot_free(s0)
    t0 = time.perf_counter()
    s1 = c.snapshot_import(path)
    import_ms = (time.perf_counter() - t0) * 1e3
    ti = c.snapshot_file_timing()
    t0 = time.perf_counter()
    c.snapshot_restore(s1)
    restore_ms = (time.perf_counter() - t0) * 1e3
    assert c.window() == w and c.stats()["rounds"] == done
    c.close()
    path.unlink()
    dev = te["device_bytes"]
    d2d_ms = raw_copy_ms(dev)
    d2h_ms, h2d_ms = pinned_copy_ms(dev, True), pinned_copy_ms(dev, False)
    rate = lambda b, ms: round(b / max(ms, 1e-6) / 1e6, 2)  # noqa: E731 (GB/s)
    return {
        "tool": "snapshot_timing_export", "build_id": sgn.build_id(), "workload": name, "hosts": hosts.n,
        "rounds_at_save": done, "file_bytes": nbytes, "device_section_bytes": dev,
        "snapshot_device_bytes": info["device_bytes"], "calendar_runs": info["calendar_runs"],
        "export_wall_ms": round(export_ms, 3), "export_call_ms": round(te["total_ms"], 3), "export_stream_ms": round(te["stream_ms"], 3),
        "export_digest_ms": round(te["digest_ms"], 4), "export_digest_gb_per_s": rate(dev, te["digest_ms"]),
        "import_wall_ms": round(import_ms, 3), "import_call_ms": round(ti["total_ms"], 3), "import_stream_ms": round(ti["stream_ms"], 3),
        "import_digest_ms": round(ti["digest_ms"], 4), "import_digest_gb_per_s": rate(ti["device_bytes"], ti["digest_ms"]),
        "restore_wall_ms": round(restore_ms, 3),
        "d2d_copy_ms": round(d2d_ms, 4), "d2d_copy_gb_per_s": rate(dev, d2d_ms),
        "pinned_d2h_ms": round(d2h_ms, 3), "pinned_d2h_gb_per_s": rate(dev, d2h_ms),
        "pinned_h2d_ms": round(h2d_ms, 3), "pinned_h2d_gb_per_s": rate(dev, h2d_ms),
        "export_digest_share": round(te["digest_ms"] / max(export_ms, 1e-6), 5),
        "import_digest_share": round(ti["digest_ms"] / max(import_ms, 1e-6), 5),
    }


def measure_group(name, rounds, k):
    g, used, hosts, cfg, tr = workload(name, rounds)
    cfg = type(cfg).from_buffer_copy(cfg)
    cfg.event_capacity = -(-cfg.event_capacity // k)  # (the calendar is sized per shard)
    shards = [sgn.Context(device=0, shard_rank=r, shard_count=k) for r in range(k)]
    arr = (C.c_void_p * k)(*[c.h.value for c in shards])
    for c in shards:
        c.routes_build(g, used)
        c.hosts_set(hosts)
    shards[0].check(shards[0].L.sgn_comm_init_local(arr, k, 1 << 13))
    for c in shards:
        c.sim_init(cfg, tr)

    def run(nr):
        d = C.c_uint64()
        shards[0].check(shards[0].L.sgn_run_local_group(arr, k, nr, C.byref(d)))
        return d.value

    done = run(rounds)
    w = shards[0].window()
    for c, s in zip(shards, sgn.shards_snapshot_save(shards)):
        c.snapshot_free(s)
    t0 = time.perf_counter()
    snaps = sgn.shards_snapshot_save(shards)  # (the second save: allocations and code objects warm)
    save_wall_ms = (time.perf_counter() - t0) * 1e3
    infos = [c.snapshot_info(s) for c, s in zip(shards, snaps)]
    run(200)
    t0 = time.perf_counter()
    sgn.shards_snapshot_restore(shards, snaps)
    restore_ms = (time.perf_counter() - t0) * 1e3
    assert all(c.window() == w and c.stats()["rounds"] == done for c in shards)
    eng = [c.engine_info() for c in shards]
    for c, s in zip(shards, snaps):
        c.snapshot_free(s)
    for c in shards:
        c.close()
    return {
        "tool": "snapshot_timing", "build_id": sgn.build_id(), "workload": name, "hosts": hosts.n, "shards": k,
        "rounds_at_save": done, "save_ms_max": round(max(i["save_ms"] for i in infos), 3),
        "save_ms_sum": round(sum(i["save_ms"] for i in infos), 3),
        "pack_ms_sum": round(sum(i["pack_ms"] for i in infos), 3), "save_wall_ms": round(save_wall_ms, 3),
        "restore_wall_ms": round(restore_ms, 3), "device_bytes": sum(i["device_bytes"] for i in infos),
        "calendar_runs": sum(i["calendar_runs"] for i in infos),
        "calendar_bytes": sum(i["calendar_bytes"] for i in infos),
        "calendar_pool_bytes": sum(i["calendar_pool_bytes"] for i in infos),
        "exchange_mode": eng[0]["exchange_mode"], "inbox_slot_runs": eng[0]["inbox_slot_runs"],
        "sim_device_bytes": sum(e["device_bytes"] for e in eng),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", nargs="+", choices=("C", "D"), default=["C", "D"])
    ap.add_argument("--rounds", type=int, default=1500)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shards", type=int, default=1)
    ap.add_argument("--export", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.export:
        lines = [json.dumps(measure_export(w, args.rounds, args.export)) for w in args.workload]
        with open(ROOT / "profiles" / "snapshot_timing.jsonl", "a") as f:
            f.write("\n".join(lines) + "\n")
    elif args.shards > 1:
        lines = [json.dumps(measure_group(w, args.rounds, args.shards)) for w in args.workload]
    else:
        lines = [json.dumps(measure(w, args.rounds)) for w in args.workload]
    for ln in lines:
        print(ln, flush=True)
    if args.out:
        pathlib.Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
