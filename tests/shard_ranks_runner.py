"""One rank of tests/test_gpu_shard_ranks.py: a shard with an RCCL communicator on device 0.

    python shard_ranks_runner.py RANK WORLD DIR T_EMULATED

Rank 0 writes the communicator id to DIR/id.bin; the others wait for it (bounded). Every rank then
runs the console sequence through the collective calls with n = 1 — run-until T_EMULATED, save, run
to the end, restore, run to the end — and writes its part of the state after each step to
DIR/rank<R>.npz (window, counters, its hosts' digests). A refused sgn_shards_run_until ends the
rank with its error code in the file instead (the ranks-disagree case)."""
import os
import pathlib
import sys
import time

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent / "shadow-gen_amd"))
sys.path.insert(0, str(HERE))

import numpy as np  # noqa: E402

ID_WAIT_S = 60.0


def main():
    rank, world, out, t = int(sys.argv[1]), int(sys.argv[2]), pathlib.Path(sys.argv[3]), int(sys.argv[4])
    # several ranks on one GPU: RCCL accepts them as if on different hosts (bench.py --one-gpu)
    os.environ["NCCL_HOSTID"] = f"sgn-one-gpu-rank{rank}"
    os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
    os.environ.setdefault("NCCL_IB_DISABLE", "1")
    import sgn
    from test_gpu_snapshot import _until_args
    from test_gpu_xpersist import ADD, DIGESTS

    t_start = time.monotonic()
    (g, used, hosts, cfg, tr), _ = _until_args("periodic")
    n = hosts.n
    ctx = sgn.Context(device=0, shard_rank=rank, shard_count=world, flags=2)
    idb = (sgn.C.c_uint8 * 128)()
    idf = out / "id.bin"
    if rank == 0:
        ctx.check(ctx.L.sgn_comm_get_unique_id(idb))
        tmp = out / "id.tmp"
        tmp.write_bytes(bytes(idb))
        os.replace(tmp, idf)
    else:
        deadline = time.monotonic() + ID_WAIT_S
        while not idf.exists():
            if time.monotonic() > deadline:
                sys.exit("rank %d: no communicator id within %.0f s" % (rank, ID_WAIT_S))
            time.sleep(0.02)
        idb = (sgn.C.c_uint8 * 128)(*idf.read_bytes())
    ctx.check(ctx.L.sgn_comm_init(ctx.h, idb, 1 << 13))
    t_comm = time.monotonic() - t_start
    ctx.routes_build(g, used)
    ctx.hosts_set(hosts)
    ctx.sim_init(cfg, tr)
    lo, hi = sgn.C.c_uint32(), sgn.C.c_uint32()
    ctx.L.sgn_shard_range(n, rank, world, sgn.C.byref(lo), sgn.C.byref(hi))
    res = {"lo": lo.value, "hi": hi.value, "t_comm": t_comm}

    def dump(tag):
        w, st, d = ctx.window(), ctx.stats(), ctx.digests(lo.value, hi.value)
        res[tag + "_window"] = np.array([w[0], w[1], int(w[2])], dtype=np.uint64)
        res[tag + "_stats"] = np.array([st["rounds"]] + [st[k] for k in ADD], dtype=np.uint64)
        for f in DIGESTS:
            res[tag + "_" + f] = d[f]

    def finish(rc):
        info = ctx.engine_info()
        res["rc"] = rc
        res["exchange_mode"] = info["exchange_mode"]
        res["persistent_x_launches"] = info["persistent_x_launches"]
        res["t_total"] = time.monotonic() - t_start
        np.savez(out / f"rank{rank}.npz", **res)

    try:
        res["done_mid"] = sgn.shards_run_until([ctx], t)
    except sgn.SgnError as e:
        finish(e.rc)
        return
    dump("mid")
    snaps = sgn.shards_snapshot_save([ctx])
    res["snap_rounds"] = ctx.snapshot_info(snaps[0])["rounds"]
    ctx.run()
    dump("end1")
    sgn.shards_snapshot_restore([ctx], snaps)
    dump("back")
    ctx.run()
    dump("end2")
    finish(0)
    ctx.close()


if __name__ == "__main__":
    main()
