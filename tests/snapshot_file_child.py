"""Child process of test_gpu_snapshot_file.py::test_across_processes: builds test_gpu_parity's
scenario() in a process of its own, runs 150 rounds, saves, exports the snapshot to argv[1] and
exits 0. The parent imports the file into a context it builds itself: the two processes allocate
independently, so a device address or a process-local value hiding in the state or in the identity
digest cannot survive the trip.

usage: python snapshot_file_child.py OUT.snap"""
import pathlib
import sys

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent / "shadow-gen_amd"))
sys.path.insert(0, str(HERE.parent / "oracle"))


def main():
    import sgn
    from test_gpu_parity import scenario

    g, used, hosts, cfg, tr = scenario()
    c = sgn.Context()
    c.routes_build(g, used)
    c.hosts_set(hosts)
    c.sim_init(cfg, tr)
    assert c.run(150) == 150
    snap = c.snapshot_save()
    n = c.snapshot_export(snap, sys.argv[1])
    info = sgn.snapshot_file_info(sys.argv[1])
    assert info["file_bytes"] == n and info["rounds"] == 150, info
    c.close()
    print("exported", n, "bytes, identity", hex(info["identity"]))


if __name__ == "__main__":
    main()
