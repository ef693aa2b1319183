"""Snapshot files (-m gpu): a snapshot exported to a file and imported into a FRESH context — one
that never ran the rounds before the save, whose pools stand at their initial sizes, in the same
or in another process — restores to exactly the saved state and runs on to the oracle's end state.

As in test_gpu_snapshot, every run is compared with the oracle's ONE uninterrupted run of the
scenario (test_gpu_snapshot.ref_run's module cache). The file is input: the refusal cases hand
import files of another simulation and damaged files, and check that nothing changed.
"""
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import sgn
from external_common import datagrams, drive_ahead, external_world
from test_abi_snapshot_file import np_digest
from test_gpu_parity import assert_same_run, ctxf, scenario  # noqa: F401 (ctxf: fixture)
from test_gpu_pools import _codel_args, _hot_args
from test_gpu_shard_control import assert_merged, group, merged, run_group
from test_gpu_snapshot import assert_state, make_ctx, ref_run, state

pytestmark = pytest.mark.gpu

EINVAL, ESTATE, EFILE = -22, -71, -74
MS = 1_000_000
HDR = sgn.SNAPSHOT_HEADER_BYTES


def refused(rc, match, call):
    with pytest.raises(sgn.SgnError, match=match) as e:
        call()
    assert e.value.rc == rc, (e.value.rc, str(e.value))


@pytest.fixture(scope="module")
def exported(ctxf, tmp_path_factory):  # noqa: F811
    """scenario() after 150 rounds, exported once: the file the damaged copies are made from."""
    args = scenario()
    n = args[2].n
    c = make_ctx(ctxf, args)
    assert c.run(150) == 150
    at = state(c, n)
    snap = c.snapshot_save()
    path = tmp_path_factory.mktemp("snapfile") / "periodic150.snap"
    nbytes = c.snapshot_export(snap, path)
    assert not pathlib.Path(str(path) + ".tmp").exists()
    info = c.snapshot_info(snap)
    c.close()
    return {"args": args, "n": n, "path": path, "at": at, "bytes": nbytes, "info": info}


# ---- 1. the digest kernel ----
@pytest.mark.parametrize("n", [0, 4, 8, 12, 16, 20, 1020, 1024, 1028, 64 * 1024 + 4, 4 * 1024 * 1024 + 12])
def test_digest_kernel_matches_host(ctxf, n):  # noqa: F811
    """Every tail (0 / 4 / 8 / 12 bytes), less than one wave's pass, one workgroup, and a section
    its grid walks more than once; the host form is checked against numpy in the CPU suite."""
    b = np.random.default_rng(n + 1).integers(0, 256, n, dtype=np.uint8)
    c = ctxf()
    want = sgn.digest_bytes(b)
    assert c.selftest_digest(b) == want
    if n <= 64 * 1024 + 4:
        assert want == np_digest(b.tobytes())
    if n >= 16:  # one changed byte anywhere changes it
        b2 = b.copy()
        b2[n - 1] ^= 1
        assert c.selftest_digest(b2) == sgn.digest_bytes(b2) != want
    c.close()


def test_section_digests_are_of_the_bytes_in_the_file(exported):
    path = exported["path"]
    fi = sgn.snapshot_file_info(path)
    assert fi["file_bytes"] == exported["bytes"] == path.stat().st_size
    assert fi["rounds"] == 150 and (fi["window_start"], fi["window_end"]) == exported["at"][0][:2], fi
    assert fi["calendar_runs"] == exported["info"]["calendar_runs"] > 0 and fi["trace_records"] == 0, fi
    assert (fi["abi"], fi["shard_rank"], fi["shard_count"]) == (10, 0, 1), fi
    raw = path.read_bytes()
    assert raw[:8] == b"SGNSNAP1"
    secs = sgn.snapshot_file_sections(path)
    assert [s["name"] for s in secs] == list(sgn.SNAPSHOT_SECTION_NAMES)
    for s in secs:
        assert s["offset"] % 16 == 0
        assert s["digest"] == np_digest(raw[s["offset"]:s["offset"] + s["bytes"]]), s["name"]
    by = {s["name"]: s for s in secs}
    assert by["calendar"]["bytes"] == 32 * fi["calendar_runs"] and by["hrec"]["bytes"] == 512 * exported["n"]
    end = secs[-1]["offset"] + (secs[-1]["bytes"] + 15) // 16 * 16
    assert end + 8 == len(raw)
    assert int.from_bytes(raw[end:], "little") == np_digest(raw[:HDR + 24 * len(secs)])  # the trailer


# ---- 2. round trip into a fresh context, PERIODIC ----
@pytest.mark.parametrize("persistent,trace", [("1", False), ("0", False), ("1", True), ("0", True)])
def test_round_trip_periodic(ctxf, oracle, monkeypatch, tmp_path, persistent, trace):  # noqa: F811
    monkeypatch.setenv("SGN_PERSISTENT", persistent)
    args = scenario()
    n = args[2].n
    o = ref_run(oracle, "periodic", args, trace=True)
    c = make_ctx(ctxf, args, trace=trace)
    assert c.run(150) == 150
    at = state(c, n)
    snap = c.snapshot_save()
    saved = c.snapshot_info(snap)
    path = tmp_path / "a.snap"
    nbytes = c.snapshot_export(snap, path)
    assert_state(state(c, n), at, "after export")  # an export changes nothing
    c.run()
    end = state(c, n)
    assert_same_run(o, c, n, trace=trace)
    c.close()
    fi = sgn.snapshot_file_info(path)
    assert fi["file_bytes"] == nbytes and (fi["trace_records"] > 0) == trace, fi
    # a context that never saw the first 150 rounds
    c2 = make_ctx(ctxf, args, trace=trace)
    fresh = state(c2, n)
    snap2 = c2.snapshot_import(path)
    assert_state(state(c2, n), fresh, "an import only creates a snapshot")
    info = c2.snapshot_info(snap2)
    for k in ("rounds", "window_start", "window_end", "calendar_runs", "calendar_bytes", "calendar_pool_bytes"):
        assert info[k] == saved[k], (k, info[k], saved[k])
    assert info["save_ms"] == 0 and info["pack_ms"] == 0 and info["device_bytes"] >= saved["device_bytes"], info
    c2.snapshot_restore(snap2)
    assert_state(state(c2, n), at, "after restore")
    c2.run()
    assert_state(state(c2, n), end, "run on")
    assert_same_run(o, c2, n, trace=trace)  # (traced: the whole trace — the first 150 rounds' records came from the file)
    assert (c2.engine_info()["persistent_grid"] > 0) == (persistent == "1" and not trace)
    c2.close()


# ---- 3. layouts a fresh context does not have ----
@pytest.mark.parametrize("kind", ["codel", "hot"])
def test_round_trip_grown_pools(ctxf, oracle, monkeypatch, tmp_path, kind):  # noqa: F811
    keys = ("codel_pages", "slab_capacity", "slab_extensions", "slab_extension_runs", "codel_pool_grows",
            "calendar_grows", "codel_page_allocs", "rounds_held", "calendar_spill_runs", "spill_area_grows")
    if kind == "codel":
        args = _codel_args(n=300)
        saved_when = lambda i, s: i["codel_pool_grows"] >= 1  # noqa: E731
    else:
        monkeypatch.setenv("SGN_SLAB_CAP", "16")
        monkeypatch.setenv("SGN_SLAB_LIM", "32")
        args = _hot_args(1200)
        saved_when = lambda i, s: (i["slab_extensions"] > 0 or i["calendar_grows"] > 0) and s["calendar_runs"] > 0  # noqa: E731
    n = args[2].n
    o = ref_run(oracle, kind, args)
    c = make_ctx(ctxf, args)
    init = c.engine_info()
    snap, i0 = None, None
    for _ in range(200):
        assert c.run(1) == 1
        i0 = c.engine_info()
        if saved_when(i0, {"calendar_runs": 1}):
            snap = c.snapshot_save()
            if saved_when(i0, c.snapshot_info(snap)):
                break
            c.snapshot_free(snap)
            snap = None
    assert snap is not None, i0
    assert any(i0[k] != init[k] for k in ("codel_pages", "slab_capacity", "slab_extensions")), (init, i0)
    at = state(c, n)
    path = tmp_path / (kind + ".snap")
    c.snapshot_export(snap, path)
    c.run()
    assert_same_run(o, c, n, trace=False)
    c.close()
    c2 = make_ctx(ctxf, args)  # its pools stand at their initial sizes
    for k in ("codel_pages", "slab_capacity", "slab_extensions"):
        assert c2.engine_info()[k] == init[k]
    c2.snapshot_restore(c2.snapshot_import(path))
    i2 = c2.engine_info()
    for k in keys:
        assert i2[k] == i0[k], (k, i2[k], i0[k])
    assert_state(state(c2, n), at, "after restore")
    c2.run()
    assert_same_run(o, c2, n, trace=False)
    c2.close()


# ---- 4. EXTERNAL traffic: drain records on the device and held, handles, a CPU-held RNG state ----
def test_round_trip_external(ctxf, oracle, tmp_path):  # noqa: F811
    world = external_world()
    g, used, hosts, cfg, tr = world
    n = hosts.n
    dg = datagrams(hosts)

    def fresh():
        c = ctxf()
        c.routes_build(g, used)
        c.hosts_set(hosts)
        c.drain_enable(1 << 16)
        c.sim_init(cfg, tr)
        return c

    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr)
    c = fresh()
    log = {}
    # stop after step 4: the last drain was at step 3, and step 4 drew from a host RNG on the CPU
    (_, d0), _ = drive_ahead([o, c], dg, 7 * MS, stop_step=4, log=log)  # (step 3's drains: the caller's)
    nxt = log["nxt"]
    assert 0 < nxt < len(dg[3])
    # the records of hosts [0, 30) leave; the drain holds the others' for a later call
    po, pc = o.drain(0, 30), c.drain(0, 30)
    assert len(pc) > 0 and all(np.array_equal(po[f], pc[f]) for f in sgn.DRAIN_DTYPE.names)
    at = state(c, n)
    snap = c.snapshot_save()
    path = tmp_path / "ext.snap"
    c.snapshot_export(snap, path)
    secs = {s["name"]: s for s in sgn.snapshot_file_sections(path)}
    assert secs["drain_held"]["bytes"] > 0 and secs["handles"]["bytes"] > 0 and secs["submit_seq"]["bytes"] == 4 * n, secs
    c.close()
    c2 = fresh()
    c2.snapshot_restore(c2.snapshot_import(path))
    assert_state(state(c2, n), at, "after restore")
    # the oracle's uninterrupted drive goes on; the fresh context resumes beside it
    log1 = {}
    (do, dc), rounds = drive_ahead([o, c2], dg, 7 * MS, k0=4, nxt0=nxt, log=log1)
    assert rounds > 50 and log1["finished"] and log1["draws"][0] == log1["draws"][1]
    assert len(do) == len(dc) and len(d0) + len(pc) + len(dc) == len(dg[3])  # one record per datagram in all
    for f in sgn.DRAIN_DTYPE.names:  # (handles included)
        assert np.array_equal(do[f], dc[f]), f
    assert np.count_nonzero(dc["handle"]) > 0
    assert_same_run(o, c2, n, trace=False)
    c2.close()


# ---- 5. sharded: a local group of two ----
def test_round_trip_sharded(oracle, tmp_path):
    args = scenario()
    n = args[2].n
    o = ref_run(oracle, "periodic", args, trace=True)
    shards, arr = group(args, 2)
    assert run_group(shards, arr, 150) == 150
    at = merged(shards, n)
    snaps = sgn.shards_snapshot_save(shards)
    paths = [tmp_path / f"shard{r}.snap" for r in range(2)]
    for c, s, p in zip(shards, snaps, paths):
        c.snapshot_export(s, p)
    infos = [sgn.snapshot_file_info(p) for p in paths]
    assert [(i["shard_rank"], i["shard_count"]) for i in infos] == [(0, 2), (1, 2)]
    assert infos[0]["identity"] != infos[1]["identity"] and infos[0]["rounds"] == infos[1]["rounds"] == 150
    for c in shards:
        c.close()
    shards, arr = group(args, 2)
    refused(EINVAL, "header field", lambda: shards[1].snapshot_import(paths[0]))  # shard 0's file into shard 1
    snaps = [c.snapshot_import(p) for c, p in zip(shards, paths)]  # (per shard: no collective)
    sgn.shards_snapshot_restore(shards, snaps)
    assert_merged(merged(shards, n), at, "after restore")
    run_group(shards, arr)
    assert_merged(merged(shards, n), state(o, n), "end")
    for c in shards:
        c.close()


# ---- 6. across processes ----
def test_across_processes(ctxf, oracle, tmp_path):  # noqa: F811
    args = scenario()
    n = args[2].n
    o = ref_run(oracle, "periodic", args, trace=True)
    path = tmp_path / "child.snap"
    child = pathlib.Path(__file__).resolve().parent / "snapshot_file_child.py"
    # (a fresh process, before this test creates its context)
    r = subprocess.run([sys.executable, str(child), str(path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert sgn.snapshot_file_info(path)["rounds"] == 150
    c = make_ctx(ctxf, args)
    c.snapshot_restore(c.snapshot_import(path))
    assert c.stats()["rounds"] == 150
    c.run()
    assert_same_run(o, c, n, trace=False)
    c.close()


# ---- 7. refusals: each before anything changes ----
def _standard(ctxf, exported, rounds=150):  # noqa: F811
    c = make_ctx(ctxf, exported["args"])
    assert c.run(rounds) == rounds
    return c, state(c, exported["n"])


def _variant_file(ctxf, args, path):  # noqa: F811
    """A file of another simulation (saved right after sgn_sim_init: the header is what counts)."""
    c = make_ctx(ctxf, args)
    c.snapshot_export(c.snapshot_save(), path)
    c.close()
    return path


def test_refuses_another_simulation(ctxf, oracle, exported, tmp_path):  # noqa: F811
    args, n = exported["args"], exported["n"]
    g, used, hosts, cfg, tr = args
    o = ref_run(oracle, "periodic", args, trace=True)
    c, at = _standard(ctxf, exported)
    # one host seed
    seed = hosts.seed.copy()
    seed[n // 2] ^= 1
    h2 = sgn.HostArrays(hosts.ip, hosts.node_id, hosts.bw_up, hosts.bw_down, seed)
    refused(EINVAL, "identity", lambda: c.snapshot_import(_variant_file(ctxf, (g, used, h2, cfg, tr), tmp_path / "seed.snap")))
    assert_state(state(c, n), at, "seed")
    # the stop time
    cfg2 = type(cfg).from_buffer_copy(cfg)
    cfg2.stop_time_ns += 1
    refused(EINVAL, "identity", lambda: c.snapshot_import(_variant_file(ctxf, (g, used, hosts, cfg2, tr), tmp_path / "stop.snap")))
    assert_state(state(c, n), at, "stop_time")
    # the same simulation, another process-local identity? no: the same calls give the same identity
    same = sgn.snapshot_file_info(_variant_file(ctxf, args, tmp_path / "same.snap"))["identity"]
    assert same == sgn.snapshot_file_info(exported["path"])["identity"]
    # a second sgn_sim_init with the same arguments: identity decides, not the generation
    c.sim_init(cfg, tr)
    snap = c.snapshot_import(exported["path"])
    c.snapshot_restore(snap)
    assert_state(state(c, n), exported["at"], "after a second sim_init")
    c.run()
    assert_same_run(o, c, n, trace=False)
    c.close()


def test_refuses_damaged_files(ctxf, oracle, exported, tmp_path):  # noqa: F811
    args, n = exported["args"], exported["n"]
    o = ref_run(oracle, "periodic", args, trace=True)
    raw = exported["path"].read_bytes()
    secs = sgn.snapshot_file_sections(exported["path"])
    by = {s["name"]: s for s in secs}
    nsec = len(secs)
    c, at = _standard(ctxf, exported, rounds=170)  # (another round edge than the file's)

    def damaged(name, data):
        p = tmp_path / name
        p.write_bytes(bytes(data))
        return p

    # one flipped payload byte: the device digest after the upload names the section
    for sec in ("hrec", "calendar", "ctrl"):
        bad = bytearray(raw)
        bad[by[sec]["offset"] + by[sec]["bytes"] // 2] ^= 0x10
        refused(EFILE, "section " + sec, lambda: c.snapshot_import(damaged("flip-" + sec, bad)))
        assert_state(state(c, n), at, "flip " + sec)
    # a flipped byte in the table: the trailer
    bad = bytearray(raw)
    bad[HDR + 24 * 3 + 17] ^= 1
    refused(EFILE, "digest", lambda: c.snapshot_import(damaged("flip-table", bad)))
    # truncated in the table, in a payload, before the trailer
    refused(EFILE, "truncated in the section table", lambda: c.snapshot_import(damaged("cut-table", raw[:HDR + 24 * 3 + 5])))
    refused(EFILE, "truncated in section fifo", lambda: c.snapshot_import(damaged("cut-fifo", raw[:by["fifo"]["offset"] + 100])))
    refused(EFILE, "truncated", lambda: c.snapshot_import(damaged("cut-trailer", raw[:-8])))
    refused(EFILE, "truncated in the header", lambda: c.snapshot_import(damaged("cut-header", raw[:100])))
    assert_state(state(c, n), at, "truncations")
    # slab fills that disagree with the packed calendar, under a CORRECT digest and trailer: only the
    # scan over the imported fills can tell
    bad = bytearray(raw)
    s = by["slab_n"]
    fills = np.frombuffer(raw[s["offset"]:s["offset"] + s["bytes"]], dtype="<u4").copy()
    i = int(np.flatnonzero(fills)[0])
    fills[i] -= 1
    bad[s["offset"]:s["offset"] + s["bytes"]] = fills.tobytes()
    k = [x["name"] for x in secs].index("slab_n")
    bad[HDR + 24 * k + 16:HDR + 24 * k + 24] = sgn.digest_bytes(fills).to_bytes(8, "little")
    bad[-8:] = sgn.digest_bytes(bytes(bad[:HDR + 24 * nsec])).to_bytes(8, "little")
    refused(EFILE, "slab fills add up to", lambda: c.snapshot_import(damaged("fills", bad)))
    assert_state(state(c, n), at, "fills")
    # a header field that is not this library's
    bad = bytearray(raw)
    bad[8] ^= 2  # format
    refused(EINVAL, "header field format", lambda: c.snapshot_import(damaged("format", bad)))
    refused(EFILE, "magic", lambda: c.snapshot_import(damaged("magic", b"SGNSNAP2" + raw[8:])))
    assert_state(state(c, n), at, "header")
    # the context still runs to the oracle's end, and the undamaged file still imports
    snap = c.snapshot_import(exported["path"])
    c.run()
    assert_same_run(o, c, n, trace=False)
    c.snapshot_restore(snap)
    assert_state(state(c, n), exported["at"], "restore after the run")
    c.close()


def test_refuses_traced_file_into_untraced_context(ctxf, exported, tmp_path):  # noqa: F811
    args, n = exported["args"], exported["n"]
    t = make_ctx(ctxf, args, trace=True)
    t.run(20)
    path = tmp_path / "traced.snap"
    t.snapshot_export(t.snapshot_save(), path)
    assert sgn.snapshot_file_info(path)["trace_records"] > 0
    refused(ESTATE, "trace", lambda: t.snapshot_import(exported["path"]))  # and the reverse
    t.close()
    c, at = _standard(ctxf, exported, rounds=20)
    refused(ESTATE, "trace", lambda: c.snapshot_import(path))
    assert_state(state(c, n), at, "traced file")
    # before sgn_sim_init there is nothing to import into
    e = ctxf()
    refused(ESTATE, "no simulation", lambda: e.snapshot_import(exported["path"]))
    e.close()
    c.close()


def test_write_callback_failure_and_no_file_left(ctxf, exported, tmp_path):  # noqa: F811
    n = exported["n"]
    c, at = _standard(ctxf, exported, rounds=30)
    snap = c.snapshot_save()
    calls = []

    def write(b):
        calls.append(len(b))
        if len(calls) == 3:
            raise OSError("disk full")

    refused(EFILE, "write callback", lambda: c.snapshot_export_stream(snap, write))
    assert len(calls) == 3 and calls[0] == HDR
    # the stream form writes what the file form writes
    chunks = []
    total = c.snapshot_export_stream(snap, chunks.append)
    good = tmp_path / "good.snap"
    assert c.snapshot_export(snap, good) == total == sum(map(len, chunks))
    assert b"".join(chunks) == good.read_bytes()
    # a file export that cannot finish leaves nothing
    gone = tmp_path / "no-such-dir" / "x.snap"
    refused(EFILE, "cannot create", lambda: c.snapshot_export(snap, gone))
    isdir = tmp_path / "is-a-dir"
    isdir.mkdir()
    refused(EFILE, "rename", lambda: c.snapshot_export(snap, isdir))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["good.snap", "is-a-dir"] and not list(isdir.iterdir())
    # a read callback that runs short, and the stream import of the good bytes
    data = good.read_bytes()
    pos = [0]

    def read(k, limit=len(data)):
        b = data[pos[0]:min(pos[0] + k, limit)]
        pos[0] += len(b)
        return b

    refused(EFILE, "truncated", lambda: c.snapshot_import_stream(lambda k: read(k, len(data) // 2)))
    pos[0] = 0
    snap2 = c.snapshot_import_stream(read)
    assert pos[0] == len(data)
    assert_state(state(c, n), at, "exports and imports change nothing")
    c.run(10)
    c.snapshot_restore(snap2)
    assert_state(state(c, n), at, "the stream's snapshot")
    c.close()


def test_imported_snapshot_restores_twice_and_is_freed(ctxf, oracle, exported):  # noqa: F811
    args, n = exported["args"], exported["n"]
    o = ref_run(oracle, "periodic", args, trace=True)
    c = make_ctx(ctxf, args)
    snap = c.snapshot_import(exported["path"])
    other = c.snapshot_import(exported["path"])  # (left for sgn_destroy)
    assert other.value != snap.value
    for _ in range(2):
        c.snapshot_restore(snap)
        assert_state(state(c, n), exported["at"], "restore")
        c.run()
        assert_same_run(o, c, n, trace=False)
    # an imported snapshot exports again, byte for byte
    again = exported["path"].with_name("again.snap")
    assert c.snapshot_export(snap, again) == exported["bytes"]
    assert again.read_bytes() == exported["path"].read_bytes()
    c.snapshot_free(snap)
    refused(EINVAL, "not a snapshot of this context", lambda: c.snapshot_restore(snap))
    c.close()
