"""bench.py --dump-outputs and the plain / --full split.

* CPU: dump_outputs over the oracle's Sim (it has the context's stats / window / digests
  calls): every file is float64, the 64-bit hashes come back bit for bit from their halves,
  and a shard past the size limit is written as the same seeded sample every time.
* GPU: a plain `bench.py --gpus 1 --steps N --warmup W --dump-outputs DIR` on a small workload,
  twice: N timed steps, `ms_per_step` in the line, nothing of the --full legs, and the two
  runs' files identical.
"""
import json
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import sgn

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
bench = pytest.importorskip("bench")


def _u64(halves):
    h = halves.astype(np.uint64)
    return (h[..., 0] << np.uint64(32)) | h[..., 1]


@pytest.fixture(scope="module")
def small_sim(oracle):
    n, V = 256, 32
    g = sgn.random_graph(V, seed=3)
    used = np.arange(V)
    seeds = sgn.derive_seeds(1, sgn.host_names(n))
    hosts = sgn.HostArrays(sgn.assign_ips(n), np.arange(n) % V, np.full(n, 10_000_000),
                           np.full(n, 10_000_000), seeds)
    cfg = sgn.make_config(200_000_000, codel_cap=1024, event_capacity=1 << 18)
    tr = sgn.make_traffic(period_ns=2_000_000, start_jitter_ns=2_000_000, unknown_dst_permille=5)
    lat, loss = oracle.routes(g, used)
    sim = oracle.Sim(used, lat, loss, hosts, cfg, tr)
    assert sim.run(50) == 50
    return sim, n


def test_f64_halves_are_exact():
    a = np.array([0, 1, (1 << 53) + 1, 0xFFFFFFFFFFFFFFFF, 0x0123456789ABCDEF], dtype=np.uint64)
    h = bench._f64(a, True)
    assert h.dtype == np.float64 and h.shape == (5, 2)
    assert np.array_equal(_u64(h), a)
    assert np.array_equal(bench._f64(a[:2], False), np.array([0.0, 1.0]))
    with pytest.raises(AssertionError):
        bench._f64(a, False)  # a value no float64 holds is never written as one


def test_dump_outputs_round_trips_the_state(small_sim, tmp_path):
    sim, n = small_sim
    bench.dump_outputs(tmp_path / "a", sim, n, 0, 1)
    got = {p.stem: np.load(p) for p in (tmp_path / "a").glob("*.npy")}
    assert set(got) == {"stats", "window", "host_ids"} | {f"digest_{f}" for f in bench.DIGEST_KEYS}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    st, dg = sim.stats(), sim.digests(0, n)
    assert st["packets_sent"] > 0
    assert _u64(got["stats"]).tolist() == [st[k] for k in bench.STAT_KEYS]
    ws, we, act = sim.window()
    assert _u64(got["window"]).tolist() == [ws, we, int(act)]
    assert np.array_equal(got["host_ids"], np.arange(n))
    for f in bench.DIGEST_KEYS:
        a = got[f"digest_{f}"]
        back = _u64(a) if f in bench.HASH_FIELDS else a.astype(np.uint64)
        assert np.array_equal(back, dg[f]), f


def test_dump_outputs_samples_a_large_shard_the_same_way(small_sim, tmp_path, monkeypatch):
    sim, n = small_sim
    per_host = 2 * sgn.DIGEST_DTYPE.itemsize + 8
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100 * per_host)
    bench.dump_outputs(tmp_path / "a", sim, n, 0, 1)
    bench.dump_outputs(tmp_path / "b", sim, n, 0, 1)
    ids = np.load(tmp_path / "a" / "host_ids.npy").astype(np.int64)
    assert len(ids) == 100 and len(set(ids.tolist())) == 100 and np.all(np.diff(ids) > 0)
    assert ids.min() >= 0 and ids.max() < n
    dg = sim.digests(0, n)
    assert np.array_equal(_u64(np.load(tmp_path / "a" / "digest_tx.npy")), dg["tx"][ids])
    for p in (tmp_path / "a").glob("*.npy"):
        assert np.array_equal(np.load(p), np.load(tmp_path / "b" / p.name)), p.name


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_dump_repeats(tmp_path):
    lines = []
    for d in ("a", "b"):
        cmd = [sys.executable, "-u", str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
               "--hosts", "3000", "--nodes", "60", "--rounds-per-step", "50", "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-4000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == 3 and line["rounds_timed"] == 150
        assert line["ms_per_step"] > 0 and line["value"] > 0 and line["packet_events_timed"] > 0
        assert line["unit"] == "packet events/s" and line["higher_is_better"] is True and line["dtype"] == "u64"
        assert line["cpu_baseline"] is None and line["parity"] is None and "parity_detail" not in line
    assert lines[0]["packet_events_timed"] == lines[1]["packet_events_timed"]
    names = sorted(p.name for p in (tmp_path / "a").glob("*.npy"))
    assert "stats.npy" in names and "digest_tx.npy" in names
    assert names == sorted(p.name for p in (tmp_path / "b").glob("*.npy"))
    total = 0
    for nme in names:
        a, b = np.load(tmp_path / "a" / nme), np.load(tmp_path / "b" / nme)
        assert a.dtype == np.float64 and np.array_equal(a, b), nme
        total += a.nbytes
    assert total <= 64 << 20
    st = dict(zip(bench.STAT_KEYS, _u64(np.load(tmp_path / "a" / "stats.npy")).tolist()))
    assert st["rounds"] == 250 and st["packets_sent"] > 0
