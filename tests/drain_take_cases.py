"""Scenarios of the ordered drain's tests, built from numpy alone so that the CPU tests can check on
the oracle what the GPU tests then claim of libsgn (tests/test_drain_take_cases.py runs every one of
them on the oracle; tests/test_gpu_drain_take.py runs libsgn beside it)."""
import numpy as np

import sgn
from external_common import external_world

S0 = sgn.SIMULATION_START
MS = 1_000_000
UNKNOWN_IP = 0x0AFF0001  # 10.255/16: not registered


def segments_case(tile):
    """Datagrams to an unregistered address: each is decided at its send and yields exactly one
    UNKNOWN record at its sender. Senders 1..6 of a 10-host world get 1, 2, 63, 64, 65 and tile + 1
    of them, all inside one window: segments on both sides of both class borders."""
    world = external_world(n=10, V=5, bw=1_000_000_000, fifo=64, slow_every=1000)
    counts = {1: 1, 2: 2, 3: 63, 4: 64, 5: 65, 6: tile + 1}
    src = np.concatenate([np.full(k, h, np.uint32) for h, k in counts.items()])
    src = src[np.random.default_rng(3).permutation(len(src))]
    k = len(src)
    t = S0 + 1000 + 700 * np.arange(k, dtype=np.uint64)  # (no two at one time, all below S0 + 1 ms)
    handle = (np.arange(k, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    dg = (src, np.full(k, UNKNOWN_IP, np.uint32), np.zeros(k, np.uint32), t, handle, np.zeros(k, np.uint32))
    return world, dg, counts


def fan_in_case(tile):
    """tile + 400 empty datagrams from the fast hosts to host 7, which sits behind a 200 kbit/s
    link, within 50 ms: more than a second of standing queue at its router, so its span holds
    DELIVERED and CODEL records, more than tile + 100 of them after the paths' loss."""
    world = external_world(fifo=64, stop_ns=5_000 * MS)
    hosts = world[2]
    rng = np.random.default_rng(23)
    k = tile + 400
    fast = np.array([h for h in range(hosts.n) if h % 7])
    src = rng.choice(fast, k).astype(np.uint32)
    t = S0 + np.sort(rng.choice(50 * MS, k, replace=False)).astype(np.uint64)
    handle = (np.arange(k, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    dg = (src, np.full(k, hosts.ip[7], np.uint32), np.zeros(k, np.uint32), t, handle, np.zeros(k, np.uint32))
    return world, dg, 7


def spans_of(recs):
    """(host, first, count) of every run of `host` in recs, as three arrays."""
    if len(recs) == 0:
        z = np.zeros(0, np.uint64)
        return z.astype(np.uint32), z, z
    h = recs["host"]
    first = np.concatenate([[0], np.nonzero(np.diff(h.astype(np.int64)) != 0)[0] + 1]).astype(np.uint64)
    count = np.diff(np.concatenate([first, [len(h)]]).astype(np.uint64))
    return h[first.astype(np.int64)], first, count
