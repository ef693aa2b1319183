"""The event path's arithmetic on the device, bit-exact against the oracle (-m gpu).

The round kernels divide nowhere by the general u64 routine (csrc/sgn_internal.h: umod64,
tb_refills, tb_quot, tb_conforming; tests/test_event_arith.py checks those on the CPU). Here
the places that use them run at their extremes:
  * token buckets from 8 bytes a refill (a removal waits dozens of refill intervals) up to a
    refill increment above 2^32 (a removal never fails), batched over trains (TGEN) and one
    datagram at a time (PERIODIC);
  * the CoDel free ring's counters pass several multiples of the pool size (the ring index is
    counter mod cq_pages by cq_pages' reciprocal) and the pool grows (the reciprocal changes);
  * the same with the diagnostic stamps on, and CPU-submitted datagrams (EXTERNAL) with them on.
"""
import numpy as np
import pytest

import sgn
from test_gpu_parity import assert_same_run, ctxf, run_both, scenario  # noqa: F401 (ctxf: fixture)

pytestmark = pytest.mark.gpu

N = 300


def _extreme_bw():
    cyc = np.array([64_000, 1_000_000, 10_000_000, 1 << 46], dtype=np.uint64)
    tenth = np.array([1 << 46, 100_000_000, 64_000], dtype=np.uint64)
    i = np.arange(N)
    return np.where(i % 10 == 0, tenth[(i // 10) % 3], cyc[i % 4]).astype(np.uint64)


def _tb_args(kind, stop_ns=1_000_000_000):
    return scenario(n=N, V=30, kind=kind, stop_ns=stop_ns, tor=True, tgen_think=100_000_000, bw=_extreme_bw())


@pytest.mark.parametrize("kind", [sgn.TRAFFIC_TGEN, sgn.TRAFFIC_PERIODIC])
def test_token_bucket_extremes(ctxf, oracle, kind):
    args = _tb_args(kind)
    o, c = run_both(ctxf, oracle, args, trace=False)
    st = c.stats()
    print(kind, st)
    assert st["packets_sent"] > 100_000, st
    if kind == sgn.TRAFFIC_TGEN:
        assert st["codel_dropped"] > 0, st
    else:
        assert st["app_blocked"] > 0, st
    assert c.engine_info()["persistent_grid"] > 0
    assert_same_run(o, c, N, trace=False)


@pytest.mark.parametrize("kind", [sgn.TRAFFIC_TGEN, sgn.TRAFFIC_PERIODIC])
def test_token_bucket_extremes_traced(ctxf, oracle, kind):
    args = _tb_args(kind, stop_ns=300_000_000)
    o, c = run_both(ctxf, oracle, args, trace=True)
    assert c.stats()["packets_sent"] > 10_000
    assert_same_run(o, c, N, trace=True)


@pytest.mark.parametrize("persistent", ["1", "0"])
def test_codel_ring_wraps_and_pool_grows(ctxf, oracle, monkeypatch, persistent):
    # slow down-links and short think times: CoDel queues stand, drain and stand again for 16 s.
    # 160 run slots a host = 3000 pages at first; the pool grows (once, to 6000 pages: the
    # reciprocal of cq_pages changes mid-run) and the allocation counter passes the pool size
    # about five times (pages come back through the free ring and leave again).
    monkeypatch.setenv("SGN_PERSISTENT", persistent)
    bw = np.where(np.arange(N) % 10 == 0, 100_000_000, 8_000_000).astype(np.uint64)
    args = scenario(n=N, V=30, kind=sgn.TRAFFIC_TGEN, stop_ns=16_000_000_000, bw=bw, tor=True,
                    tgen_think=20_000_000, codel=160)
    o, c = run_both(ctxf, oracle, args, trace=False)
    st, info = c.stats(), c.engine_info()
    print({k: info[k] for k in ("codel_pages", "codel_page_allocs", "codel_pool_grows")}, st["codel_dropped"])
    assert info["codel_page_allocs"] >= 4 * info["codel_pages"], info
    assert info["codel_pool_grows"] >= 1, info
    assert info["codel_pages_free"] + info["codel_pages_chained"] == info["codel_pages"], info
    assert (info["persistent_grid"] > 0) == (persistent == "1"), info
    assert_same_run(o, c, N, trace=False)


@pytest.mark.parametrize("kind", ["default", "tgen", "external"])
def test_stamps_on_is_bit_exact(ctxf, oracle, monkeypatch, kind):
    # the diagnostic stamps are read by the host only: a run with them on computes the same
    monkeypatch.setenv("SGN_STAMPS", "1")
    if kind == "external":
        # CPU-submitted datagrams, submitted ahead and run many rounds per call (k_rounds_diag<EXTERNAL>):
        # test_gpu_external's CoDel world, every drain record compared on the way
        from test_gpu_external import run_case
        o, c, _, _ = run_case(ctxf, oracle, "codel", flags=sgn.CREATE_TIME_KERNELS)
        assert c.stats()["packets_sent"] > 1000
        assert c.kernel_times()["k_rounds"][0] > 0, c.kernel_times()
        assert_same_run(o, c, 60, trace=False)
        return
    if kind == "default":
        args, n = scenario(), 200
    else:
        args, n = scenario(n=N, V=30, kind=sgn.TRAFFIC_TGEN, stop_ns=600_000_000, tor=True,
                           tgen_think=100_000_000), N
    # (kernel_times() samples launches only in a context created with the timing flag)
    o, c = run_both(lambda: ctxf(flags=sgn.CREATE_TIME_KERNELS), oracle, args, trace=False)
    assert c.stats()["packets_sent"] > 1000
    assert c.kernel_times()["k_rounds"][0] > 0, c.kernel_times()
    assert_same_run(o, c, n, trace=False)
