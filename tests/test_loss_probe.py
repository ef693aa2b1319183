"""The loss-boundary probes (loss_probe.py) on the CPU: the numpy generator against the
oracle's, the probe search, and the oracle's own traced runs of the scenarios that
test_gpu_loss_boundary.py runs on the GPU — every probe reached, decided as the numpy stream
predicts, on a threshold recomputed from the oracle's route table."""
import numpy as np
import pytest

import loss_probe as lp
import sgn


def test_numpy_stream_is_the_oracles(oracle):
    L = oracle.load()
    seeds = np.array([0, 1, 2, 0xDEADBEEF, 2 ** 63, 2 ** 64 - 1, 892350, 108819870], dtype=np.uint64)
    n = 300
    x, carry = lp.draws(seeds, 0, n)
    for k, seed in enumerate(seeds):
        st = np.zeros(4, dtype=np.uint64)
        L.ora_xoshiro_seed_from_u64(int(seed), sgn.ptr(st, sgn.C.c_uint64))
        assert np.array_equal(st, lp.seed_state(seeds)[:, k])
        for i in range(n):
            a = (int(st[0]) + int(st[3])) & (2 ** 64 - 1)
            r = ((a << 23) | (a >> 41)) & (2 ** 64 - 1)
            nc = ((r >> 32) + (int(st[0]) >> 32)) & 0xFFFFFFFF
            got = int(L.ora_xoshiro_next_u64(sgn.ptr(st, sgn.C.c_uint64)))
            assert got == int(x[k, i]), (seed, i)
            assert (got >> 32) - nc in (0, 1, 1 - 2 ** 32) and bool(carry[k, i]) == ((got >> 32) != nc)
            if i in (0, 7, 299):
                assert np.array_equal(lp.state_after(seeds[k:k + 1], [i + 1])[0], st)
    assert np.array_equal(lp.state_after(seeds[:2], [0, 0]), lp.seed_state(seeds[:2]).T)
    assert 0.3 < carry.mean() < 0.7  # both kinds of draw are common


def test_thresholds_and_losses():
    for Th in (256, 1 << 31, lp.SCREEN_TH - 256, lp.SCREEN_TH, 0xFFFFFF00):
        loss = lp.loss_of(Th)
        assert loss.dtype == np.float32 and lp.th_of(loss) == Th
    assert lp.th_of(np.float32(1 / 32)) == lp.SCREEN_TH and lp.loss_of(lp.SCREEN_TH) == np.float32(1 / 32)
    assert lp.th_of(np.float32(1.0)) == 0 and lp.th_of(np.float32(0.0)) == 1 << 32
    assert [lp.th_of(v) for v in lp.END_LOSSES] == [1 << 32, 0xFFFFFF00, lp.SCREEN_TH, lp.SCREEN_TH,
                                                    1 << 31, 256, 0]


def test_probe_search():
    probes = lp.probe_set()
    lo, hi = lp.WINDOW
    by = {c: [p for p in probes if p.cls == c] for c in lp.CLASSES}
    for c, ps in by.items():
        assert len(ps) >= 8, c
        assert {p.index % 8 for p in ps} == set(range(8)), c
        assert min(p.index for p in ps) < lo + (hi - lo) // 4 and max(p.index for p in ps) >= hi - (hi - lo) // 4
        for p in ps:
            assert lo <= p.index < hi and p.Th % 256 == 0 and lp.th_of(p.loss) == p.Th
            h = p.x >> 32
            assert h == (p.Th if c in "ABE" else p.Th - 1) and p.drop == (c in "ABE")
            assert (p.Th >= lp.SCREEN_TH) == (c in "ABCD")
            if c in "AD":
                assert p.carry
            if c in "BC":
                assert not p.carry
    for c in "EF":
        assert sum(p.loss >= 0.5 for p in by[c]) * 2 >= len(by[c]), c
    # the draws that equal their threshold beyond the high word: all of x, or x >> 11 alone
    exact = [p for p in probes if p.cls in "GH"]
    assert len(exact) + sum(len(ps) for ps in by.values()) == len(probes)
    for p in exact:
        assert p.drop and p.x >> 32 == p.Th and p.x >> 11 == (p.Th << 32) >> 11
        assert (p.x == p.Th << 32) == (p.cls == "G") and lo <= p.index < hi
    for c in "GH":
        assert any(p.cls == c and p.Th < lp.SCREEN_TH for p in exact), c
    assert any(p.cls == "H" and p.Th >= lp.SCREEN_TH for p in exact)
    assert {p.cls for p in probes if p.Th == lp.SCREEN_TH} == set("ABCD")
    assert {p.cls for p in probes if p.Th == lp.SCREEN_TH - 256} == set("EF")
    assert len({p.seed for p in probes}) == len(probes)
    assert lp.probe_set() == probes  # deterministic


def test_addresses_are_the_automatic_ones(oracle):
    rc, ips = oracle.assign_ips(600)
    assert rc == 0 and np.array_equal(ips, lp.auto_ips(600))


@pytest.fixture(scope="module", params=["tgen", "periodic"])
def oracle_probe_run(request, oracle):
    probes = lp.probe_set()
    args = (lp.tgen_scenario if request.param == "tgen" else lp.periodic_scenario)(probes)
    g, used, hosts, cfg, tr = args
    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=True)
    o.run()
    return request.param, probes, hosts, lat, loss, o, o.trace()


def test_oracle_routes_hold_the_thresholds(oracle_probe_run):
    _, probes, _, lat, loss, _, _ = oracle_probe_run
    V = len(probes)
    assert lat.shape == (V, V) and (lat[~np.eye(V, dtype=bool)] == 5_000_000).all()
    for v, p in enumerate(probes):
        for b in range(V):
            assert lp.th_of(loss[v, b]) == p.Th, (v, b)
            assert (int(np.float64(np.float32(1.0) - loss[v, b]) * 2.0 ** 53) << 11) >> 32 == p.Th


def test_oracle_reaches_and_decides_every_probe(oracle_probe_run):
    kind, probes, hosts, _, _, o, trace = oracle_probe_run
    assert len(trace) < 1 << 22  # the GPU tests' trace capacity
    assert (hosts.bw_up != hosts.bw_down).all()
    lp.check_probe_sends(trace, probes, "oracle")
    s = trace[(trace["kind"] == sgn.TRACE_SEND) & (trace["host"] < len(probes))]
    # the window lies well inside what the slowest probe host sends
    assert np.bincount(s["host"], minlength=len(probes)).min() >= 1.5 * lp.WINDOW[1]
    st = o.stats()
    assert st["packets_loss_dropped"] > 0 and st["packets_unknown_dst"] == 0
    if kind == "tgen":
        # a 1 Gbit/s server's refill admits ~83 packets, so a train's send is ten eight-draw
        # batches and a tail of three or four: most probes of every class sit in the batches
        pos = lp.probe_batch_positions(trace, probes)
        for c in lp.CLASSES:
            inb = [j < 8 * (n // 8) for p, (j, n) in zip(probes, pos) if p.cls == c]
            assert sum(inb) >= 6, (c, [q for p, q in zip(probes, pos) if p.cls == c])
        # the draws equal to all of Tx (class G) are few: each sits in an eight-draw batch,
        # on a screened path (the redo's comparison) and on exact ones
        g = [(p.Th >= lp.SCREEN_TH, j < 8 * (n // 8)) for p, (j, n) in zip(probes, pos) if p.cls == "G"]
        assert (True, True) in g and (False, True) in g, g
        print("probe (class, position in its send, packets in the send):",
              [(p.cls, j, n) for p, (j, n) in zip(probes, pos)])


@pytest.mark.parametrize("case", list(lp.END_CASES))
def test_oracle_range_ends(oracle, case):
    g, used, hosts, cfg, tr = lp.ends_scenario(case)
    lat, loss = oracle.routes(g, used, shortest=False)
    assert np.array_equal(loss.view(np.uint32), np.repeat(lp.END_LOSSES, len(used)).reshape(loss.shape).view(np.uint32))
    for trace in (False, True):
        o = oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=trace)
        o.run()
        lp.check_ends(case, o, hosts, o.trace() if trace else None)
