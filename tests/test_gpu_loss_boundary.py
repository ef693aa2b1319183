"""The loss draw at its decision boundaries (engine.hip send_batch) against the oracle.

send_batch holds Worker::send_packet's rule `chance >= reliability` (core/worker.rs:363-371)
in three forms: per packet for traced hosts ((x >> 11) >= T), batched and exact for untraced
ones (x >= Tx, eight, four and one draw at a time) and, in the TGEN kernel on paths losing at
most 1/32, behind a screen on the eight draws' carry-less high words. Random losses and seeds
put a draw on a threshold once in 2^31, so here chosen draws of chosen hosts sit exactly on it
(loss_probe.py: classes A-F on the high word, G and H on the whole draw, and the ends of the
loss range); test_loss_probe.py shows on the CPU that the oracle reaches every probe and decides
it as the numpy stream predicts. What each class catches (single changes tried on the GPU):
`hm >= Th` for the screen's `hm >= Th - 1` fails class A; `x > Tx` in the exact eight-draw test
or in the screen's redo fails class G alone (hi32(x) == Th with a nonzero low word is still
above Tx); `(x >> 11) > T` in the per-packet form fails G and H in the traced variants.
"""
import numpy as np
import pytest

import loss_probe as lp
import sgn
from test_gpu_parity import assert_same_run, ctxf, run_both  # noqa: F401

pytestmark = pytest.mark.gpu


def assert_probe_hosts_agree(o, c, probes):
    """Names the probe classes whose hosts sent something else than the oracle's (a wrong
    decision changes the host's tx digest and its count of sent packets)."""
    V = len(probes)
    do, dg = o.digests(0, V), c.digests(0, V)
    bad = [(v, p.cls, p.index, hex(p.Th), int(do["n_sent"][v]), int(dg["n_sent"][v]))
           for v, p in enumerate(probes)
           if do["tx"][v] != dg["tx"][v] or do["n_sent"][v] != dg["n_sent"][v] or
           not np.array_equal(do["rng"][v], dg["rng"][v])]
    assert not bad, ("probe classes decided differently: " + "".join(sorted({b[1] for b in bad})), bad)


def check_probe_run(o, c, probes, hosts, trace):
    st = c.stats()
    assert st["packets_loss_dropped"] > 0 and st["packets_unknown_dst"] == 0, st
    assert_probe_hosts_agree(o, c, probes)  # first: it names the classes
    if trace:
        lp.check_probe_sends(o.trace(), probes, "oracle")
        lp.check_probe_sends(c.trace(), probes, "libsgn")
    assert_same_run(o, c, hosts.n, trace=trace)


@pytest.mark.parametrize("variant", ["persistent", "rounds", "traced"])
def test_tgen_probes(ctxf, oracle, monkeypatch, variant):
    """At least eight probes of every class on 1 Gbit/s servers whose trains go out ~83
    packets a refill: untraced in the persistent kernel and on per-round launches (the screen,
    its redo and the exact batches) and traced (the per-packet form, every probe's SEND record
    against the numpy prediction)."""
    probes = lp.probe_set()
    assert all(sum(p.cls == c for p in probes) >= 8 for c in lp.CLASSES)
    if variant == "rounds":
        monkeypatch.setenv("SGN_PERSISTENT", "0")
    args = lp.tgen_scenario(probes)
    o, c = run_both(ctxf, oracle, args, trace=variant == "traced")
    info = c.engine_info()
    assert (info["persistent_grid"] > 0) == (variant == "persistent"), info
    assert info["persistent_fallbacks"] == 0, info
    assert c.stats()["packets_sent"] > 300_000
    check_probe_run(o, c, probes, args[2], variant == "traced")


@pytest.mark.parametrize("trace", [False, True])
def test_periodic_probes(ctxf, oracle, trace):
    """The same probes, one host a node sending a datagram every millisecond: the PERIODIC
    kernel has no screen, every class takes the exact form (one draw per send)."""
    probes = lp.probe_set()
    args = lp.periodic_scenario(probes)
    o, c = run_both(ctxf, oracle, args, trace=trace)
    assert c.stats()["packets_sent"] > 20_000
    check_probe_run(o, c, probes, args[2], trace)


@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("case", list(lp.END_CASES))
def test_range_ends(ctxf, oracle, case, trace):
    """Paths losing 0, 2^-24, 1/32 and its f32 neighbour, 1/2, 1 - 2^-24 and everything
    (T == 0), direct (the table holds the arc's value), with full and with empty payloads: an
    empty payload cannot drop, yet its draw advances the stream."""
    g, used, hosts, cfg, tr = lp.ends_scenario(case)
    lat, loss = oracle.routes(g, used, shortest=False)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=trace)
    c = ctxf()
    c.routes_build(g, used, shortest=False)
    glat, gloss = c.routes_copy()
    assert np.array_equal(lat, glat) and np.array_equal(loss.view(np.uint32), gloss.view(np.uint32))
    assert [lp.th_of(v) for v in gloss[:, 0]] == [lp.th_of(v) for v in lp.END_LOSSES]
    c.hosts_set(hosts)
    if trace:
        c.trace_enable(1 << 20)
    c.sim_init(cfg, tr)
    o.run()
    c.run()
    lp.check_ends(case, c, hosts, c.trace() if trace else None)
    assert_same_run(o, c, hosts.n, trace=trace)
