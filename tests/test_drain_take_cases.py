"""The ordered drain's scenarios on the oracle alone (CPU): what tests/test_gpu_drain_take.py claims
of its simulations — exact segment sizes, a span that mixes DELIVERED and CODEL records — holds for
the oracle's records, which the GPU tests then compare libsgn's takes with. TILE is the class limit
libsgn reports today (sgn_drain_take_timing::tile); the GPU tests build the cases from the value
they read."""
import numpy as np

import sgn
from drain_take_cases import fan_in_case, segments_case, spans_of
from external_common import calendar_shape

TILE = 1024


def run_oracle(oracle, world, dg):
    g, used, hosts, cfg, tr = world
    lat, loss = oracle.routes(g, used)
    o = oracle.Sim(used, lat, loss, hosts, cfg, tr)
    nb, bw = calendar_shape(lat, cfg)
    assert int(dg[3][-1]) < sgn.SIMULATION_START + (nb - 2) * bw  # everything can be submitted at once
    o.submit(dg[0], dg[1], dg[2], dg[3], dg[4], wire_len=dg[5])
    o.run()
    return o.drain()


def test_segments_case_yields_the_exact_segments(oracle):
    world, dg, counts = segments_case(TILE)
    d = run_oracle(oracle, world, dg)
    assert len(d) == len(dg[3]) and np.all(d["status"] == sgn.DRAIN_UNKNOWN)
    host, first, count = spans_of(d)
    assert dict(zip(host.tolist(), count.tolist())) == counts
    assert np.array_equal(d["host"], d["src_host"]) and len(np.unique(d["handle"])) == len(d)


def test_fan_in_case_mixes_delivered_and_codel(oracle):
    world, dg, dst = fan_in_case(TILE)
    d = run_oracle(oracle, world, dg)
    assert len(d) == len(dg[3])  # every datagram was decided before the stop time
    at = d[d["host"] == dst]
    st = np.bincount(at["status"], minlength=6)
    assert len(at) >= TILE + 100, len(at)
    assert st[sgn.DRAIN_DELIVERED] >= 10 and st[sgn.DRAIN_CODEL] >= 10, st
    assert st[sgn.DRAIN_DELIVERED] + st[sgn.DRAIN_CODEL] == len(at)
