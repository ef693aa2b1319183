"""The router delay report's model on the oracle alone (CPU): what tests/test_gpu_delay.py relies
on. On the oracle's trace the rank match the kernels use (the k-th exit of a host with its k-th POP)
and the key match of the model (host, peer, c) give the same pairs; the fan-in scenario has CoDel
drops, delays above a second and nothing standing at its end; and the model's result does not depend
on where the record stream is cut into intervals. TILE is the class limit libsgn reports today
(sgn_drain_take_timing::tile), as in tests/test_drain_take_cases.py."""
import numpy as np
import pytest

import sgn
from delay_model import (CODEL_DROP, DELIVER, POP, DelayModel, delay_bin, ordered, pairs_by_key, pairs_by_rank,
                         run_model)
from drain_take_cases import fan_in_case
from external_common import datagrams, drive_ahead, external_world

TILE = 1024
SEC = 1_000_000_000


def traced(oracle, world):
    g, used, hosts, cfg, tr = world
    lat, loss = oracle.routes(g, used)
    return oracle.Sim(used, lat, loss, hosts, cfg, tr, trace=True)


@pytest.fixture(scope="module")
def fan_in(oracle):
    world, dg, dst = fan_in_case(TILE)
    o = traced(oracle, world)
    o.submit(dg[0], dg[1], dg[2], dg[3], dg[4], wire_len=dg[5])
    o.run()
    return ordered(o.trace()), dst


@pytest.fixture(scope="module")
def external(oracle):
    world = external_world()
    o = traced(oracle, world)
    drive_ahead([o], datagrams(world[2]), 20_000_000)
    return ordered(o.trace())


def test_bins():
    assert [delay_bin(d) for d in (0, 1, 2, 3, 4, 2 ** 20 - 1, 2 ** 20, 2 ** 46 - 1, 2 ** 46, 2 ** 47, 2 ** 63)] == \
        [0, 1, 2, 2, 3, 20, 21, 46, 47, 47, 47]


@pytest.mark.parametrize("which", ["fan_in", "external"])
def test_rank_match_is_the_key_match(which, request):
    t = request.getfixturevalue(which)
    t = t[0] if which == "fan_in" else t
    by_key, by_rank = pairs_by_key(t), pairs_by_rank(t)
    exits = int(((t["kind"] == DELIVER) | (t["kind"] == CODEL_DROP)).sum())
    assert len(by_key) == exits > 300  # every exit has its POP in the trace
    assert sorted(by_key) == sorted(by_rank)
    for p, x in by_rank:  # field by field
        assert t["host"][p] == t["host"][x] and t["peer"][p] == t["peer"][x] and t["c"][p] == t["c"][x]
        assert t["a"][x] >= t["a"][p] and t["seq"][x] > t["seq"][p]


def test_fan_in_has_drops_long_delays_and_nothing_left(fan_in):
    t, dst = fan_in
    rows, info = run_model(t)
    assert info["total"][1] >= 20, info["total"]                 # CODEL_DROP exits
    assert int((t["kind"] == CODEL_DROP).sum()) == info["total"][1]
    assert info["delay_max"] > SEC and info["delay_max_host"] == dst
    assert info["total"][4] == 0 and info["total"][5] == 0       # nothing standing, nothing unmatched
    assert np.all(rows["standing"] == 0) and np.all(rows["standing_oldest"] == sgn.EMUTIME_INVALID)
    at = rows[rows["host"] == dst][0]
    assert at["delivered"] + at["dropped"] == int(((t["host"] == dst) & (t["kind"] == POP)).sum()) > TILE // 2
    nz = [k for k in range(sgn.DELAY_BINS) if k and info["hist_delivered"][k] + info["hist_dropped"][k]]
    assert 20 <= min(nz) and max(nz) <= 31, nz
    assert sum(info["hist_delivered"]) == info["total"][0] and sum(info["hist_dropped"]) == info["total"][1]


@pytest.mark.parametrize("which", ["fan_in", "external"])
def test_cut_into_pieces_changes_nothing(which, request):
    t = request.getfixturevalue(which)
    t = t[0] if which == "fan_in" else t
    # an interval is a range of time: cut the stream where the records' times pass a threshold
    # (a (host, seq) order restricted to an interval stays a (host, seq) order)
    when = t["a"]  # (a host's records carry non-decreasing times)
    whole_rows, whole = run_model(t)
    rng = np.random.default_rng(4)
    for cuts in (1, 3, 25):  # at record positions of the (host, seq) order: every host's stream stays in order
        ends = np.sort(rng.choice(np.arange(1, len(t)), cuts, replace=False)).tolist() + [len(t)]
        rows, info = run_model(t, ends)
        assert info["folds"] == cuts + 1
        info["folds"] = 1
        assert info == whole and rows.tobytes() == whole_rows.tobytes()
    for cuts in (1, 2, 7, 40):
        edges = np.sort(rng.choice(np.unique(when), cuts, replace=False))
        m = DelayModel()
        lo = 0
        standing_seen = 0
        for e in list(edges) + [int(when.max()) + 1]:
            m.fold(t[(when >= lo) & (when < e)])
            standing_seen = max(standing_seen, m.result()[1]["total"][4])
            lo = e
        rows, info = m.result()
        assert info["folds"] == cuts + 1 and info["records"] == len(t)
        info["folds"] = 1
        assert info == whole and rows.tobytes() == whole_rows.tobytes()
        if cuts == 40:
            assert standing_seen > 0  # some cut crossed packets between their POP and their exit


def test_standing0_counts_as_unmatched(fan_in):
    """The records from a mid-way time on, with what stood at the routers then as unknown entries:
    their exits are unmatched, everything popped later is matched as in the whole run."""
    t, dst = fan_in
    edge = int(np.median(t["a"][t["kind"] == POP]))
    m = DelayModel()
    m.fold(t[t["a"] < edge])
    before_rows, before = m.result()
    assert before["total"][4] > 10  # packets stand at the edge
    standing0 = np.zeros(int(t["host"].max()) + 1, np.uint32)
    standing0[before_rows["host"]] = before_rows["standing"]
    rows, info = run_model(t[t["a"] >= edge], standing0=standing0)
    whole_rows, whole = run_model(t)
    assert info["total"][5] == before["total"][4] and info["total"][4] == 0
    assert info["total"][0] + info["total"][1] + info["total"][5] + before["total"][0] + before["total"][1] == \
        whole["total"][0] + whole["total"][1]
