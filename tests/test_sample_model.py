"""sgn.Samples on hand-made rows (CPU only): dense() and cumulative() put every row where its
sample and host say, an empty sample is a row of zeros, a host that never appears a column of
zeros, and the pieces of successive takes join into one set."""
import numpy as np
import pytest

import sgn

N = 6  # hosts 0..5; host 4 never appears


def rows_of(items):
    r = np.zeros(len(items), sgn.SAMPLE_ROW_DTYPE)
    for k, (host, sample, vals) in enumerate(items):
        r[k]["host"], r[k]["sample"] = host, sample
        for f, v in zip(sgn.SAMPLE_FIELDS, vals):
            r[k][f] = v
    return r


def infos_of(counts, first_index=0):
    i = np.zeros(len(counts), sgn.SAMPLE_INFO_DTYPE)
    i["sample"] = first_index + np.arange(len(counts))
    i["rounds"] = 10 * (1 + np.arange(len(counts)))
    i["rows"] = counts
    i["first_row"] = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return i


def vals(base):
    return [base + k for k in range(7)]


ITEMS = [(0, 3, vals(10)), (2, 3, vals(20)), (5, 3, vals(30)),   # sample 3: three hosts
         # sample 4: empty
         (1, 5, vals(40)), (2, 5, vals(50)),                     # sample 5
         (5, 6, [0, 0, 0, 0, 0, 0, 2 ** 40])]                    # sample 6: one counter only, beyond 32 bits
COUNTS = [3, 0, 2, 1]


def expected(field):
    f = sgn.SAMPLE_FIELDS.index(field)
    d = np.zeros((4, N), np.uint64)
    for host, sample, v in ITEMS:
        d[sample - 3, host] = v[f]
    return d


@pytest.mark.parametrize("field", sgn.SAMPLE_FIELDS)
def test_dense_and_cumulative_round_trip(field):
    s = sgn.Samples(rows_of(ITEMS), infos_of(COUNTS, first_index=3))
    assert len(s) == 4
    d = s.dense(field, N)
    assert d.dtype == np.uint64 and d.shape == (4, N)
    assert np.array_equal(d, expected(field))
    assert not d[1].any()      # the empty sample
    assert not d[:, 4].any()   # the host that never appears
    c = s.cumulative(field, N)
    assert c.dtype == np.uint64 and np.array_equal(c, np.cumsum(expected(field), axis=0, dtype=np.uint64))
    # the rows come back from the dense form: every non-zero cell is a row's field
    k, h = np.nonzero(d)
    got = {(int(a) + 3, int(b)): int(d[a, b]) for a, b in zip(k, h)}
    f = sgn.SAMPLE_FIELDS.index(field)
    assert got == {(sample, host): v[f] for host, sample, v in ITEMS if v[f]}


def test_takes_join_into_one_set():
    r = rows_of(ITEMS)
    i = infos_of(COUNTS, first_index=3)
    a = (r[:3], infos_of(COUNTS[:2], first_index=3))                      # samples 3, 4
    b = (np.zeros(0, sgn.SAMPLE_ROW_DTYPE), np.zeros(0, sgn.SAMPLE_INFO_DTYPE))  # a take with nothing pending
    c = (r[3:], infos_of(COUNTS[2:], first_index=5))                      # samples 5, 6: first_row from 0 again
    s = sgn.Samples.from_takes([a, b, c])
    assert np.array_equal(s.rows, r)
    assert np.array_equal(s.infos["first_row"], i["first_row"]) and np.array_equal(s.infos["sample"], i["sample"])
    assert np.array_equal(s.dense("sent", N), expected("sent"))
    assert c[1]["first_row"][0] == 0  # (the pieces themselves are not modified)


def test_no_samples_and_mismatched_infos():
    s = sgn.Samples()
    assert len(s) == 0 and s.dense("sent", N).shape == (0, N) and s.cumulative("blocked", N).shape == (0, N)
    with pytest.raises(ValueError):
        sgn.Samples(rows_of(ITEMS), infos_of([3, 0, 2]))
