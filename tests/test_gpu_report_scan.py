"""The reports' scan (-m gpu): k_sample_scan, through sgn_selftest_report_scan, against numpy.

sgn_sample and sgn_backlog scan one count per wave of 64 hosts, in tiles of 1024 counts: their
simulations of a few thousand hosts never leave the first tile. Here the kernel runs on counts of
its own, so that the carry from tile to tile is under test: 1024 is one full tile, 1025 and 2049
carry into a last tile of one item, 4103 carries four times and ends ragged, 255 and 1023 leave the
last thread or threads of a tile partly empty. A wave's count is at most 64.
"""
import numpy as np
import pytest

import sgn
from test_gpu_parity import ctxf  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 4, 5, 255, 1023, 1024, 1025, 2048, 2049, 4103)


def scan(c, counts):
    n = len(counts)
    off = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    total = sgn.C.c_uint64(0xFFFFFFFFFFFFFFFF)
    c.check(c.L.sgn_selftest_report_scan(c.h, sgn.ptr(counts, sgn.C.c_uint32) if n else None, n,
                                         sgn.ptr(off, sgn.C.c_uint32) if n else None, sgn.C.byref(total)))
    return off, total.value


@pytest.mark.parametrize("n", SIZES)
def test_scan_matches_numpy(ctxf, n):
    c = ctxf()
    drawn = np.random.default_rng(1000 + n).integers(0, 65, size=n, dtype=np.uint32)
    for counts in (drawn, np.full(n, 64, dtype=np.uint32)):
        off, total = scan(c, counts)
        want = np.cumsum(counts, dtype=np.uint64) - counts  # the exclusive sum
        assert np.array_equal(off.astype(np.uint64), want)
        assert total == int(counts.sum(dtype=np.uint64))
