"""The router delay report's entry points of the C ABI (CPU only: no GPU calls): the six calls are
exported, refuse a null context without touching a device, leave the ABI version alone (they are
additive), and the three structs they move have the layout of include/sgn.h."""
import ctypes as C
import pathlib
import re
import subprocess

import sgn

EINVAL = -22
NAMES = ("sgn_delay_enable", "sgn_delay_fold", "sgn_delay_get", "sgn_delay_clear", "sgn_delay_timing_get",
         "sgn_selftest_delay_fold")


def test_library_exports_delay_calls(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(sgn.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (sgn_[a-z0-9_]+)", out))
    for n in NAMES:
        assert n in exported, n
        assert hasattr(lib, n)
    assert lib.sgn_abi_version() == 10


def test_null_context_is_refused(lib):
    info = sgn.DelayInfo()
    rows = (sgn.DelayRow * 2)()
    n = C.c_uint64(7)
    timing = sgn.DelayTiming()
    assert lib.sgn_delay_enable(None) == EINVAL
    assert lib.sgn_delay_fold(None, C.byref(info)) == EINVAL
    assert lib.sgn_delay_fold(None, None) == EINVAL
    assert lib.sgn_delay_get(None, rows, 2, C.byref(n), C.byref(info)) == EINVAL and n.value == 0
    assert lib.sgn_delay_get(None, None, 0, None, None) == EINVAL
    assert lib.sgn_delay_clear(None) == EINVAL
    assert lib.sgn_delay_timing_get(None, C.byref(timing)) == EINVAL
    assert lib.sgn_delay_timing_get(None, None) == EINVAL
    n.value = 7
    ends = (C.c_uint64 * 1)(0)
    assert lib.sgn_selftest_delay_fold(None, None, ends, 1, 0, 4, None, rows, 2, C.byref(n), C.byref(info)) == EINVAL
    assert n.value == 0


ROW_FIELDS = ("host", "reserved", "standing", "unmatched", "delivered", "dropped", "delay_sum_delivered",
              "delay_sum_dropped", "delay_max", "standing_oldest")
INFO_FIELDS = ("rounds", "window_start", "window_end", "folds", "records", "hosts", "rows", "total", "delay_max",
               "delay_max_host", "pad0", "hist_delivered", "hist_dropped")
TIMING_FIELDS = ("total_ms", "order_ms", "kernel_ms", "records", "hosts", "largest_span", "carry_entries",
                 "spans_by_class", "wave_max", "tile")


def test_delay_structs_match_header(tmp_path):
    root = pathlib.Path(__file__).resolve().parent.parent
    lines = ['printf("%zu %zu %zu\\n", sizeof(sgn_delay_row), sizeof(sgn_delay_info), sizeof(sgn_delay_timing));',
             'printf("%d\\n", SGN_DELAY_BINS);']
    for st, fields in (("sgn_delay_row", ROW_FIELDS), ("sgn_delay_info", INFO_FIELDS), ("sgn_delay_timing", TIMING_FIELDS)):
        for f in fields:
            lines.append('printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (st, f, st, f))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgn.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    out = [tuple(map(int, ln.split())) for ln in
           subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert out[0] == (64, C.sizeof(sgn.DelayInfo), C.sizeof(sgn.DelayTiming))
    assert C.sizeof(sgn.DelayRow) == 64 == sgn.DELAY_ROW_DTYPE.itemsize
    assert out[1] == (sgn.DELAY_BINS,) == (48,)
    k = 2
    for struct, dtype, fields in ((sgn.DelayRow, sgn.DELAY_ROW_DTYPE, ROW_FIELDS), (sgn.DelayInfo, None, INFO_FIELDS),
                                  (sgn.DelayTiming, None, TIMING_FIELDS)):
        for f in fields:
            d = getattr(struct, f)
            assert out[k] == (d.offset, d.size), (struct.__name__, f, out[k])
            if dtype is not None:
                assert dtype.fields[f][1] == d.offset and dtype.fields[f][0].itemsize == d.size, (struct.__name__, f)
            k += 1
    assert [n for n, _ in sgn.DelayRow._fields_] == list(ROW_FIELDS)
    assert len(sgn.DELAY_TOTALS) == 6 == len(sgn.DelayInfo().total)
    assert len(sgn.delay_bin_edges()) == sgn.DELAY_BINS == len(sgn.DelayInfo().hist_delivered) == len(sgn.DelayInfo().hist_dropped)


def test_quantile_reads_the_histogram():
    """Delay.quantile: the upper edge of the bin that holds the q-th matched packet."""
    info = sgn.DelayInfo()
    info.hist_delivered[0] = 5    # delay 0
    info.hist_delivered[3] = 4    # [4, 8)
    info.hist_delivered[47] = 1   # from 2^46 up
    info.hist_dropped[21] = 2     # [2^20, 2^21)
    d = sgn.Delay(info)
    assert d.quantile(0.5) == 0 and d.quantile(0.51) == 7 and d.quantile(0.9) == 7
    assert d.quantile(1.0) == sgn.EMUTIME_INVALID and d.quantile(1e-9) == 0
    assert d.quantile(0.5, dropped=True) == (1 << 21) - 1
    assert sgn.Delay(sgn.DelayInfo()).quantile(0.5) is None
