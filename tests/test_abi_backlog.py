"""The backlog report's entry points of the C ABI (CPU only: no GPU calls): sgn_backlog and
sgn_backlog_timing_get are exported, refuse a null context without touching a device, leave the ABI
version alone (they are additive), and the three structs they move have the layout of include/sgn.h."""
import ctypes as C
import pathlib
import re
import subprocess

import sgn

EINVAL = -22
NAMES = ("sgn_backlog", "sgn_backlog_timing_get")


def test_library_exports_backlog_calls(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(sgn.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (sgn_[a-z0-9_]+)", out))
    for n in NAMES:
        assert n in exported, n
        assert hasattr(lib, n)
    assert lib.sgn_abi_version() == 10


def test_null_context_is_refused(lib):
    info = sgn.BacklogInfo()
    rows = (sgn.BacklogRow * 2)()
    n = C.c_uint64(7)
    timing = sgn.BacklogTiming()
    assert lib.sgn_backlog(None, rows, 2, C.byref(n), C.byref(info)) == EINVAL and n.value == 0
    assert lib.sgn_backlog(None, None, 0, C.byref(n), C.byref(info)) == EINVAL
    assert lib.sgn_backlog(None, None, 0, None, None) == EINVAL
    assert lib.sgn_backlog_timing_get(None, C.byref(timing)) == EINVAL
    assert lib.sgn_backlog_timing_get(None, None) == EINVAL


ROW_FIELDS = ("host", "flags", "router_packets", "send_packets", "router_bytes", "send_bytes", "router_oldest",
              "inflight_packets", "submit_pending", "inflight_earliest", "inflight_latest")
INFO_FIELDS = ("rounds", "window_start", "window_end", "hosts", "rows", "total", "max_router_packets", "max_router_host",
               "max_sojourn_ns", "max_sojourn_host", "inflight_earliest")
TIMING_FIELDS = ("total_ms", "kernel_ms", "copy_ms", "hosts", "rows", "calendar_runs")


def test_backlog_structs_match_header(tmp_path):
    root = pathlib.Path(__file__).resolve().parent.parent
    lines = ['printf("%zu %zu %zu\\n", sizeof(sgn_backlog_row), sizeof(sgn_backlog_info), sizeof(sgn_backlog_timing));',
             'printf("%u %u\\n", SGN_BACKLOG_ROUTER_HELD, SGN_BACKLOG_OUT_HELD);']
    for st, fields in (("sgn_backlog_row", ROW_FIELDS), ("sgn_backlog_info", INFO_FIELDS), ("sgn_backlog_timing", TIMING_FIELDS)):
        for f in fields:
            lines.append('printf("%%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (st, f, st, f))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgn.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    out = [tuple(map(int, ln.split())) for ln in
           subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert out[0] == (64, C.sizeof(sgn.BacklogInfo), C.sizeof(sgn.BacklogTiming))
    assert C.sizeof(sgn.BacklogRow) == 64 == sgn.BACKLOG_ROW_DTYPE.itemsize
    assert C.sizeof(sgn.BacklogInfo) == sgn.BACKLOG_INFO_DTYPE.itemsize
    assert out[1] == (sgn.BACKLOG_ROUTER_HELD, sgn.BACKLOG_OUT_HELD) == (1, 2)
    k = 2
    for struct, dtype, fields in ((sgn.BacklogRow, sgn.BACKLOG_ROW_DTYPE, ROW_FIELDS),
                                  (sgn.BacklogInfo, sgn.BACKLOG_INFO_DTYPE, INFO_FIELDS),
                                  (sgn.BacklogTiming, None, TIMING_FIELDS)):
        for f in fields:
            d = getattr(struct, f)
            assert out[k] == (d.offset, d.size), (struct.__name__, f, out[k])
            if dtype is not None:
                assert dtype.fields[f][1] == d.offset and dtype.fields[f][0].itemsize == d.size, (struct.__name__, f)
            k += 1
    # the rows' fields are all there is, and the totals name eight of them
    assert [n for n, _ in sgn.BacklogRow._fields_] == list(ROW_FIELDS)
    assert len(sgn.BACKLOG_TOTALS) == 8 == len(sgn.BacklogInfo().total)
