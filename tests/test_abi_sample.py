"""The interval-statistics entry points of the C ABI (CPU only: no GPU calls): the six sgn_sample_*
calls are exported, refuse a null context without touching a device, leave the ABI version alone
(they are additive), and the two structs they move have the layout of include/sgn.h."""
import ctypes as C
import pathlib
import re
import subprocess

import sgn

EINVAL = -22
NAMES = ("sgn_sample_enable", "sgn_sample", "sgn_sample_rebase", "sgn_sample_pending", "sgn_sample_take",
         "sgn_sample_timing_get")


def test_library_exports_sample_calls(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(sgn.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (sgn_[a-z0-9_]+)", out))
    for n in NAMES:
        assert n in exported, n
        assert hasattr(lib, n)
    assert lib.sgn_abi_version() == 10


def test_null_context_is_refused(lib):
    info = sgn.SampleInfo()
    rows = (sgn.SampleRow * 2)()
    infos = (sgn.SampleInfo * 2)()
    n, ni = C.c_uint64(7), C.c_uint64(7)
    timing = sgn.SampleTiming()
    assert lib.sgn_sample_enable(None, 16) == EINVAL
    assert lib.sgn_sample_enable(None, 0) == EINVAL
    assert lib.sgn_sample(None, C.byref(info)) == EINVAL
    assert lib.sgn_sample(None, None) == EINVAL
    assert lib.sgn_sample_rebase(None) == EINVAL
    assert lib.sgn_sample_pending(None, C.byref(n), C.byref(ni)) == EINVAL and (n.value, ni.value) == (0, 0)
    n.value = ni.value = 7
    assert lib.sgn_sample_take(None, rows, 2, C.byref(n), infos, 2, C.byref(ni)) == EINVAL and (n.value, ni.value) == (0, 0)
    assert lib.sgn_sample_take(None, None, 0, None, None, 0, None) == EINVAL
    assert lib.sgn_sample_timing_get(None, C.byref(timing)) == EINVAL
    assert lib.sgn_sample_timing_get(None, None) == EINVAL


def test_sample_structs_match_header(tmp_path):
    root = pathlib.Path(__file__).resolve().parent.parent
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgn.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(sgn_sample_row), offsetof(sgn_sample_row, sent),\n'
                   '         offsetof(sgn_sample_row, blocked), sizeof(sgn_sample_info), offsetof(sgn_sample_info, first_row),\n'
                   '         offsetof(sgn_sample_info, total), sizeof(sgn_sample_timing), offsetof(sgn_sample_timing, hosts));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    row, off_sent, off_blocked, info, off_first, off_total, timing, off_hosts = map(
        int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert row == 64 == C.sizeof(sgn.SampleRow) == sgn.SAMPLE_ROW_DTYPE.itemsize
    assert off_sent == 8 == sgn.SampleRow.sent.offset == sgn.SAMPLE_ROW_DTYPE.fields["sent"][1]
    assert off_blocked == 56 == sgn.SampleRow.blocked.offset == sgn.SAMPLE_ROW_DTYPE.fields["blocked"][1]
    assert info == 104 == C.sizeof(sgn.SampleInfo) == sgn.SAMPLE_INFO_DTYPE.itemsize
    assert off_first == sgn.SampleInfo.first_row.offset == sgn.SAMPLE_INFO_DTYPE.fields["first_row"][1]
    assert off_total == sgn.SampleInfo.total.offset == sgn.SAMPLE_INFO_DTYPE.fields["total"][1]
    assert timing == C.sizeof(sgn.SampleTiming) and off_hosts == sgn.SampleTiming.hosts.offset
    # the rows' fields, in the order of sgn_sample_info::total
    assert [n for n, _ in sgn.SampleRow._fields_[2:]] == list(sgn.SAMPLE_FIELDS)
