"""The ordered drain's entry points of the C ABI (CPU only: no GPU calls): sgn_drain_pending,
sgn_drain_take, sgn_drain_take_timing_get and sgn_selftest_drain_order are exported, refuse a null
context without touching a device, leave the ABI version alone (they are additive), and
sgn_drain_take_timing has the layout of include/sgn.h."""
import ctypes as C
import pathlib
import re
import subprocess

import sgn

EINVAL = -22
NAMES = ("sgn_drain_pending", "sgn_drain_take", "sgn_drain_take_timing_get", "sgn_selftest_drain_order")


def test_library_exports_drain_take_calls(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(sgn.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (sgn_[a-z0-9_]+)", out))
    for n in NAMES:
        assert n in exported, n
        assert hasattr(lib, n)
    assert lib.sgn_abi_version() == 10


def test_null_context_is_refused(lib):
    recs = (sgn.DrainRec * 2)()
    spans = (sgn.TraceSpan * 2)()
    n, ns = C.c_uint64(7), C.c_uint64(7)
    assert lib.sgn_drain_pending(None, C.byref(n)) == EINVAL and n.value == 0
    assert lib.sgn_drain_pending(None, None) == EINVAL
    n.value = 7
    assert lib.sgn_drain_take(None, recs, 2, C.byref(n), spans, 2, C.byref(ns)) == EINVAL
    assert n.value == 0 and ns.value == 0
    assert lib.sgn_drain_take(None, None, 0, C.byref(n), None, 0, None) == EINVAL
    assert lib.sgn_drain_take(None, None, 0, None, None, 0, None) == EINVAL
    timing = sgn.DrainTakeTiming()
    assert lib.sgn_drain_take_timing_get(None, C.byref(timing)) == EINVAL
    assert lib.sgn_drain_take_timing_get(None, None) == EINVAL
    ns.value = 7
    assert lib.sgn_selftest_drain_order(None, recs, 2, 0, 4, recs, spans, 2, C.byref(ns)) == EINVAL and ns.value == 0


TIMING_FIELDS = ("total_ms", "kernel_ms", "copy_ms", "records", "hosts", "largest_span", "spans_by_class", "wave_max", "tile")


def test_drain_take_timing_matches_header(tmp_path):
    root = pathlib.Path(__file__).resolve().parent.parent
    lines = ['printf("%zu %zu %zu\\n", sizeof(sgn_drain_take_timing), sizeof(sgn_drain_rec), sizeof(sgn_trace_span));']
    for f in TIMING_FIELDS:
        lines.append('printf("%%zu %%zu\\n", offsetof(sgn_drain_take_timing, %s), sizeof(((sgn_drain_take_timing*)0)->%s));'
                     % (f, f))
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgn.h"\nint main(void) {\n' + "\n".join(lines) +
                   "\nreturn 0;\n}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    out = [tuple(map(int, ln.split())) for ln in
           subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()]
    assert out[0] == (C.sizeof(sgn.DrainTakeTiming), C.sizeof(sgn.DrainRec), C.sizeof(sgn.TraceSpan)) == (104, 48, 24)
    for k, f in enumerate(TIMING_FIELDS, start=1):
        d = getattr(sgn.DrainTakeTiming, f)
        assert out[k] == (d.offset, d.size), (f, out[k])
    assert [n for n, _ in sgn.DrainTakeTiming._fields_] == list(TIMING_FIELDS)
    assert len(sgn.DrainTakeTiming().kernel_ms) == 4 and len(sgn.DrainTakeTiming().spans_by_class) == 3
