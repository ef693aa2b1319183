"""The run-control entry points of the C ABI (CPU only: no GPU calls): sgn_run_until and the
sgn_snapshot_* family are exported, refuse null arguments without touching a device, and leave
the ABI version alone (they are additive)."""
import ctypes as C
import re
import subprocess

import sgn

EINVAL = -22
NAMES = ("sgn_snapshot_save", "sgn_snapshot_restore", "sgn_snapshot_free", "sgn_snapshot_info_get",
         "sgn_run_until")


def test_library_exports_run_control(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(sgn.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (sgn_[a-z0-9_]+)", out))
    # (the sixth name of the family is the opaque type sgn_snapshot itself)
    for n in NAMES:
        assert n in exported, n
        assert hasattr(lib, n)
    assert lib.sgn_abi_version() == 10


def test_null_arguments_are_refused(lib):
    snap = C.c_void_p()
    done = C.c_uint64(7)
    info = sgn.SnapshotInfo()
    assert lib.sgn_snapshot_save(None, C.byref(snap)) == EINVAL and not snap.value
    assert lib.sgn_snapshot_save(None, None) == EINVAL
    assert lib.sgn_snapshot_restore(None, None) == EINVAL
    assert lib.sgn_run_until(None, sgn.SIMULATION_START + 1, C.byref(done)) == EINVAL
    assert lib.sgn_run_until(None, 0, None) == EINVAL
    assert lib.sgn_snapshot_info_get(None, C.byref(info)) == EINVAL
    assert lib.sgn_snapshot_info_get(None, None) == EINVAL
    assert lib.sgn_snapshot_free(None, None) is None  # returns


def test_snapshot_info_layout_matches_header(tmp_path):
    import pathlib
    root = pathlib.Path(__file__).resolve().parent.parent
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgn.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(sgn_snapshot_info), offsetof(sgn_snapshot_info, save_ms),\n'
                   '         offsetof(sgn_snapshot_info, calendar_pool_bytes));\n  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    size, off_ms, off_pool = map(int, subprocess.run([str(exe)], capture_output=True, text=True,
                                                     check=True).stdout.split())
    assert size == C.sizeof(sgn.SnapshotInfo)
    assert off_ms == sgn.SnapshotInfo.save_ms.offset
    assert off_pool == sgn.SnapshotInfo.calendar_pool_bytes.offset
