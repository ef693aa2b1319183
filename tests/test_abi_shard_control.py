"""The collective run-control entry points of the C ABI (CPU only: no GPU calls):
sgn_shards_run_until, sgn_shards_snapshot_save and sgn_shards_snapshot_restore are exported, refuse
null arguments without touching a device, and leave the ABI version alone (they are additive)."""
import ctypes as C
import re
import subprocess

import sgn

EINVAL = -22
NAMES = ("sgn_shards_run_until", "sgn_shards_snapshot_save", "sgn_shards_snapshot_restore")


def test_library_exports_shard_control(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(sgn.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (sgn_[a-z0-9_]+)", out))
    for n in NAMES:
        assert n in exported, n
        assert hasattr(lib, n)
    assert lib.sgn_abi_version() == 10


def test_null_arguments_are_refused(lib):
    done = C.c_uint64(7)
    one = (C.c_void_p * 1)()  # an array of one null context
    snaps = (C.c_void_p * 1)()
    t = sgn.SIMULATION_START + 1
    assert lib.sgn_shards_run_until(None, 2, t, C.byref(done)) == EINVAL and done.value == 0
    assert lib.sgn_shards_run_until(None, 0, t, None) == EINVAL
    assert lib.sgn_shards_run_until(one, 1, t, None) == EINVAL
    assert lib.sgn_shards_run_until(one, 0, t, None) == EINVAL
    assert lib.sgn_shards_snapshot_save(None, 2, snaps) == EINVAL
    assert lib.sgn_shards_snapshot_save(one, 1, None) == EINVAL
    assert lib.sgn_shards_snapshot_save(one, 1, snaps) == EINVAL and not snaps[0]
    assert lib.sgn_shards_snapshot_restore(None, 2, snaps) == EINVAL
    assert lib.sgn_shards_snapshot_restore(one, 1, None) == EINVAL
    assert lib.sgn_shards_snapshot_restore(one, 1, snaps) == EINVAL


def test_python_binding_has_the_module_functions():
    for n in ("shards_run_until", "shards_snapshot_save", "shards_snapshot_restore"):
        assert callable(getattr(sgn, n)), n
