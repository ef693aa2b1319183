"""The snapshot-file entry points of the C ABI (CPU only: no GPU calls): the sgn_snapshot_export /
_import family and the digest hooks are exported, refuse null arguments without touching a device,
leave the ABI version alone (they are additive), and the host form of the section digest is the
formula of include/sgn.h, restated here in numpy."""
import ctypes as C
import pathlib
import re
import subprocess

import numpy as np
import pytest

import sgn

EINVAL, ENOENT, EFILE = -22, -2, -74
NAMES = ("sgn_snapshot_export", "sgn_snapshot_import", "sgn_snapshot_export_file", "sgn_snapshot_import_file",
         "sgn_snapshot_file_info_get", "sgn_digest_bytes", "sgn_selftest_digest", "sgn_snapshot_file_timing_get")
GOLD = np.uint64(0x9E3779B97F4A7C15)
SEED = 0x5EED5EED5EED5EED  # SGN_DIGEST_SEED (sgn_workload.h)


def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def np_digest(buf):
    """D = mix64(len ^ seed) + sum_j mix64(w_j ^ (gold * (j + 1))) mod 2^64 over the little-endian
    u64 words of buf, a 4-byte tail zero-extended (uint64 arrays wrap, as the formula asks)."""
    b = bytes(buf)
    assert len(b) % 4 == 0
    w = np.frombuffer(b + b"\0" * (-len(b) % 8), dtype="<u8")
    with np.errstate(over="ignore"):
        keys = GOLD * np.arange(1, len(w) + 1, dtype=np.uint64)
        terms = _mix64(w ^ keys)
        head = _mix64(np.array([len(b) ^ SEED], dtype=np.uint64))
        return int((head.sum() + terms.sum(dtype=np.uint64)) & np.uint64(0xFFFFFFFFFFFFFFFF))


def test_library_exports_snapshot_files(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", str(sgn.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (sgn_[a-z0-9_]+)", out))
    for n in NAMES:
        assert n in exported, n
        assert hasattr(lib, n)
    assert lib.sgn_abi_version() == 10


def test_null_arguments_are_refused(lib):
    snap = C.c_void_p(1)
    n = C.c_uint64(7)
    info = sgn.SnapshotFileInfo()
    wr = sgn.WRITE_FN(lambda u, d, k: 0)
    rd = sgn.READ_FN(lambda u, d, k: 0)
    assert lib.sgn_snapshot_export(None, None, wr, None, C.byref(n)) == EINVAL and n.value == 0
    assert lib.sgn_snapshot_export(None, None, sgn.WRITE_FN(0), None, None) == EINVAL
    assert lib.sgn_snapshot_import(None, rd, None, C.byref(snap)) == EINVAL and not snap.value
    assert lib.sgn_snapshot_import(None, sgn.READ_FN(0), None, None) == EINVAL
    assert lib.sgn_snapshot_export_file(None, None, b"/nonexistent/x", None) == EINVAL
    snap = C.c_void_p(1)
    assert lib.sgn_snapshot_import_file(None, b"/nonexistent/x", C.byref(snap)) == EINVAL and not snap.value
    assert lib.sgn_snapshot_import_file(None, None, None) == EINVAL
    assert lib.sgn_snapshot_file_info_get(None, C.byref(info)) == EINVAL
    assert lib.sgn_snapshot_file_info_get(b"x", None) == EINVAL
    assert lib.sgn_selftest_digest(None, None, 0, C.byref(n)) == EINVAL
    assert lib.sgn_snapshot_file_timing_get(None, None) == EINVAL


def test_file_info_layout_matches_header(tmp_path):
    root = pathlib.Path(__file__).resolve().parent.parent
    fields = [n for n, _ in sgn.SnapshotFileInfo._fields_]
    tfields = [n for n, _ in sgn.SnapshotFileTiming._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "sgn.h"\nint main(void) {\n'
                   '  printf("%zu %zu", sizeof(sgn_snapshot_file_info), sizeof(sgn_snapshot_file_timing));\n'
                   + "".join(f'  printf(" %zu", offsetof(sgn_snapshot_file_info, {f}));\n' for f in fields)
                   + "".join(f'  printf(" %zu", offsetof(sgn_snapshot_file_timing, {f}));\n' for f in tfields)
                   + '  printf(" %d\\n", SGN_EFILE);\n  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", str(root / "include"), str(src), "-o", str(exe)], check=True)
    v = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert v[0] == C.sizeof(sgn.SnapshotFileInfo) and v[1] == C.sizeof(sgn.SnapshotFileTiming)
    offs = v[2:-1]
    assert offs[:len(fields)] == [getattr(sgn.SnapshotFileInfo, f).offset for f in fields]
    assert offs[len(fields):] == [getattr(sgn.SnapshotFileTiming, f).offset for f in tfields]
    assert v[-1] == EFILE == sgn.EFILE


def test_file_info_refuses_what_is_no_snapshot_file(lib, tmp_path):
    with pytest.raises(sgn.SgnError) as e:
        sgn.snapshot_file_info(tmp_path / "missing.snap")
    assert e.value.rc == ENOENT
    cases = {"empty": b"", "seven": b"SGNSNAP", "magic": b"SGNSNAP2" + bytes(4096),
             "header-only": b"SGNSNAP1" + bytes(280)}
    for name, content in cases.items():
        p = tmp_path / name
        p.write_bytes(content)
        with pytest.raises(sgn.SgnError) as e:
            sgn.snapshot_file_info(p)
        assert e.value.rc == EFILE, name


@pytest.mark.parametrize("n", [0, 4, 8, 12, 16, 20, 4096 + 4])
def test_digest_bytes_is_the_formula(lib, n):
    b = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
    assert sgn.digest_bytes(b) == np_digest(b)
    assert sgn.digest_bytes(np.frombuffer(b, dtype=np.uint8)) == np_digest(b)


def test_digest_bytes_is_keyed_by_position(lib):
    w = np.random.default_rng(1).integers(1, 1 << 62, 64, dtype=np.uint64)
    base = sgn.digest_bytes(w)
    assert base == np_digest(w.tobytes())
    sw = w.copy()
    sw[[3, 40]] = sw[[40, 3]]  # two words swap
    assert sgn.digest_bytes(sw) != base and sgn.digest_bytes(sw) == np_digest(sw.tobytes())
    z = w.copy()
    z[5] = 0
    z2 = w.copy()
    z2[5], z2[6] = w[6], 0      # the zero word moves: (0, a) -> (a, 0)
    z[6] = w[6]
    assert sgn.digest_bytes(z) != sgn.digest_bytes(z2)
    assert sgn.digest_bytes(bytes(8)) != sgn.digest_bytes(bytes(16))  # zeros of different lengths
    assert lib.sgn_digest_bytes(None, 0) == np_digest(b"")
    assert lib.sgn_digest_bytes(None, 8) == 0 and sgn.digest_bytes(bytes(6)) == 0  # refused: 0
