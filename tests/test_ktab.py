"""The round kernel's lane table on the host (CPU only).

k_rounds<TGEN, *> keeps DevSim in the lanes of four vector registers and reads a uniform field
with one constant-lane v_readlane_b32 per dword (csrc/sgn_internal.h: ktab_src for the fill,
ktab_reg / ktab_lane for the accessor). tests/native/ktab_check.cpp packs a DevSim with a
different value in every dword into the table's image with the same arithmetic and reads every
field of the accessor's list back — u32, u64, pointers, the UDiv64 members, the array elements,
and a field placed by hand across each 256-byte register boundary."""
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _build(tmp_path, name, *flags):
    exe = tmp_path / name
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", *flags,
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "shadow-gen_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "ktab_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    return exe


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 bad" in out.stdout, out.stdout
    assert int(out.stdout.split()[0]) > 500, out.stdout  # dwords + fields + straddling reads


def test_lane_table_reads_every_field(tmp_path):
    _run(_build(tmp_path, "ktab_check", "-O2"))


def test_lane_table_host_twin_is_clean_under_sanitizers(tmp_path):
    # the same stand-alone program with its host code under UBSan and ASan (the packed image's
    # indexing, the clamped fill, the straddling reads): any report aborts it
    _run(_build(tmp_path, "ktab_check_san", "-O1", "-Xarch_host", "-fsanitize=undefined,address",
                "-Xarch_host", "-fno-sanitize-recover=undefined"))
