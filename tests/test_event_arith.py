"""The event path's division-free arithmetic against plain / and % (CPU only).

csrc/sgn_internal.h: umod64 (the CoDel free ring's index, counter mod cq_pages by a
reciprocal), tb_refills (refill intervals until a refused packet conforms), tb_quot and
tb_conforming (how many packets of a train a token bucket's balance covers). They replace
the general u64 division routine in the round kernels and must equal it on every input the
ABI admits; tests/native/event_arith_check.cpp walks the edge cases and a few million seeded
random pairs, and checks the batched removal against removals one after another."""
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent


def _build(tmp_path, name, *flags):
    exe = tmp_path / name
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", *flags,
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "shadow-gen_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "event_arith_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True)
    return exe


def test_event_arithmetic_matches_division(tmp_path):
    out = subprocess.run([str(_build(tmp_path, "event_arith_check", "-O2"))], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    assert " 0 bad" in out.stdout
    assert int(out.stdout.split()[0]) > 3_000_000, out.stdout


def test_event_arithmetic_has_no_undefined_behaviour(tmp_path):
    # the same stand-alone program with the host code under UBSan (shifts, overflow, the
    # f64 -> u64 conversion of tb_quot): any report aborts it
    exe = _build(tmp_path, "event_arith_check_ub", "-O1", "-Xarch_host", "-fsanitize=undefined",
                 "-Xarch_host", "-fno-sanitize-recover=undefined")
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 bad" in out.stdout
