"""Static budget of the flagship round kernel, k_rounds<TGEN, false> (CPU only).

The round is latency-bound on its slowest waves' instruction stream, so what the compiler
makes of the event path is part of the product: no general 64-bit division (a ~140-instruction
software routine per inlined copy) and fewer SGPR spills than before the divisions left.

Bounds: the figures of commit 7fa1680 (the parent of the change that removed the divisions),
taken with tools/isa_census.py from the same compiler: 17,610 instructions, 285 SGPR spills,
418 v_mad_u64_u32; its three division lines (tb_remove_'s req / inc, cq_free_page's
j % S.cq_pages, div_small's a / b) cost 137-146 instructions per inlined copy, a u32 division
costs 28. The figures reached are in DESIGN.md section 4 (round 7).
"""
import importlib.util
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "shadow-gen_amd" / "csrc"
LLVM = pathlib.Path("/opt/rocm/lib/llvm/bin")
KERNEL = "_ZN3sgn8k_roundsILj2ELb0EEEvPKNS_6DevSimEjjj"

PARENT_SGPR_SPILLS = 285      # 7fa1680
PARENT_INSTRUCTIONS = 17610   # 7fa1680
PARENT_MAD_U64 = 418          # 7fa1680
# between a u32 division (28 instructions a copy) and the u64 routine (137 and up)
DIV_COPY_MAX = 60

pytestmark = pytest.mark.skipif(not (LLVM / "clang-offload-bundler").exists(), reason="ROCm LLVM tools absent")


def _notes(so, tmp):
    """{kernel name: {metadata key: int}} of the gfx950 code objects bundled into a library."""
    fb = tmp / "fb.bin"
    subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", str(so), str(fb)], check=True)
    data = fb.read_bytes()
    offs = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), data)]
    out = {}
    for i, o in enumerate(offs):
        b, co = tmp / f"b{i}.bin", tmp / f"b{i}.co"
        b.write_bytes(data[o:offs[i + 1] if i + 1 < len(offs) else len(data)])
        r = subprocess.run([str(LLVM / "clang-offload-bundler"), "--unbundle", "--type=o", f"--input={b}",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={co}"], capture_output=True)
        if r.returncode:
            continue
        text = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True, text=True,
                              check=True).stdout
        # one YAML map per kernel, opened by a list item at two spaces; keys sorted
        for block in re.split(r"\n  - \.", text):
            name = re.search(r"\n\s+\.name:\s+(\S+)", block)
            if name:
                out[name.group(1)] = {k: int(v) for k, v in re.findall(r"\n\s+\.(\w+):\s+(\d+)\s*(?=\n)", block)}
    return out


def test_flagship_round_kernel_spills_fewer_sgprs(tmp_path):
    meta = _notes(ROOT / "shadow-gen_amd" / "libsgn.so", tmp_path)
    assert KERNEL in meta, sorted(meta)[:5]
    m = meta[KERNEL]
    print(KERNEL, m)
    assert m["sgpr_spill_count"] < PARENT_SGPR_SPILLS, m
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m


@pytest.fixture(scope="module")
def census(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("isa_census", ROOT / "tools" / "isa_census.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    asm = tmp_path_factory.mktemp("census") / "engine.s"
    mod.compile_asm(CSRC / "engine.hip", asm)
    return mod.census(asm, KERNEL)


def _division_lines():
    """(file, line) of every source line of the engine with a / or % operator outside comments."""
    out = []
    for p in (CSRC / "engine.hip", CSRC / "sgn_internal.h"):
        for i, ln in enumerate(p.read_text().splitlines(), 1):
            code = ln.split("//")[0]
            if re.search(r"[\w)\]]\s*[/%]\s*[\w(]", code) and not code.lstrip().startswith(("#", "*")):
                out.append((p.name, i))
    return out


def test_flagship_round_kernel_has_no_u64_division(census):
    t = census["totals"]
    print({k: t.get(k) for k in ("instructions", "VALU", "SALU", ".sgpr_spill_count", "v_mad_u64_u32", "v_rcp_*")})
    assert 0 < t["instructions"] < PARENT_INSTRUCTIONS, t
    assert t["v_mad_u64_u32"] < PARENT_MAD_U64, t
    lines = _division_lines()
    assert len(lines) > 10  # (the scan finds the engine's divisions)
    seen = 0
    for key in lines:
        for chain, n in census["copies"].get(key, {}).items():
            seen += 1
            assert n <= DIV_COPY_MAX, (key, n, chain)
    assert seen > 0  # (and some of them are in this kernel: the attribution works)
