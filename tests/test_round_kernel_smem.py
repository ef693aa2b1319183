"""No scalar load of a DevSim field on the TGEN round kernel's event path (CPU only).

k_rounds<TGEN, *> keeps DevSim in the lanes of four vector registers, filled once at kernel
entry, and reads a uniform field with v_readlane_b32 (csrc/sgn_internal.h, SK() in engine.hip).
Read from memory, each use was a scalar load waited for on the spot: the parent of this change
had 262 s_load_dword* in k_rounds<TGEN, false>, 250 of them on the one DevSim pointer, 219
followed by their s_waitcnt within five instructions (tools/isa_census.py --smem).

The test compiles engine.hip to an assembly listing the way test_kernel_budget.py does and asks
that no scalar load is attributed — by its own source line or by any call site of its inlining
chain — to HostExec, exec_group, rb_edge, rb_arrive, rb_bookkeep or the body of the round loop,
in both TGEN instantiations. The ranges come from the function signatures in the source.
"""
import importlib.util
import pathlib
import re

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "shadow-gen_amd" / "csrc"
KERNELS = {
    "k_rounds<TGEN, false>": "_ZN3sgn8k_roundsILj2ELb0EEEvPKNS_6DevSimEjjj",
    "k_rounds<TGEN, true>": "_ZN3sgn8k_roundsILj2ELb1EEEvPKNS_6DevSimEjjj",
}
PARENT_LOADS = 262  # k_rounds<TGEN, false> before the table

# Loads that may stay, by the function whose own source line they carry: (name, reason).
ALLOW = [
    ("fail_timeout", "a workgroup that gives up on a grid barrier (OVF_TIMEOUT) and leaves the launch: runs at "
                     "most once per workgroup, after a wait of seconds; it takes the struct in memory (sk_mem)"),
]
assert len(ALLOW) <= 8

pytestmark = pytest.mark.skipif(not pathlib.Path("/opt/rocm/bin/hipcc").exists(), reason="hipcc absent")


def _code_lines():
    """engine.hip's lines with // comments removed (for brace matching)."""
    return [ln.split("//")[0] for ln in (CSRC / "engine.hip").read_text().splitlines()]


def _block(lines, start):
    """(first, last) line numbers (1-based) of the brace block that opens at or after line `start`."""
    depth, opened = 0, False
    for i in range(start - 1, len(lines)):
        for ch in lines[i]:
            if ch == "{":
                depth += 1
                opened = True
            elif ch == "}":
                depth -= 1
        if opened and depth == 0:
            return start, i + 1
        if not opened and ";" in lines[i]:
            raise AssertionError(f"line {start}: a declaration, not a definition")
    raise AssertionError(f"line {start}: block not closed")


def _find(lines, pattern):
    hits = [i + 1 for i, ln in enumerate(lines) if re.search(pattern, ln)]
    assert len(hits) == 1, (pattern, hits)
    return hits[0]


def _ranges():
    lines = _code_lines()
    r = {
        "HostExec": _block(lines, _find(lines, r"^struct HostExec\b")),
        "exec_group": _block(lines, _find(lines, r"^__device__ .*\bvoid exec_group\(")),
        "rb_edge": _block(lines, _find(lines, r"^__device__ .*\bRbEdge rb_edge\(")),
        "rb_arrive": _block(lines, _find(lines, r"^__device__ .*\bvoid rb_arrive\(")),
        "rb_bookkeep": _block(lines, _find(lines, r"^__device__ .*\bvoid rb_bookkeep\(")),
        "fail_timeout": _block(lines, _find(lines, r"^__device__ .*\bvoid fail_timeout\(")),
    }
    body = _block(lines, _find(lines, r"^__device__ .*\bvoid rounds_body\("))
    loop = [i for i in range(body[0], body[1] + 1) if re.search(r"for \(; r < max_rounds; r\+\+\) \{", lines[i - 1])]
    assert len(loop) == 1, loop
    r["round loop"] = _block(lines, loop[0])
    assert body[0] < r["round loop"][0] < r["round loop"][1] < body[1]
    return r


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("isa_census", ROOT / "tools" / "isa_census.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    asm = tmp_path_factory.mktemp("smem") / "engine.s"
    mod.compile_asm(CSRC / "engine.hip", asm)
    return mod, asm


def test_ranges_come_from_the_source():
    r = _ranges()
    for name, (a, b) in r.items():
        assert b > a, (name, a, b)
    assert r["HostExec"][1] - r["HostExec"][0] > 1000 and r["exec_group"][1] - r["exec_group"][0] > 500, r


@pytest.mark.parametrize("name", list(KERNELS))
def test_no_scalar_load_on_the_event_path(listing, name):
    mod, asm = listing
    loads = mod.smem(asm, KERNELS[name])
    assert 0 < len(loads) < PARENT_LOADS // 4, len(loads)  # (the kernel was found: its argument loads remain)
    r = _ranges()
    watched = ("HostExec", "exec_group", "rb_edge", "rb_arrive", "rb_bookkeep", "round loop")
    allowed = {a for a, _ in ALLOW}

    def inside(file, line, rng):
        return file == "engine.hip" and rng[0] <= line <= rng[1]

    bad = []
    for e in loads:
        if any(inside(e["file"], e["line"], r[a]) for a in allowed):
            continue
        sites = [(e["file"], e["line"])] + [tuple(c) for c in e["chain"]]
        hit = [w for w in watched if any(inside(f, ln, r[w]) for f, ln in sites)]
        if hit:
            bad.append((hit, e["file"], e["line"], e["op"], e["base"], e["offset"], e["chain"]))
    print(name, len(loads), "scalar loads:", [(e["file"], e["line"], e["base"], e["offset"], e["wait"]) for e in loads])
    assert not bad, bad


def test_parent_form_still_has_them(listing):
    # the attribution works: a kernel built without the table (PERIODIC keeps S.field) has its
    # scalar loads in the same ranges
    mod, asm = listing
    loads = mod.smem(asm, "_ZN3sgn8k_roundsILj1ELb0EEEvPKNS_6DevSimEjjj")
    r = _ranges()
    n = sum(1 for e in loads
            if any(f == "engine.hip" and r["HostExec"][0] <= ln <= r["HostExec"][1]
                   for f, ln in [(e["file"], e["line"])] + [tuple(c) for c in e["chain"]]))
    assert n > 50, (n, len(loads))
