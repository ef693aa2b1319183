#!/usr/bin/env python3
"""Static instruction census of one kernel from the compiler's assembly listing.

Where do a kernel's instructions come from? Compile the source for the device only, with the
Makefile's flags plus line tables, and attribute every instruction to the source line of its
innermost `.loc` (an inlined helper's own line, summed over its inlined copies):

    python tools/isa_census.py --compile shadow-gen_amd/csrc/engine.hip -o engine.s
    python tools/isa_census.py engine.s [--kernel MANGLED] [--top 20] [--json]

Output: the kernel's totals (instructions by unit, SGPR spills, scalar loads, ...) and the
largest source lines. `--per-copy` lists, for the chosen lines, the instructions of each
inlined copy (one copy = one distinct inlining chain), which is what tells a 64-bit software
division (~90+ instructions a copy) from a 32-bit one (~30).

`--smem` lists every scalar load of the kernel instead: its source line and inlining chain, its
base register and offset, and how many instructions later the first `s_waitcnt lgkmcnt(..)`
follows in the listing (a load waited for at once stalls the wave's only instruction stream for
a scalar-cache round trip), with a summary per base register:

    python tools/isa_census.py engine.s --smem [--kernel MANGLED] [--json]

`--same A.s B.s` answers whether two builds have the same kernels (a refactor of the host code
must not change one): every function symbol of both listings, its instruction stream compared
with the comments stripped and the numbers of local labels blanked. With `--blank-regs` the
line-table labels, register numbers and spill lanes are ignored too, and a differing pair's places
are listed: where a refactor of device code moved instructions, and that it moved no others.
"""
import argparse
import collections
import json
import pathlib
import re
import subprocess
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
TGEN_ROUNDS = "_ZN3sgn8k_roundsILj2ELb0EEEvPKNS_6DevSimEjjj"  # k_rounds<TGEN, false>: config C
# the Makefile's CXXFLAGS (device side), plus line tables
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off",
         "-gline-tables-only", "--cuda-device-only", "-S"]

_LOC = re.compile(r"^\s*\.loc\s+(\d+)\s+(\d+)\s+\d+(.*)$")
_FILE = re.compile(r'^\s*\.file\s+(\d+)\s+"[^"]*"\s+"([^"]+)"')
_FILE1 = re.compile(r'^\s*\.file\s+(\d+)\s+"([^"]+)"')
_INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b")
_CHAIN = re.compile(r"@\[\s*(.*?)\s*\]\s*$")


def compile_asm(src, out, hipcc="/opt/rocm/bin/hipcc"):
    src = pathlib.Path(src).resolve()
    subprocess.run([hipcc, *FLAGS, "-I", str(ROOT / "include"), "-I", str(src.parent), src.name,
                    "-o", str(pathlib.Path(out).resolve())], check=True, cwd=src.parent,
                   capture_output=True)


def _unit(op):
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    return "other"


def census(asm_path, kernel=TGEN_ROUNDS):
    """{'totals': {...}, 'lines': {(file, line): n}, 'copies': {(file, line): {chain: n}},
    'salu_lines': {(file, line): n}} for one kernel of an assembly listing."""
    files = {}
    totals = collections.Counter()
    lines = collections.Counter()
    salu = collections.Counter()
    copies = collections.defaultdict(collections.Counter)
    meta = {}
    inside = False
    cur = ("?", 0)
    chain = ""
    with open(asm_path, errors="replace") as f:
        for ln in f:
            m = _FILE.match(ln) or _FILE1.match(ln)
            if m:
                files[int(m.group(1))] = pathlib.Path(m.group(2)).name
                continue
            if not inside:
                if ln.startswith(kernel + ":"):
                    inside = True
                elif ln.startswith("    .name:") and ln.split()[-1] == kernel:
                    meta["_hit"] = True
                elif ln.startswith("  - ."):
                    if meta.get("_hit"):
                        break
                    meta = {}
                else:
                    m = re.match(r"\s+\.(sgpr_spill_count|vgpr_spill_count|vgpr_count|sgpr_count|"
                                 r"private_segment_fixed_size|group_segment_fixed_size):\s+(\d+)", ln)
                    if m:
                        meta[m.group(1)] = int(m.group(2))
                continue
            if ln.startswith(".Lfunc_end"):
                inside = False
                continue
            m = _LOC.match(ln)
            if m:
                cur = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
                c = _CHAIN.search(m.group(3))
                chain = c.group(1) if c else ""
                continue
            m = _INSN.match(ln)
            if not m or ln.lstrip().startswith((".", ";")):
                continue
            op = m.group(1)
            totals["instructions"] += 1
            totals[_unit(op)] += 1
            lines[cur] += 1
            copies[cur][chain] += 1
            if op.startswith("s_"):
                salu[cur] += 1
            for key, pat in (("v_writelane", "v_writelane"), ("v_readlane", "v_readlane"), ("s_nop", "s_nop"),
                             ("s_load_dword*", "s_load_dword"), ("v_mad_u64_u32", "v_mad_u64_u32"),
                             ("v_rcp_*", "v_rcp_"), ("s_waitcnt", "s_waitcnt")):
                if op.startswith(pat):
                    totals[key] += 1
    meta.pop("_hit", None)
    for k, v in meta.items():
        totals["." + k] = v
    return {"totals": dict(totals), "lines": dict(lines), "copies": {k: dict(v) for k, v in copies.items()},
            "salu_lines": dict(salu)}


_SLOAD = re.compile(r"^\s+(s_(?:buffer_)?load_dword\w*)\s+([^,]+),\s*([^,]+),\s*(\S+)")
_CHAIN_ENT = re.compile(r"([^\s@\[\]]+):(\d+):\d+")


def smem(asm_path, kernel=TGEN_ROUNDS):
    """Every scalar load of one kernel, in listing order: [{'op', 'dst', 'base', 'offset', 'file',
    'line', 'chain': [(file, line), ...] (the inlining call sites, innermost first), 'wait': the
    instructions from the load to the next s_waitcnt that names lgkmcnt (1: the very next one;
    None: none before the function ends)}]. The distance follows the listing, not the branches."""
    files = {}
    out, pending = [], []
    inside = False
    cur, chain = ("?", 0), []
    with open(asm_path, errors="replace") as f:
        for ln in f:
            m = _FILE.match(ln) or _FILE1.match(ln)
            if m:
                files[int(m.group(1))] = pathlib.Path(m.group(2)).name
                continue
            if not inside:
                inside = ln.startswith(kernel + ":")
                continue
            if ln.startswith(".Lfunc_end"):
                break
            m = _LOC.match(ln)
            if m:
                cur = (files.get(int(m.group(1)), m.group(1)), int(m.group(2)))
                c = _CHAIN.search(m.group(3))
                chain = [(pathlib.Path(a).name, int(b)) for a, b in _CHAIN_ENT.findall(c.group(1))] if c else []
                continue
            m = _INSN.match(ln)
            if not m or ln.lstrip().startswith((".", ";")):
                continue
            for p in pending:
                p["wait"] += 1
            if m.group(1) == "s_waitcnt" and "lgkmcnt" in ln:
                pending = []
            elif m.group(1) == "s_waitcnt" and re.match(r"\s+s_waitcnt\s+(0x[0-9a-f]+|\d+)\s*$", ln):
                pending = []  # (a raw immediate: counted as a wait for everything)
            s = _SLOAD.match(ln)
            if s:
                e = {"op": s.group(1), "dst": s.group(2).strip(), "base": s.group(3).strip(),
                     "offset": s.group(4).strip(), "file": cur[0], "line": cur[1], "chain": list(chain), "wait": 0}
                out.append(e)
                pending.append(e)
    for p in pending:
        p["wait"] = None
    return out


def smem_report(loads, srcs):
    t = collections.Counter()
    by_base = collections.defaultdict(set)
    for e in loads:
        by_base[e["base"]].add(e["offset"])
        t["loads"] += 1
        if e["wait"] is not None and e["wait"] <= 5:
            t["waited for within 5 instructions"] += 1
        if e["wait"] == 1:
            t["waited for by the next instruction"] += 1
    print("| measure | value |\n|---|---|")
    for k in ("loads", "waited for within 5 instructions", "waited for by the next instruction"):
        print(f"| {k} | {t.get(k, 0)} |")
    print("\n| base | loads | distinct offsets |\n|---|---|---|")
    for b, offs in sorted(by_base.items(), key=lambda kv: -len(kv[1])):
        print(f"| {b} | {sum(1 for e in loads if e['base'] == b)} | {len(offs)} |")
    print("\n| line | what it is | inlined into | op | base | offset | next wait |\n|---|---|---|---|---|---|---|")
    for e in loads:
        ch = " < ".join(f"{a}:{b}" for a, b in e["chain"]) or "-"
        print(f"| {e['file']}:{e['line']} | `{source_line(srcs, (e['file'], e['line']))}` | {ch} | {e['op']} | "
              f"{e['base']} | {e['offset']} | {e['wait'] if e['wait'] is not None else '-'} |")


_LABEL_NO = re.compile(r"\.(LBB|Lfunc_end|Lfunc_begin|Ltmp|LJTI|LCPI)[0-9_]+")


def functions(asm_path):
    """{symbol: [instruction and label lines]} of a listing, in listing order: comments (from ';')
    and directives dropped, the numbers of local labels blanked (they count functions and blocks
    of the whole file, so they shift when another function is added or the order changes)."""
    out = {}
    cur = None
    is_fn = set()
    with open(asm_path, errors="replace") as f:
        for ln in f:
            m = re.match(r"^\s*\.type\s+([^,\s]+),@function", ln)
            if m:
                is_fn.add(m.group(1))
                continue
            m = re.match(r"^([A-Za-z_][\w$.]*):", ln)
            if m and cur is None and m.group(1) in is_fn:
                cur = out.setdefault(m.group(1), [])
                continue
            if ln.startswith(".Lfunc_end"):
                cur = None
                continue
            if cur is None:
                continue
            s = _LABEL_NO.sub(lambda k: "." + k.group(1) + "_", ln.split(";")[0]).strip()
            if s and (not s.startswith(".") or s.startswith(".L")):
                cur.append(s)
    return out


_REG = re.compile(r"\b([sv])(\d+|\[\d+:\d+\])")
_SPILL_LANE = re.compile(r"^(v_(?:read|write)lane_b32 .*), \d+$")


def _blank(lines):
    """A stream with the line-table labels dropped and register numbers and SGPR spill lanes
    blanked: what is left differs only where the instructions themselves do."""
    return [_REG.sub(lambda k: k.group(1) + "#", _SPILL_LANE.sub(r"\1, #", x)) for x in lines if not x.startswith(".Ltmp_")]


def same(a_path, b_path, blank=False):
    """Compare two listings function by function; prints one line each and returns 0 when both
    hold the same symbols with identical instruction streams. blank: compare the blanked streams
    (_blank) and list where a differing pair parts, as A's line ranges START+LINES_A/LINES_B."""
    a, b = functions(a_path), functions(b_path)
    if blank:
        import difflib
        a, b = {k: _blank(v) for k, v in a.items()}, {k: _blank(v) for k, v in b.items()}
    bad = 0
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            print(f"ONLY IN {'A' if sym in a else 'B'}  {sym}")
            bad += 1
        elif blank and a[sym] != b[sym]:
            ops = [o for o in difflib.SequenceMatcher(None, a[sym], b[sym], autojunk=False).get_opcodes() if o[0] != "equal"]
            print(f"DIFFERENT  {sym}: {len(a[sym])} vs {len(b[sym])} lines, {len(ops)} places: "
                  + " ".join(f"{o[1]}+{o[2] - o[1]}/{o[4] - o[3]}" for o in ops))
            bad += 1
        elif a[sym] != b[sym]:
            first = next((i for i, (x, y) in enumerate(zip(a[sym], b[sym])) if x != y), min(len(a[sym]), len(b[sym])))
            print(f"DIFFERENT  {sym}: {len(a[sym])} vs {len(b[sym])} lines, first difference at line {first}")
            bad += 1
        else:
            print(f"same  {len(a[sym]):6d} lines  {sym}")
    print(f"{len(a)} functions in A, {len(b)} in B, {bad} differ")
    return 1 if bad else 0


def source_line(path_by_name, key):
    p = path_by_name.get(key[0])
    if not p or key[1] == 0:
        return "(compiler-made control flow and exec-mask glue)" if key[1] == 0 else ""
    try:
        return p.read_text(errors="replace").splitlines()[key[1] - 1].strip()[:70]
    except (OSError, IndexError):
        return ""


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", nargs="?")
    ap.add_argument("--compile", metavar="SRC", help="compile SRC (a .hip file) to the listing -o names, then stop")
    ap.add_argument("-o", default="engine.s")
    ap.add_argument("--kernel", default=TGEN_ROUNDS)
    ap.add_argument("--top", type=int, default=20)
    ap.add_argument("--per-copy", default="", help="comma-separated FILE:LINE list: instructions per inlined copy")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--smem", action="store_true", help="list the kernel's scalar loads instead of the census")
    ap.add_argument("--same", nargs=2, metavar=("A.s", "B.s"),
                    help="compare two listings function by function (exit status 1 when they differ)")
    ap.add_argument("--blank-regs", action="store_true",
                    help="with --same: ignore line-table labels, register numbers and spill lanes; list where streams part")
    a = ap.parse_args()
    if a.same:
        return same(*a.same, blank=a.blank_regs)
    if a.compile:
        compile_asm(a.compile, a.o)
        return 0
    if not a.asm:
        ap.error("an assembly listing, or --compile SRC")
    if a.smem:
        loads = smem(a.asm, a.kernel)
        if a.json:
            print(json.dumps(loads))
            return 0
        srcs = {p.name: p for p in (ROOT / "shadow-gen_amd" / "csrc").glob("*.h*")}
        srcs.update({p.name: p for p in (ROOT / "include").glob("*.h")})
        smem_report(loads, srcs)
        return 0
    c = census(a.asm, a.kernel)
    if not c["totals"]:
        print("kernel not found:", a.kernel, file=sys.stderr)
        return 1
    if a.json:
        print(json.dumps({"totals": c["totals"],
                          "lines": {f"{k[0]}:{k[1]}": v for k, v in c["lines"].items()}}))
        return 0
    srcs = {p.name: p for p in (ROOT / "shadow-gen_amd" / "csrc").glob("*.h*")}
    srcs.update({p.name: p for p in (ROOT / "include").glob("*.h")})
    t = c["totals"]
    print("| measure | value |\n|---|---|")
    for k in ("instructions", "VALU", "SALU", "LDS", "VMEM", "s_waitcnt", ".sgpr_spill_count", "v_writelane",
              "v_readlane", "s_nop", "s_load_dword*", ".vgpr_count", "v_mad_u64_u32", "v_rcp_*"):
        print(f"| {k} | {t.get(k, 0):,} |")
    print("\n| line | what it is | instr. | SALU | copies |\n|---|---|---|---|---|")
    for key, n in sorted(c["lines"].items(), key=lambda kv: -kv[1])[:a.top]:
        print(f"| {key[0]}:{key[1]} | `{source_line(srcs, key)}` | {n:,} | {c['salu_lines'].get(key, 0):,} | "
              f"{len(c['copies'][key])} |")
    for spec in filter(None, a.per_copy.split(",")):
        fn, _, ln = spec.rpartition(":")
        key = (fn, int(ln))
        print(f"\n{spec}: {c['lines'].get(key, 0)} instructions")
        for ch, n in sorted(c["copies"].get(key, {}).items(), key=lambda kv: -kv[1]):
            print(f"  {n:5d}  {ch or '(not inlined)'}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
