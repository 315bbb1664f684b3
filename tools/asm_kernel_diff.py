"""Compare two gfx950 device assembly files (hipcc --cuda-device-only -S) kernel by kernel.

    python tools/asm_kernel_diff.py PARENT.s BRANCH.s [--rename OLD=NEW ...]

For every kernel: the instruction text, the kernel descriptor (.amdhsa_* block) and the resource metadata (registers, scratch,
LDS, kernarg size) are compared after the kernel's own symbol, the function numbers in local labels and the compilation unit's
`__hip_cuid_*` symbol are normalised away.  Kernels are matched by demangled name; --rename rewrites a substring of the parent's
demangled names first (a kernel that moved or gained a template argument).  Prints one line per differing kernel and a summary;
exit status 1 when anything differs or a kernel has no partner."""
import argparse
import difflib
import re
import shutil
import subprocess
import sys

_META = (".sgpr_count", ".vgpr_count", ".agpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size",
         ".kernarg_segment_size", ".wavefront_size", ".max_flat_workgroup_size", ".sgpr_spill_count", ".vgpr_spill_count")


def _demangle(names):
    out = subprocess.run([shutil.which("llvm-cxxfilt") or "c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return [re.sub(r"\((?!anonymous namespace\)).*$", "", n) for n in out.stdout.splitlines()]   # without the argument list


def _norm(line, sym):
    line = line.replace(sym, "K")
    line = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", line)
    return re.sub(r";.*$", "", line).rstrip()


def parse(path):
    """{mangled: {"text": [...], "desc": [...], "meta": {...}}}"""
    lines = open(path).read().splitlines()
    kernels = {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            sym = m.group(1)
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            kernels.setdefault(sym, {})["desc"] = [_norm(x, sym) for x in lines[i:j]]
            i = j
        i += 1
    for sym, k in kernels.items():
        beg = next(n for n, x in enumerate(lines) if x.startswith(sym + ":"))
        end = beg
        while not re.match(r"\.Lfunc_end\d+:", lines[end]):
            end += 1
        k["text"] = [t for t in (_norm(x, sym) for x in lines[beg + 1:end]) if t.strip()]
        k["meta"] = {}
    # metadata: one YAML entry per kernel ("  - .key:" opens it); its .name may come after the resource keys
    entry = {}
    for x in lines + ["  - .end:"]:
        if re.match(r"  - \.", x):
            if entry.get(".name") in kernels:
                kernels[entry[".name"]]["meta"] = {k: v for k, v in entry.items() if k in _META}
            entry = {}
        m = re.match(r"  [ -] (\.\w+):\s*(\S+)\s*$", x)
        if m:
            entry[m.group(1)] = m.group(2)
    return kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--rename", action="append", default=[], help="OLD=NEW on the parent's demangled kernel names")
    ap.add_argument("--show", type=int, default=0, help="print up to this many diff lines per differing kernel")
    a = ap.parse_args()
    sides = []
    for path in (a.parent, a.branch):
        ks = parse(path)
        syms = list(ks)
        sides.append(dict(zip(_demangle(syms), (ks[s] for s in syms))))
    parent, branch = sides
    for r in a.rename:
        old, new = r.split("=", 1)
        parent = {re.sub(old, new, n): k for n, k in parent.items()}
    bad = 0
    for name in sorted(set(parent) | set(branch)):
        if name not in parent or name not in branch:
            print(f"UNMATCHED ({'branch' if name in branch else 'parent'} only): {name}")
            bad += 1
            continue
        p, b = parent[name], branch[name]
        d_text = [x for x in difflib.unified_diff(p["text"], b["text"], lineterm="", n=0) if x[:1] in "+-" and x[:3] not in ("+++", "---")]
        d_desc = [x for x in difflib.unified_diff(p["desc"], b["desc"], lineterm="", n=0) if x[:1] in "+-" and x[:3] not in ("+++", "---")]
        if d_text or d_desc or p["meta"] != b["meta"]:
            bad += 1
            res = " ".join(f"{k[1:]}={p['meta'].get(k)}/{b['meta'].get(k)}" for k in _META[:6])
            print(f"DIFF {name}: {len(p['text'])} instruction lines, {len(d_text)} differ, descriptor lines differ {len(d_desc)}; parent/branch {res}")
            for x in (d_text + d_desc)[:a.show]:
                print("    " + x)
    print(f"{len(branch)} kernels in the branch, {len(parent)} in the parent, {bad} differ or unmatched")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
