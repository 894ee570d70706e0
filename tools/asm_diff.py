#!/usr/bin/env python3
"""Compare two `make asm` listings per symbol: is the generated code of a refactor the parent's?

usage: tools/asm_diff.py PARENT.s THIS.s [--only SUBSTRING]

For every kernel of either listing (the entries of the amdhsa.kernels metadata) one row: whether the normalised
instruction streams are identical, the instruction counts, and the metadata fields that decide residency.  The
out-of-line device functions (symbols of type @function that are no kernel) follow with their streams alone.
A stream is normalised by dropping comments, directives and blank lines and the numbers of local labels
(.LBB12_3 -> .LBB), so that code which merely moved inside the file compares equal.  The script looks at no
particular instruction.  Exit status 1 if the symbol sets differ or a metadata field of a kernel rose; a field that
fell (fewer registers, less LDS) is shown as parent>this and counted in the last line, and costs no residency.

The parent's listing comes from a clean export of the parent commit, as tools/build_commit_variant.sh does it:
    d=$(mktemp -d); git archive HEAD dirt_amd/csrc include Makefile | tar -x -C $d; make -C $d asm NAME=parent
"""
import argparse
import re
import shutil
import subprocess
import sys

FIELDS = (".sgpr_count", ".vgpr_count", ".agpr_count", ".sgpr_spill_count", ".vgpr_spill_count",
          ".private_segment_fixed_size", ".group_segment_fixed_size")
SHORT = ("sgpr", "vgpr", "agpr", "s_spill", "v_spill", "private", "lds")
LOCAL_LABEL = re.compile(r"\.L[A-Za-z_]+[0-9_]+")


def parse(path):
    """-> ({symbol: [normalised instruction lines]}, {kernel symbol: {field: int}})"""
    streams, meta, functions = {}, {}, set()
    cur, entry, in_meta = None, None, False
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].strip()
        if in_meta:
            # one "  - " list entry per kernel; its own keys sit at four columns, those of its arguments deeper
            m = re.match(r"  (?:- |  )(\.[a-z_]+):\s*(\S*)", raw)
            if raw.startswith("  - "):
                entry = {}
            if line.startswith(".end_amdgpu_metadata") or raw.startswith("amdhsa.target"):
                in_meta = False
            elif m and m.group(1) == ".name" and entry is not None:
                meta[m.group(2).strip("'\"")] = entry
            elif m and m.group(1) in FIELDS and entry is not None:
                entry[m.group(1)] = int(m.group(2))
            continue
        m = re.match(r"\.type\s+([^,\s]+),@function", line)
        if raw.startswith("amdhsa.kernels:"):
            in_meta = True
        elif m:
            functions.add(m.group(1))
        elif line.endswith(":") and line[:-1] in functions:
            cur = streams.setdefault(line[:-1], [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line and not line.startswith(".") and not line.endswith(":"):
            cur.append(LOCAL_LABEL.sub(lambda m: re.sub(r"[0-9_]+$", "", m.group(0)), line))
    return streams, {k: v for k, v in meta.items() if k in streams}


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    # (the parameter list of a kernel says nothing its template arguments do not)
    return {n: re.sub(r"\(.*$", "", re.sub(r"^void ", "", d.replace("(anonymous namespace)::", "")))
            for n, d in zip(names, out)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--only", default="", help="rows whose demangled name contains this")
    a = ap.parse_args()
    (sp, mp), (st, mt) = parse(a.parent), parse(a.this)
    names = sorted(set(sp) | set(st))
    nice = demangle(names)
    bad = lowered = 0
    same_k = diff_k = 0
    print("%-9s %7s %7s  %s  %s" % ("stream", "n_par", "n_this", " ".join("%7s" % s for s in SHORT), "symbol"))
    for is_kernel in (True, False):
        for n in sorted(names, key=lambda n: nice[n]):
            if ((n in mp or n in mt) != is_kernel) or a.only not in nice[n]:
                continue
            if n not in sp or n not in st:
                print("%-9s %7s %7s  %s  %s" % ("ONLY-" + ("PAR" if n in sp else "THIS"), len(sp.get(n, ())) or "-",
                                                 len(st.get(n, ())) or "-", " " * (8 * len(SHORT) - 1), nice[n]))
                bad += 1
                continue
            same = sp[n] == st[n]
            cols = []
            for f in FIELDS if is_kernel else ():
                p, t = mp[n].get(f), mt[n].get(f)
                cols.append("%7s" % (p if p == t else "%s>%s" % (p, t)))
                bad += (p is None) != (t is None) or (p is not None and t is not None and t > p)
                lowered += p is not None and t is not None and t < p
            if is_kernel:
                same_k += same
                diff_k += not same
            print("%-9s %7d %7d  %s  %s" % ("same" if same else "DIFFERENT", len(sp[n]), len(st[n]),
                                             " ".join(cols) if cols else " " * (8 * len(SHORT) - 1), nice[n]))
    print("kernels: %d identical streams, %d different; symbols missing or metadata fields raised: %d; fields lowered: %d"
          % (same_k, diff_k, bad, lowered))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
