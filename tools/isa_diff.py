#!/usr/bin/env python3
"""Compare the device functions of two builds of rspt_hip.hip, instruction for instruction.

A kernel here is sometimes kept exactly what was timed (filter.hip, iir_cascade.hip: the bodies included into a native kernel and
its planar form), and "the native instantiations did not move" is then a claim about the compiler's output.  This tool makes it
repeatable: it compiles the device assembly of two source trees as tests/devasm.py does (or takes two .s files), normalises what
differs without meaning -- comments, directives, the numbers of local labels and of unnamed strings -- and lists every function
whose lines differ, with the first differing lines.

    python tools/isa_diff.py <tree or .s of the older build> [<tree or .s of this build, default: this tree>] [--only REGEX]

Exit status 1 if a function present in both differs (functions only one side has are listed, and do not count).
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def assembly(where, tmp):
    """the device assembly of a tree (compiled into tmp), or the .s file itself"""
    if os.path.isfile(where):
        return where
    out = os.path.join(tmp, "%s.s" % abs(hash(os.path.abspath(where))))
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value", "-w",
                           "-I" + os.path.join(where, "include"), "-o", out, os.path.join(where, "rspt_amd", "csrc", "rspt_hip.hip")])
    return out


def functions(path):
    """mangled name -> its normalised lines"""
    funcs, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = funcs[m.group(1)] = []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            line = line.split(";")[0].rstrip()
            if not line.strip() or (line.lstrip().startswith(".") and not re.match(r"^\.LBB", line)):
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            cur.append(re.sub(r"\.L__unnamed_\d+|\.L?\.?str\.\d+", ".Lstr", line))
    return funcs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new", nargs="?", default=ROOT)
    ap.add_argument("--only", default=None, help="compare only the functions whose mangled name matches")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="rspt_isa_") as tmp:
        A, B = functions(assembly(a.old, tmp)), functions(assembly(a.new, tmp))
    keep = (lambda n: re.search(a.only, n)) if a.only else (lambda n: True)
    both = [n for n in A if n in B and keep(n)]
    differ = [n for n in both if A[n] != B[n]]
    for n in differ:
        d = [x for x in difflib.unified_diff(A[n], B[n], lineterm="", n=0) if x[:1] in "+-" and not x.startswith(("+++", "---"))]
        print("DIFFERENT %s: %d -> %d lines, %d changed" % (n, len(A[n]), len(B[n]), len(d)))
        print("\n".join(d[:8]))
    for tag, X, Y in (("only in the older build", A, B), ("only in the newer build", B, A)):
        names = [n for n in X if n not in Y and keep(n)]
        if names:
            print("%s: %d functions" % (tag, len(names)))
            for n in names:
                print("   ", n)
    print("%d functions in both, %d identical, %d different" % (len(both), len(both) - len(differ), len(differ)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
