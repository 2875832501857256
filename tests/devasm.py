"""The device assembly of rspt_hip.hip for gfx950 (hipcc -S), for the tests and tools that read the kernels' ISA.  The tests take
it through tests/devframe.py: its `asm` fixture, and the checks that several modules make of it (rounds_separately, uses_no_scratch).

Compiled once per process (the unity build takes over a minute on one core) and removed when the process ends."""
import atexit
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

_cache = {}


def asm_path():
    """the path of the device assembly, compiled on the first call"""
    if "path" not in _cache:
        tmp = tempfile.mkdtemp(prefix="rspt_asm_")
        atexit.register(shutil.rmtree, tmp, True)
        path = os.path.join(tmp, "rspt.s")
        subprocess.check_call(
            [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-Wno-unused-value", "-w",
             "-I" + os.path.join(ROOT, "include"), "-o", path, os.path.join(ROOT, "rspt_amd", "csrc", "rspt_hip.hip")]
        )
        _cache["path"] = path
    return _cache["path"]


def functions():
    """mangled name -> the function's lines as written (from the line after its label up to its .Lfunc_end)"""
    if "funcs" not in _cache:
        funcs, cur = {}, None
        for line in open(asm_path()):
            m = re.match(r"^(_Z\w+):", line)
            if m:
                cur = funcs[m.group(1)] = []
            elif cur is not None:
                if line.startswith(".Lfunc_end"):
                    cur = None
                else:
                    cur.append(line)
        _cache["funcs"] = funcs
    return _cache["funcs"]


def innermost_loops(body):
    """instruction counts of the innermost loops of one function's lines, in program order: a loop is a label up to a branch
    back to it, innermost when no other such branch lies inside"""
    labels, edges = {}, []  # back edges: (label line, branch line)
    for i, ln in enumerate(body):
        lm = re.match(r"^(\.LBB\w+):", ln)
        if lm:
            labels[lm.group(1)] = i
        bm = re.match(r"^\s+s_(?:cbranch_\w+|branch)\s+(\.LBB\w+)", ln)
        if bm and bm.group(1) in labels:
            edges.append((labels[bm.group(1)], i))
    loops = []
    for lo, hi in sorted(edges):
        if not any(lo <= l2 and h2 <= hi and (l2, h2) != (lo, hi) for l2, h2 in edges):
            loops.append(sum(1 for s in body[lo : hi + 1] if re.match(r"^\s+[sv]_|^\s+(global|buffer|flat|ds|scratch)_", s)))
    return loops
