"""What the make_*_record.py generators share: where the repository and the reference are, compiling reference sources with a
shim into a library that lives for one run, and writing a record one entry per line.

A generator keeps what is its own: which reference sources, the shim's argtypes, how a case is run and what its record holds.
Nothing of the reference is read here but the paths a generator names under its root.
"""
import argparse
import contextlib
import ctypes
import glob
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

CXX = ["g++", "-O2", "-std=gnu++11", "-w", "-fPIC"]  # the oracle's reference flags: plain x86-64, no fused multiply-add
CC = ["gcc", "-O2", "-std=c11", "-DNDEBUG", "-fPIC"]

# ref_library's arguments for a shim that drives the packers: the whole library
PACKERS = dict(sources=["lib_rspt/lib_signalpacker/*.cpp", "lib_rspt/lib_zaxtensor/*.cpp", "lib_rspt/lib_filter/*.cpp"], include_dirs=[""],
               c_sources=["lib_rspt/lib_hzr/*.c", "lib_rspt/lib_fwht/fwht.c"])


def repo_paths():
    """the repository root and tests/ on sys.path: the case modules and the oracle import as they do under pytest"""
    for p in (os.path.join(ROOT, "tests"), ROOT):
        if p not in sys.path:
            sys.path.insert(0, p)


def ref_root():
    """the reference's root: --ref DIR, default $REF or /root/reference, as in oracle/Makefile"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    return ap.parse_args().ref


@contextlib.contextmanager
def ref_library(name, sources, include_dirs, c_sources=()):
    """lib<name>_ref.so of tests/golden/<name>_shim.cpp and the reference's sources (paths under its root; a * is expanded),
    compiled in a fresh temporary directory outside the repository and loaded; the directory goes when the block ends.
    -> the ctypes.CDLL, its build directory as .tmp"""
    ref = ref_root()

    def under_ref(paths):
        out = []
        for p in paths:
            p = os.path.join(ref, p)
            out += sorted(glob.glob(p)) if "*" in p else [p]
        return out

    tmp = tempfile.mkdtemp(prefix=name + "_ref_")
    try:
        objs = []
        for f in under_ref(c_sources):
            objs.append(os.path.join(tmp, os.path.basename(f) + ".o"))
            subprocess.check_call(CC + ["-c", f, "-o", objs[-1]])
        lib = os.path.join(tmp, "lib%s_ref.so" % name)
        subprocess.check_call(CXX + ["-shared"] + ["-I" + d for d in under_ref(include_dirs)] + ["-o", lib] + under_ref(sources)
                              + [os.path.join(HERE, name + "_shim.cpp")] + objs)
        L = ctypes.CDLL(lib)
        L.tmp = tmp
        yield L
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def write_record(path, out, per_line=("cases",)):
    """the record `out` as JSON into path (relative: beside the generators), the entries of its per_line keys one per line"""
    repo_paths()
    from casetools import record_text

    with open(os.path.join(HERE, path), "w") as f:
        f.write(record_text(out, per_line))
