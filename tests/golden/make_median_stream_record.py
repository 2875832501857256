#!/usr/bin/env python3
"""Generate tests/golden/median_stream_record.json: the reference's rolling_window_median<double> (lib_rspt/lib_stat/
rolling_window_median.h) on the recordings of tests/median_stream_cases.py, one object per channel living across the blocks
(tests/golden/median_stream_shim.cpp).

The script compiles the header and the shim (g++ -O2 -std=gnu++11) into a temporary directory outside the repository, runs
every case, writes the record and deletes the build.  Nothing under oracle/ is used.  The record holds per case the shape, W,
the crc32 of the input and the crc32 and digest (tests/cases.py) of the filtered recording in the native width; no sample data.

    python tests/golden/make_median_stream_record.py [--ref DIR]     (DIR: the reference's root, default $REF or
                                                                       /root/reference, as in oracle/Makefile)
"""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import median_stream_cases as msc  # noqa: E402
from cases import digest  # noqa: E402


def build(ref, tmp):
    lib = os.path.join(tmp, "libmedian_stream_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=gnu++11", "-w", "-fPIC", "-shared", "-I" + os.path.join(ref, "lib_rspt", "lib_stat"), "-o", lib,
                           os.path.join(HERE, "median_stream_shim.cpp")])
    L = C.CDLL(lib)
    L.median_stream_shim_run.restype = None
    L.median_stream_shim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("REF", "/root/reference"))
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="median_stream_ref_")
    rec = []
    try:
        L = build(a.ref, tmp)
        for c in msc.stream_cases():
            x = np.ascontiguousarray(msc.native_to_i32(c["data"], c["bps"], c["nch"], c["ns"] * c["nblocks"]))
            y = np.zeros_like(x)
            L.median_stream_shim_run(x.ctypes.data, y.ctypes.data, c["nch"], c["ns"], c["nblocks"], c["W"])
            y = msc.i32_to_native(y, c["bps"])
            rec.append({"name": c["name"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "nblocks": c["nblocks"], "W": c["W"],
                        "in_crc32": msc.crc(c["data"]), "crc32": msc.crc(y), "digest": digest(y)})
            print(c["name"], rec[-1]["digest"], flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(HERE, "median_stream_record.json"), "w") as f:  # (one case per line)
        f.write("{\n")
        f.write('"generator": ' + json.dumps("tests/golden/make_median_stream_record.py (lib_stat/rolling_window_median.h + "
                                             "tests/golden/median_stream_shim.cpp, g++ -O2 -std=gnu++11)") + ",\n")
        f.write('"digest": ' + json.dumps("first 32 hex digits of the sha256 of the filtered native bytes (tests/cases.py: digest)") + ",\n")
        f.write('"cases": [\n' + ",\n".join(json.dumps(c) for c in rec) + "\n]\n}\n")


if __name__ == "__main__":
    main()
