#!/usr/bin/env python3
"""Generate tests/golden/median_record.json: the reference's rolling_window_median<double> (lib_rspt/lib_stat/
rolling_window_median.h) on the inputs of tests/median_cases.py, one fresh object per channel (tests/golden/median_shim.cpp).

The script compiles the header and the shim (g++ -O2 -std=gnu++11) into a temporary directory outside the repository, runs
every case, writes the record and deletes the build.  Nothing under oracle/ is used.  The record holds per case the crc32 of
the input and the crc32 and digest (tests/cases.py) of the filtered block in the native width; the 64 ch x 65536 block only as
crc32s; and the doubles the reference returns on its own test's 20 inputs.

    python tests/golden/make_median_record.py [--ref DIR]     (DIR: the reference's root, default $REF or /root/reference,
                                                                as in oracle/Makefile)
"""
import ctypes as C

import numpy as np
import refrecord

refrecord.repo_paths()

import median_cases as mc  # noqa: E402
from cases import digest  # noqa: E402


def bind(L):
    L.median_shim_run.restype = None
    L.median_shim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t]
    L.median_shim_doubles.restype = None
    L.median_shim_doubles.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t]


def run(L, native, bps, nch, ns, W):
    x = np.ascontiguousarray(mc.native_to_i32(native, bps, nch, ns))
    y = np.zeros_like(x)
    L.median_shim_run(x.ctypes.data, y.ctypes.data, nch, ns, W)
    return mc.i32_to_native(y, bps)


def main():
    with refrecord.ref_library("median", [], ["lib_rspt/lib_stat"]) as L:
        bind(L)
        out = {"generator": "tests/golden/make_median_record.py (lib_stat/rolling_window_median.h + tests/golden/median_shim.cpp, g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of the filtered native bytes (tests/cases.py: digest)",
               "ref20": {}, "cases": []}
        x = np.ascontiguousarray(mc.REF20, dtype=np.float64)
        for W in sorted(mc.REF20_EXPECTED):
            y = np.zeros_like(x)
            L.median_shim_doubles(x.ctypes.data, y.ctypes.data, x.size, W)
            out["ref20"][str(W)] = [float(v) for v in y]
        for c in mc.median_cases():
            y = run(L, c["data"], c["bps"], c["nch"], c["ns"], c["W"])
            rec = {"name": c["name"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "W": c["W"], "in_crc32": mc.crc(c["data"]),
                   "crc32": mc.crc(y), "digest": digest(y)}
            out["cases"].append(rec)
            print(c["name"], rec["digest"], flush=True)
        B = mc.BIG
        d = mc.big_data()
        big = {"name": B["name"], "bps": B["bps"], "nch": B["nch"], "ns": B["ns"], "block": B["block"], "in_crc32": mc.crc(d), "crc32": {}}
        for W in B["windows"]:
            big["crc32"][str(W)] = mc.crc(run(L, d, B["bps"], B["nch"], B["ns"], W))
        out["big"] = big
        print(B["name"], big["crc32"])
    refrecord.write_record("median_record.json", out)


if __name__ == "__main__":
    main()
