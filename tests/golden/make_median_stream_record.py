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
import ctypes as C

import numpy as np
import refrecord

refrecord.repo_paths()

import median_stream_cases as msc  # noqa: E402
from cases import digest  # noqa: E402


def bind(L):
    L.median_stream_shim_run.restype = None
    L.median_stream_shim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_size_t]


def main():
    with refrecord.ref_library("median_stream", [], ["lib_rspt/lib_stat"]) as L:
        bind(L)
        out = {"generator": "tests/golden/make_median_stream_record.py (lib_stat/rolling_window_median.h + "
                            "tests/golden/median_stream_shim.cpp, g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of the filtered native bytes (tests/cases.py: digest)",
               "cases": []}
        for c in msc.stream_cases():
            x = np.ascontiguousarray(msc.native_to_i32(c["data"], c["bps"], c["nch"], c["ns"] * c["nblocks"]))
            y = np.zeros_like(x)
            L.median_stream_shim_run(x.ctypes.data, y.ctypes.data, c["nch"], c["ns"], c["nblocks"], c["W"])
            y = msc.i32_to_native(y, c["bps"])
            out["cases"].append({"name": c["name"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "nblocks": c["nblocks"], "W": c["W"],
                                 "in_crc32": msc.crc(c["data"]), "crc32": msc.crc(y), "digest": digest(y)})
            print(c["name"], out["cases"][-1]["digest"], flush=True)
    refrecord.write_record("median_stream_record.json", out)


if __name__ == "__main__":
    main()
