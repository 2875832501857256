#!/usr/bin/env python3
"""Generate tests/golden/stream_filter_record.json: the reference's IIR and FIR filters (lib_rspt/lib_filter/iir_filter.cpp,
fir_filter.cpp) on the recordings of tests/stream_filter_cases.py, one object per channel living on from block to block
(tests/golden/stream_filter_shim.cpp).

The script compiles the two reference sources and the shim with the oracle's reference flags (g++ -O2 -std=gnu++11, plain
x86-64: no fused multiply-add) into a temporary directory outside the repository, runs every case, writes the record and
deletes the build.  Nothing under oracle/ is used or changed.  The record holds per case the coefficients exactly
(iir_cases.to_bits / fir_cases.kernel_to_record), the crc32 of the input, and the crc32 and digest (tests/cases.py) of the
filtered recording in the native width.

    python tests/golden/make_stream_filter_record.py [--ref DIR]     (DIR: the reference's root, default $REF or /root/reference,
                                                                       as in oracle/Makefile)
"""
import ctypes as C

import numpy as np
import refrecord

refrecord.repo_paths()

import fir_cases as fc  # noqa: E402
import stream_filter_cases as sc  # noqa: E402
from cases import digest  # noqa: E402


def bind(L):
    L.stream_filter_shim_run.restype = None
    L.stream_filter_shim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]


def run(L, c):
    rows = c["ns"] * c["nblocks"]
    x = np.ascontiguousarray(fc.native_to_i32(c["data"], c["bps"], c["nch"], rows))
    y = np.zeros_like(x)
    if c["kind"] == "fir":
        a = np.ascontiguousarray(c["kernel"], dtype=np.float64)
        L.stream_filter_shim_run(x.ctypes.data, y.ctypes.data, c["nch"], c["ns"], c["nblocks"], 1, a.ctypes.data, None, a.size, 0)
    else:
        a, b = np.ascontiguousarray(c["n"], dtype=np.float64), np.ascontiguousarray(c["d"], dtype=np.float64)
        L.stream_filter_shim_run(x.ctypes.data, y.ctypes.data, c["nch"], c["ns"], c["nblocks"], 0, a.ctypes.data, b.ctypes.data, a.size, c["init"])
    return fc.i32_to_native(y, c["bps"])


def main():
    with refrecord.ref_library("stream_filter", ["lib_rspt/lib_filter/iir_filter.cpp", "lib_rspt/lib_filter/fir_filter.cpp"], ["lib_rspt"]) as L:
        bind(L)
        out = {"generator": "tests/golden/make_stream_filter_record.py (lib_filter/iir_filter.cpp, fir_filter.cpp + "
                            "tests/golden/stream_filter_shim.cpp, g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of the filtered native bytes (tests/cases.py: digest)",
               "cases": []}
        for c in sc.stream_cases():
            rec = {"name": c["name"], "kind": c["kind"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "nblocks": c["nblocks"]}
            rec.update(sc.coef_to_record(c))
            y = run(L, c)
            rec.update({"in_crc32": fc.crc(c["data"]), "crc32": fc.crc(y), "digest": digest(y)})
            out["cases"].append(rec)
            print(c["name"], rec["digest"], flush=True)
    refrecord.write_record("stream_filter_record.json", out)


if __name__ == "__main__":
    main()
