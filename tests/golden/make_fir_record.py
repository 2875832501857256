#!/usr/bin/env python3
"""Generate tests/golden/fir_record.json: the reference's FIR filter (lib_rspt/lib_filter/fir_filter.cpp) on the inputs of
tests/fir_cases.py, driven as its test harness drives a filter (tests/golden/fir_shim.cpp).

The script compiles fir_filter.cpp and the shim with the oracle's reference flags (g++ -O2 -std=gnu++11, plain x86-64: no
fused multiply-add) into a temporary directory outside the repository, runs every case with one filter object shared by the
channels and with one object per channel, writes the record and deletes the build.  Nothing under oracle/ is used or
changed.  The record holds per case the coefficients exactly (float.hex, or one hex digit per tap for the long random
kernels: tests/fir_cases.py kernel_to_record), the crc32 of the input, and per driving the crc32
and digest (tests/cases.py) of the filtered block in the native width; the 64 ch x 65536 block only as crc32s.

    python tests/golden/make_fir_record.py [--ref DIR]     (DIR: the reference's root, default $REF or /root/reference,
                                                             as in oracle/Makefile)
"""
import ctypes as C

import numpy as np
import refrecord

refrecord.repo_paths()

import fir_cases as fc  # noqa: E402
from cases import digest  # noqa: E402


def bind(L):
    L.fir_shim_run.restype = None
    L.fir_shim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int]


def run(L, native, bps, nch, ns, kernel, shared):
    x = np.ascontiguousarray(fc.native_to_i32(native, bps, nch, ns))
    y = np.zeros_like(x)
    k = np.ascontiguousarray(kernel, dtype=np.float64)
    L.fir_shim_run(x.ctypes.data, y.ctypes.data, nch, ns, k.ctypes.data, k.size, int(shared))
    return fc.i32_to_native(y, bps)


def main():
    with refrecord.ref_library("fir", ["lib_rspt/lib_filter/fir_filter.cpp"], ["lib_rspt"]) as L:
        bind(L)
        out = {"generator": "tests/golden/make_fir_record.py (lib_filter/fir_filter.cpp + tests/golden/fir_shim.cpp, g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of the filtered native bytes (tests/cases.py: digest)",
               "cases": []}
        for c in fc.fir_cases():
            rec = {"name": c["name"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "kernel": fc.kernel_to_record(c["kernel"]),
                   "in_crc32": fc.crc(c["data"])}
            for mode, shared in (("shared", True), ("per_channel", False)):
                y = run(L, c["data"], c["bps"], c["nch"], c["ns"], c["kernel"], shared)
                rec[mode] = {"crc32": fc.crc(y), "digest": digest(y)}
            out["cases"].append(rec)
            print(c["name"], rec["shared"]["digest"], rec["shared"] == rec["per_channel"], flush=True)
        B = fc.BIG
        d, k = fc.big_data(), fc.big_kernel()
        big = dict(B, kernel=fc.kernel_to_record(k), in_crc32=fc.crc(d))
        for mode, shared in (("shared", True), ("per_channel", False)):
            big[mode] = {"crc32": fc.crc(run(L, d, B["bps"], B["nch"], B["ns"], k, shared))}
        out["big"] = big
        print(B["name"], big["shared"], big["per_channel"])
    refrecord.write_record("fir_record.json", out)


if __name__ == "__main__":
    main()
