#!/usr/bin/env python3
"""Generate tests/golden/iir_cascade_record.json: the reference's IIR filters (lib_rspt/lib_filter/iir_filter.cpp) chained per
sample on the recordings of tests/iir_cascade_cases.py, one chain of objects per channel (tests/golden/iir_cascade_shim.cpp),
carried from block to block (`stream`) and fresh for every block (`stateless`).

The script compiles the reference source and the shim with the oracle's reference flags (g++ -O2 -std=gnu++11, plain x86-64:
no fused multiply-add) into a temporary directory outside the repository, runs every case, writes the record and deletes the
build.  Nothing under oracle/ is used or changed.  The record holds per case the name, the shape, every section's coefficients
exactly (iir_cases.to_bits), init and mode, the crc32 of the input, and the crc32 and digest (tests/cases.py) of both answers
in the native width.

    python tests/golden/make_iir_cascade_record.py [--ref DIR]     (DIR: the reference's root, default $REF or /root/reference,
                                                                     as in oracle/Makefile)
"""
import ctypes as C

import numpy as np
import refrecord

refrecord.repo_paths()

import fir_cases as fc  # noqa: E402
import iir_cascade_cases as cc  # noqa: E402
from cases import digest  # noqa: E402


def bind(L):
    L.iir_cascade_shim_run.restype = None
    L.iir_cascade_shim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int]


def run(L, c, carry):
    rows = c["ns"] * c["nblocks"]
    x = np.ascontiguousarray(fc.native_to_i32(c["data"], c["bps"], c["nch"], rows))
    y = np.zeros_like(x)
    S = len(c["sections"])
    n, d = np.zeros((S, 5)), np.zeros((S, 5))
    nc, init, filt = np.zeros(S, dtype=np.uint32), np.zeros(S, dtype=np.int32), np.zeros(S, dtype=np.uint8)
    for k, (sn, sd, si, sf) in enumerate(c["sections"]):
        n[k, : len(sn)], d[k, : len(sd)] = sn, sd
        nc[k], init[k], filt[k] = len(sn), si, sf
    L.iir_cascade_shim_run(x.ctypes.data, y.ctypes.data, c["nch"], c["ns"], c["nblocks"], S, n.ctypes.data, d.ctypes.data, nc.ctypes.data,
                           init.ctypes.data, filt.ctypes.data, carry)
    return fc.i32_to_native(y, c["bps"])


def main():
    with refrecord.ref_library("iir_cascade", ["lib_rspt/lib_filter/iir_filter.cpp"], ["lib_rspt"]) as L:
        bind(L)
        out = {"generator": "tests/golden/make_iir_cascade_record.py (lib_filter/iir_filter.cpp + tests/golden/iir_cascade_shim.cpp, "
                            "g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of the filtered native bytes (tests/cases.py: digest)",
               "cases": []}
        for c in cc.cascade_cases():
            rec = {"name": c["name"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "nblocks": c["nblocks"],
                   "sections": cc.sections_to_record(c), "in_crc32": fc.crc(c["data"])}
            for form, carry in (("stateless", 0), ("stream", 1)):
                y = run(L, c, carry)
                rec[form] = {"crc32": fc.crc(y), "digest": digest(y)}
            out["cases"].append(rec)
            print(c["name"], rec["stateless"]["digest"], rec["stream"]["digest"], flush=True)
    refrecord.write_record("iir_cascade_record.json", out)


if __name__ == "__main__":
    main()
