#!/usr/bin/env python3
"""Generate tests/golden/iir_zero_phase_record.json: the reference's IIR filter (lib_rspt/lib_filter/iir_filter.cpp) run forward
and then, the same object, backward over its own untruncated output on the blocks of tests/iir_zero_phase_cases.py, one fresh
object per (block, channel) (tests/golden/iir_zero_phase_shim.cpp).

The script compiles the reference source and the shim with the oracle's reference flags (g++ -O2 -std=gnu++11, plain x86-64:
no fused multiply-add) into a temporary directory outside the repository, runs every case, writes the record and deletes the
build.  Nothing under oracle/ is used or changed.  The record holds per case the name, the shape, the coefficients exactly
(iir_cases.to_bits), both history lengths, the crc32 of the input, and the crc32 and digest (tests/cases.py) of the answer in
the native width.

    python tests/golden/make_iir_zero_phase_record.py [--ref DIR]     (DIR: the reference's root, default $REF or /root/reference,
                                                                        as in oracle/Makefile)
"""
import ctypes as C

import numpy as np
import refrecord

refrecord.repo_paths()

import fir_cases as fc  # noqa: E402
import iir_zero_phase_cases as zc  # noqa: E402
from cases import digest  # noqa: E402


def bind(L):
    L.iir_zero_phase_shim_run.restype = None
    L.iir_zero_phase_shim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]


def run(L, c):
    rows = c["ns"] * c["nblocks"]
    x = np.ascontiguousarray(fc.native_to_i32(c["data"], c["bps"], c["nch"], rows))
    y = np.zeros_like(x)
    n, d = np.array(c["n"], dtype=np.float64), np.array(c["d"], dtype=np.float64)
    L.iir_zero_phase_shim_run(x.ctypes.data, y.ctypes.data, c["nch"], c["ns"], c["nblocks"], n.ctypes.data, d.ctypes.data, n.size, c["init"], c["binit"])
    return fc.i32_to_native(y, c["bps"])


def main():
    with refrecord.ref_library("iir_zero_phase", ["lib_rspt/lib_filter/iir_filter.cpp"], ["lib_rspt"]) as L:
        bind(L)
        out = {"generator": "tests/golden/make_iir_zero_phase_record.py (lib_filter/iir_filter.cpp + tests/golden/iir_zero_phase_shim.cpp, "
                            "g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of the filtered native bytes (tests/cases.py: digest)",
               "cases": []}
        for c in zc.zero_phase_cases():
            y = run(L, c)
            rec = {"name": c["name"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "nblocks": c["nblocks"]}
            rec.update(zc.to_record(c))
            rec.update({"in_crc32": fc.crc(c["data"]), "crc32": fc.crc(y), "digest": digest(y)})
            out["cases"].append(rec)
            print(c["name"], rec["digest"], flush=True)
    refrecord.write_record("iir_zero_phase_record.json", out)


if __name__ == "__main__":
    main()
