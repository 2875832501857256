#!/usr/bin/env python3
"""Generate tests/golden/iir_zero_phase_planar_record.json: the reference's IIR filter (lib_rspt/lib_filter/iir_filter.cpp) run
forward and then, the same object, backward over its own untruncated output on the int32 matrices of
tests/iir_zero_phase_planar_cases.py (recorded_cases: the seeded shape sweep, and values outside a narrower handle's sample
width), one fresh object per row -- what tests/golden/iir_zero_phase_record.json, whose inputs are native samples of the case's
width, cannot express.

The shim is the native record's (tests/golden/iir_zero_phase_shim.cpp): it filters int32 values, so a matrix goes through it as
the int32 block that interleaves its rows, at bps = 4 whatever the case's handle.  Compiled with the oracle's reference flags
(g++ -O2 -std=gnu++11, plain x86-64: no fused multiply-add) into a temporary directory outside the repository, which is deleted
afterwards.  Nothing under oracle/ is used or changed.  The record holds per case the name, the shape, the coefficients exactly
(iir_cases.to_bits), both history lengths, the crc32 of the input and the crc32 and digest (tests/cases.py) of the answer, both
as the int32 values of the matrix [nblocks][nch][ns] in memory order, little-endian.

    python tests/golden/make_iir_zero_phase_planar_record.py [--ref DIR]     (DIR: the reference's root, default $REF or
                                                                               /root/reference, as in oracle/Makefile)
"""
import numpy as np
import refrecord

refrecord.repo_paths()

import iir_zero_phase_planar_cases as zp  # noqa: E402
from cases import digest  # noqa: E402
from make_iir_zero_phase_record import bind  # noqa: E402


def matrix_bytes(P):
    return np.ascontiguousarray(P, dtype="<i4").view(np.uint8).reshape(-1)


def run(L, c):
    """the reference's answer as a matrix [nblocks][nch][ns]"""
    x = np.ascontiguousarray(zp.rows_of(c["planar"]), dtype=np.int32)
    y = np.zeros_like(x)
    n, d = np.array(c["n"], dtype=np.float64), np.array(c["d"], dtype=np.float64)
    L.iir_zero_phase_shim_run(x.ctypes.data, y.ctypes.data, c["nch"], c["ns"], c["nblocks"], n.ctypes.data, d.ctypes.data, n.size, c["init"], c["binit"])
    return zp.planar_of(y, c["nblocks"], c["nch"], c["ns"])


def main():
    with refrecord.ref_library("iir_zero_phase", ["lib_rspt/lib_filter/iir_filter.cpp"], ["lib_rspt"]) as L:
        bind(L)
        out = {"generator": "tests/golden/make_iir_zero_phase_planar_record.py (lib_filter/iir_filter.cpp + tests/golden/iir_zero_phase_shim.cpp, "
                            "g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of the filtered matrix [nblocks][nch][ns], int32 little-endian (tests/cases.py: digest)",
               "cases": []}
        for c in zp.recorded_cases():
            y = matrix_bytes(run(L, c))
            rec = {"name": c["name"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "nblocks": c["nblocks"]}
            rec.update(zp.to_record(c))
            rec.update({"in_crc32": zp.crc(matrix_bytes(c["planar"])), "crc32": zp.crc(y), "digest": digest(y)})
            out["cases"].append(rec)
            print(c["name"], rec["digest"], flush=True)
    refrecord.write_record("iir_zero_phase_planar_record.json", out)


if __name__ == "__main__":
    main()
