#!/usr/bin/env python3
"""Generate tests/golden/peak_record.json: the reference's R-peak detectors (lib_rspt/peak_detector.h) and filter designer
(lib_rspt/lib_filter/iir_filter_design.cpp, create_filter_iir) on the inputs of tests/peak_cases.py, driven as the GPU stage
restates them (tests/golden/peak_shim.cpp).

The script compiles the headers, the designer and the shim (g++ -O2 -std=gnu++11) into a temporary directory outside the
repository, runs every case, writes the record and deletes the build.  Nothing under oracle/ is used.  The record holds
  designs  create_filter_iir over tests/peak_cases.py:design_grid(): the coefficient count (-1: refused) and the exact
           coefficients as little-endian float64 hex
  cases    per input x variant x sampling rate: the events (the samples at which detect() takes its marker branch) as counts
           per (block, channel) and indices, the values a marker of -1.0 returns at them (exact, hex), and digests of the
           detector's two traces (tests/peak_cases.py: tdigest); an event is a sample where the marker-1.0 run returns 1.0

    python tests/golden/make_peak_record.py [--ref DIR]     (DIR: the reference's root, default $REF or /root/reference,
                                                              as in oracle/Makefile)
"""
import ctypes as C

import numpy as np
import refrecord

refrecord.repo_paths()

import peak_cases as pc  # noqa: E402


def bind(L):
    P = C.c_void_p
    L.peak_shim_design.restype = C.c_int
    L.peak_shim_design.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, P, P]
    L.peak_shim_run.restype = None
    L.peak_shim_run.argtypes = [C.c_int, P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, P, P, P]


def run(L, c, marker):
    x = np.ascontiguousarray(pc.case_i32(c))
    ret, sig, thr = (np.zeros(x.shape) for _ in range(3))
    L.peak_shim_run(c["variant"], x.ctypes.data, c["nblocks"], c["nch"], c["ns"], c["fs"], marker, int(c["stateful"]), ret.ctypes.data,
                    sig.ctypes.data, thr.ctypes.data)
    return ret, sig, thr


def main():
    with refrecord.ref_library("peak", ["lib_rspt/lib_filter/iir_filter_design.cpp"], ["lib_rspt"]) as L:
        bind(L)
        out = {"generator": "tests/golden/make_peak_record.py (peak_detector.h, iir_filter_opt.h, filter.h, lib_filter/iir_filter_design.cpp + "
                            "tests/golden/peak_shim.cpp, g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of a [nblocks][ns][nch] float64 trace, NaNs made one (tests/peak_cases.py: tdigest)",
               "designs": [], "cases": []}
        for t, o, fs, lo, hi in pc.design_grid():
            num, den = np.zeros(5), np.zeros(5)
            n = L.peak_shim_design(t, o, fs, lo, hi, num.ctypes.data, den.ctypes.data)
            rec = {"type": t, "order": o, "fs": fs, "lo": lo, "hi": hi, "n": n}
            if n > 0:
                rec["num"], rec["den"] = num[:n].tobytes().hex(), den[:n].tobytes().hex()
            out["designs"].append(rec)
        for c in pc.peak_cases():
            r1, s1, h1 = run(L, c, 1.0)
            rm, sm, hm = run(L, c, -1.0)
            assert pc.tdigest(s1) == pc.tdigest(sm) and pc.tdigest(h1) == pc.tdigest(hm), c["name"]
            assert np.all((r1 == 0) | (r1 == 1.0)) and np.all((rm == 0) | (r1 == 1.0)), c["name"]  # (marker 1.0 marks every event)
            ev = r1 == 1.0
            count = ev.sum(axis=1).reshape(-1).tolist()  # [nblocks][nch]
            index, values = [], []
            for b in range(c["nblocks"]):
                for ch in range(c["nch"]):
                    i = np.nonzero(ev[b, :, ch])[0]
                    index += i.tolist()
                    values += rm[b, i, ch].tolist()
            rec = {"name": c["name"], "variant": c["variant"], "fs": c["fs"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"],
                   "nblocks": c["nblocks"], "stateful": c["stateful"], "in_crc32": pc.crc(c["data"]), "count": count, "index": index,
                   "values_m1": pc.vhex(values), "sig": pc.tdigest(s1), "thr": pc.tdigest(h1), "nan": bool(np.isnan(s1).any())}
            out["cases"].append(rec)
            print(c["name"], sum(count), "events", "(NaN traces)" if rec["nan"] else "", flush=True)
    refrecord.write_record("peak_record.json", out, per_line=("designs", "cases"))


if __name__ == "__main__":
    main()
