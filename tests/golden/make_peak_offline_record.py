#!/usr/bin/env python3
"""Generate tests/golden/peak_offline_record.json: the reference's zero-phase offline R-peak detector
(peak_detector_offline::detect, lib_rspt/peak_detector.h) on the inputs of tests/peak_offline_cases.py, driven as the GPU stage
restates it (tests/golden/peak_offline_shim.cpp).

The script compiles the headers, the designer and the shim (g++ -O2 -std=gnu++11) into a temporary directory outside the
repository, runs every case, writes the record and deletes the build.  Nothing under oracle/ is used.  Per input x sampling
rate the record holds, for marker 1.0 and for marker -1.0, the events (the non-zero entries of the final peak_signal; for a
detect_fw block of the alternating chain, the samples at which it takes its marker branch) as counts per (block, channel),
indices and exact values (little-endian float64 hex), digests of filt_signal and threshold_signal (tests/peak_cases.py:
tdigest), and the revisits and collisions of the relocation as the restatement (tests/peak_offline_cases.py) counts them
(collisions_ahead: those onto a live peak ahead of the one being moved, not yet visited).

    python tests/golden/make_peak_offline_record.py [--ref DIR]     (DIR: the reference's root, default $REF or /root/reference,
                                                                      as in oracle/Makefile)
"""
import ctypes as C

import numpy as np
import refrecord

refrecord.repo_paths()

import peak_cases as pc  # noqa: E402
import peak_offline_cases as oc  # noqa: E402


def bind(L):
    P = C.c_void_p
    L.peak_offline_shim_run.restype = None
    L.peak_offline_shim_run.argtypes = [P, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, P, P, P, P]


def run(L, c, marker):
    x = np.ascontiguousarray(oc.case_i32(c))
    ret, sig, thr = (np.zeros(x.shape) for _ in range(3))
    calls = None
    if c["calls"] is not None:
        calls = np.array([1 if k == "fw" else 0 for k in c["calls"]], dtype=np.int32)
    L.peak_offline_shim_run(x.ctypes.data, c["nblocks"], c["nch"], c["ns"], c["fs"], marker, int(c["stateful"]),
                            calls.ctypes.data if calls is not None else None, ret.ctypes.data, sig.ctypes.data, thr.ctypes.data)
    return ret, sig, thr


def events(c, ret, sig, marker):
    """per (block, channel): the non-zero peak_signal, or for a detect_fw block the marker branch (where ret is the marker
    value, bitwise: marker -1.0 writes filt_signal)"""
    ev = ret != 0
    if c["calls"] is not None:
        for b, k in enumerate(c["calls"]):
            if k == "fw":
                want = sig[b] if marker == -1.0 else np.full_like(sig[b], marker)
                ev[b] = (ret[b] == want) & (want != 0)
    count, index, values = [], [], []
    for b in range(c["nblocks"]):
        for ch in range(c["nch"]):
            i = np.nonzero(ev[b, :, ch])[0]
            count.append(int(i.size))
            index += i.tolist()
            values += ret[b, i, ch].tolist()
    return count, index, values


def main():
    with refrecord.ref_library("peak_offline", ["lib_rspt/lib_filter/iir_filter_design.cpp"], ["lib_rspt"]) as L:
        bind(L)
        out = {"generator": "tests/golden/make_peak_offline_record.py (peak_detector.h, iir_filter_opt.h, filter.h, lib_filter/iir_filter_design.cpp + "
                            "tests/golden/peak_offline_shim.cpp, g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of a [nblocks][ns][nch] float64 trace, NaNs made one (tests/peak_cases.py: tdigest)",
               "cases": []}
        for c in oc.offline_cases():
            r1, s1, h1 = run(L, c, 1.0)
            rm, sm, hm = run(L, c, -1.0)
            assert pc.tdigest(s1) == pc.tdigest(sm) and pc.tdigest(h1) == pc.tdigest(hm), c["name"]
            count, index, values = events(c, r1, s1, 1.0)
            assert all(v == 1.0 for v in values), c["name"]
            count_m1, index_m1, values_m1 = events(c, rm, sm, -1.0)
            st = {}
            oc.detect(oc.case_i32(c), c["fs"], 1.0, c["stateful"], c["calls"], st)
            rec = {"name": c["name"], "fs": c["fs"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "nblocks": c["nblocks"],
                   "stateful": c["stateful"], "calls": c["calls"], "in_crc32": pc.crc(c["data"]), "count": count, "index": index,
                   "count_m1": count_m1, "index_m1": index_m1, "values_m1": pc.vhex(values_m1), "sig": pc.tdigest(s1), "thr": pc.tdigest(h1),
                   "revisit_moves": st["revisit_moves"], "collisions": st["collisions"], "collisions_ahead": st["collisions_ahead"]}
            out["cases"].append(rec)
            print(c["name"], sum(count), "events", st, flush=True)
    refrecord.write_record("peak_offline_record.json", out)


if __name__ == "__main__":
    main()
