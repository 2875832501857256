#!/usr/bin/env python3
"""Generate tests/golden/peak_planar_record.json: the reference's R-peak detectors (lib_rspt/peak_detector.h: the three online
detectors and peak_detector_offline::detect) on the int32 matrices of tests/peak_planar_cases.py (recorded_cases: row lengths,
row counts, carried state, events, moved peaks, and values outside a narrower handle's sample width -- what the native records,
whose inputs are native samples of the case's width, cannot express).

The shims are the native records' (tests/golden/peak_shim.cpp, peak_offline_shim.cpp): they take int32 blocks [nblocks][ns][nch]
and hand (double) of every value to detect(), so a matrix goes through them transposed, whatever the case's handle.  Compiled
with the oracle's reference flags (g++ -O2 -std=gnu++11) into temporary directories outside the repository, which are deleted
afterwards.  Nothing under oracle/ is used or changed.  Per case the record holds the name, the shape, the crc32 of the matrix
(int32 little-endian, memory order) and, as the native records do, the events of a marker 1.0 run (counts per row, indices), the
events (null where they are the marker 1.0 run's) and exact values (little-endian float64 hex) of a marker -1.0 run, and the digests of both traces taken on the
transposed trace [nblocks][ns][nch] (tests/peak_cases.py: tdigest).  No trace is stored.

    python tests/golden/make_peak_planar_record.py [--ref DIR]     (DIR: the reference's root, default $REF or /root/reference,
                                                                     as in oracle/Makefile)
"""
import numpy as np
import refrecord

refrecord.repo_paths()

import make_peak_offline_record as mo  # noqa: E402
import make_peak_record as mp  # noqa: E402
import peak_cases as pc  # noqa: E402
import peak_planar_cases as pp  # noqa: E402


def run(Lon, Loff, c, marker):
    """(ret, sig, thr) [nblocks][ns][nch] of the reference on the transposed matrix"""
    x = np.ascontiguousarray(pp.rows_of(c["planar"]), dtype=np.int32)
    ret, sig, thr = (np.zeros(x.shape) for _ in range(3))
    if c["kind"] == "online":
        Lon.peak_shim_run(c["variant"], x.ctypes.data, c["nblocks"], c["nch"], c["ns"], c["fs"], marker, int(c["stateful"]), ret.ctypes.data,
                          sig.ctypes.data, thr.ctypes.data)
    else:
        calls = None
        if c["calls"] is not None:
            calls = np.array([1 if k == "fw" else 0 for k in c["calls"]], dtype=np.int32)
        Loff.peak_offline_shim_run(x.ctypes.data, c["nblocks"], c["nch"], c["ns"], c["fs"], marker, int(c["stateful"]),
                                   calls.ctypes.data if calls is not None else None, ret.ctypes.data, sig.ctypes.data, thr.ctypes.data)
    return ret, sig, thr


def events(c, r1, rm, sm, marker):
    """counts, indices and values per row.  Online: an event is a sample where the marker 1.0 run returns 1.0 (a marker -1.0 run
    returns s there, which may be 0).  Offline: make_peak_offline_record.events."""
    if c["kind"] == "offline":
        return mo.events(c, r1 if marker == 1.0 else rm, sm, marker)
    ev = r1 == 1.0
    ret = r1 if marker == 1.0 else rm
    count, index, values = [], [], []
    for b in range(c["nblocks"]):
        for ch in range(c["nch"]):
            i = np.nonzero(ev[b, :, ch])[0]
            count.append(int(i.size))
            index += i.tolist()
            values += ret[b, i, ch].tolist()
    return count, index, values


def main():
    with refrecord.ref_library("peak", ["lib_rspt/lib_filter/iir_filter_design.cpp"], ["lib_rspt"]) as Lon, \
            refrecord.ref_library("peak_offline", ["lib_rspt/lib_filter/iir_filter_design.cpp"], ["lib_rspt"]) as Loff:
        mp.bind(Lon)
        mo.bind(Loff)
        out = {"generator": "tests/golden/make_peak_planar_record.py (peak_detector.h, iir_filter_opt.h, filter.h, lib_filter/iir_filter_design.cpp + "
                            "tests/golden/peak_shim.cpp, peak_offline_shim.cpp, g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of a trace transposed to [nblocks][ns][nch] float64, NaNs made one (tests/peak_cases.py: tdigest)",
               "cases": []}
        for c in pp.recorded_cases():
            r1, s1, h1 = run(Lon, Loff, c, 1.0)
            rm, sm, hm = run(Lon, Loff, c, -1.0)
            assert pc.tdigest(s1) == pc.tdigest(sm) and pc.tdigest(h1) == pc.tdigest(hm), c["name"]
            count, index, values = events(c, r1, rm, s1, 1.0)
            assert all(v == 1.0 for v in values), c["name"]
            count_m1, index_m1, values_m1 = events(c, r1, rm, sm, -1.0)
            rec = {"name": c["name"], "kind": c["kind"], "variant": c["variant"], "fs": c["fs"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"],
                   "nblocks": c["nblocks"], "stateful": c["stateful"], "calls": c["calls"], "in_crc32": pp.crc(pp.matrix_bytes(c["planar"])),
                   "count": count, "index": index, "count_m1": None if count_m1 == count else count_m1,
                   "index_m1": None if index_m1 == index else index_m1, "values_m1": pc.vhex(values_m1),
                   "sig": pc.tdigest(s1), "thr": pc.tdigest(h1)}
            out["cases"].append(rec)
            print(c["name"], sum(count), "events", flush=True)
    refrecord.write_record("peak_planar_record.json", out)


if __name__ == "__main__":
    main()
