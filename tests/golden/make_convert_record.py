#!/usr/bin/env python3
"""Generate tests/golden/convert_record.json: what the reference's convert_native_to_i32 / convert_i32_to_native
(lib_rspt/lib_signalpacker/utils.cpp:51-191) return for the inputs of tests/convert_cases.py, and size and hash of the streams
its packers make of a few blocks of more than 8192 channels (tests/golden/convert_shim.cpp drives both).

The script compiles the reference's lib_signalpacker, lib_zaxtensor, lib_filter, lib_hzr and lib_fwht sources and the shim
(gcc -O2 -std=c11 -DNDEBUG, g++ -O2 -std=gnu++11) into a temporary directory outside the repository, writes the record and
deletes the build.  Large outputs appear as size and FNV-1a only.

    python tests/golden/make_convert_record.py [--ref DIR]     (DIR: the reference's root, default $REF or /root/reference)
"""
import ctypes as C
import os

import numpy as np
import refrecord

refrecord.repo_paths()

import convert_cases as cc  # noqa: E402

KINDS = {"hzr": 0, "xdelta_hzr": 1, "dct": 2, "hadamard": 3}


class ShimBackend:
    def __init__(self, L):
        self.L = L
        L.convert_shim_native_to_i32.restype = None
        L.convert_shim_native_to_i32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.convert_shim_i32_to_native.restype = None
        L.convert_shim_i32_to_native.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.convert_shim_pack.restype = C.c_size_t
        L.convert_shim_pack.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_size_t]

    def native_to_i32(self, native, ns, nch, bps, reverse):
        a = np.zeros(native.size + 8, dtype=np.uint8)  # (the reference reads whole int32s: up to 3 bytes past the last sample)
        a[: native.size] = native
        out = np.zeros((nch, ns), dtype=np.int32)
        self.L.convert_shim_native_to_i32(out.ctypes.data, a.ctypes.data, ns, nch, bps, int(reverse))
        return out

    def i32_to_native(self, planar, bps, reverse):
        pl = np.ascontiguousarray(planar, dtype=np.int32)
        nch, ns = pl.shape
        out = np.zeros(bps * nch * ns + 8, dtype=np.uint8)
        self.L.convert_shim_i32_to_native(out.ctypes.data, pl.ctypes.data, ns, nch, bps, int(reverse))
        return out[: bps * nch * ns].tobytes()

    def pack(self, kind, bps, nch, ns, nb, data):
        a = np.zeros(data.size + 8, dtype=np.uint8)
        a[: data.size] = data
        cap = 2 * data.size + 4096
        out = np.zeros(cap + 64, dtype=np.uint8)
        n = self.L.convert_shim_pack(KINDS[kind], a.ctypes.data, bps, nch, ns, nb, out.ctypes.data, cap)
        return out[:n].tobytes()


def main():
    from oracle.oracle import Oracle

    with refrecord.ref_library("convert", **refrecord.PACKERS) as L:
        entries = cc.record_cases(ShimBackend(L), Oracle().fnv1a)
    with open(os.path.join(refrecord.HERE, "convert_record.json"), "w") as f:
        f.write(cc.dump_record(entries))  # (tests/test_convert.py makes the same text again from oracle/_ref)
    print("%d cases" % len(entries))


if __name__ == "__main__":
    main()
