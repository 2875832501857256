#!/usr/bin/env python3
"""Generate tests/golden/prdn_record.json: the PRDN[%] that the reference's own test_packer_ (lib_rspt_test/rspt_test.cpp:58-112)
prints for the inputs of tests/prdn_cases.py (tests/golden/prdn_shim.cpp drives it).

The script compiles the reference's lib_signalpacker, lib_zaxtensor, lib_filter, lib_hzr and lib_fwht sources and the shim
(gcc -O2 -std=c11 -DNDEBUG, g++ -O2 -std=gnu++11) into a temporary directory outside the repository, runs every case INSIDE that
directory (test_packer_ writes _original.bin and _decoded.bin where it runs), writes the record and deletes the build.
Nothing under oracle/ is used: the lossy fixtures go through the reference's real dct / hadamard round trip, and the decoded
block the reference leaves behind is what the record's crc32 describes.  Per case the record holds
  orig_crc32, dec_crc32   of the two native blocks
  prdn                    the reference's figure, as the 16 hex digits of the double ("-nan" is 0xFFF8000000000000)
  mse, ref, path          from the numpy restatement (tests/prdn_cases.py) -- the reference prints PRDN only; path = 1 where a sum
                          depends on the order of its adds (the GPU stage's sequential path)
Full-size cases appear only as these figures, never as data.

    python tests/golden/make_prdn_record.py [--ref DIR]     (DIR: the reference's root, default $REF or /root/reference,
                                                              as in oracle/Makefile)
"""
import ctypes as C
import os
import struct

import numpy as np
import refrecord

refrecord.repo_paths()

import prdn_cases as pc  # noqa: E402

KINDS = {"dct": 2, "hadamard": 3}


def bind(L):
    L.prdn_shim_run.restype = C.c_int
    L.prdn_shim_run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.prdn_shim_packer.restype = C.c_int
    L.prdn_shim_packer.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]


def printed_bits(text):
    """what the reference printed with 17 significant digits -> the double's bit pattern"""
    t = text.decode().strip().lower()
    if "nan" in t:
        return 0xFFF8000000000000 if t.startswith("-") else 0x7FF8000000000000
    return struct.unpack("<Q", struct.pack("<d", float(t)))[0]


def entry(c, prdn_bits):
    p, mse, ref, path, info = pc.prdn_parts(c["orig"], c["dec"], c["bps"], c["nch"], c["ns"])
    return {"name": c["name"], "group": c["group"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "orig_crc32": pc.crc(c["orig"]),
            "dec_crc32": pc.crc(c["dec"]), "prdn": "%016x" % prdn_bits, "mse": pc.hexbits(mse), "ref": pc.hexbits(ref), "path": path}


def main():
    out = {"generator": "tests/golden/make_prdn_record.py (lib_rspt_test/rspt_test.cpp test_packer_ + tests/golden/prdn_shim.cpp, g++ -O2 -std=gnu++11)",
           "prdn": "the reference's printed figure as the bit pattern of the double",
           "mse, ref, path": "from the numpy restatement tests/prdn_cases.py:prdn_parts (the reference prints PRDN only)", "cases": []}
    cwd = os.getcwd()
    with refrecord.ref_library("prdn", **refrecord.PACKERS) as L:
        bind(L)
        os.chdir(L.tmp)  # (test_packer_ writes _original.bin and _decoded.bin where it runs)
        try:
            buf = C.create_string_buffer(256)
            for c in pc.synthetic_cases() + [pc.ref_seq_case()]:
                rc = L.prdn_shim_run(c["orig"].ctypes.data, c["dec"].ctypes.data, c["ns"], c["nch"], c["bps"], buf, len(buf))
                assert rc == 0, (c["name"], rc)
                e = entry(c, printed_bits(buf.value))
                out["cases"].append(e)
                print(e["name"], buf.value.decode(), e["prdn"], "path", e["path"], flush=True)
            for f in pc.lossy_fixtures():
                data = np.ascontiguousarray(f["data"])
                rc = L.prdn_shim_packer(KINDS[f["kind"]], data.ctypes.data, f["ns"], f["nch"], f["bps"], buf, len(buf))
                assert rc == 0, (f["name"], rc)
                with open("_decoded.bin", "rb") as fh:
                    e = entry(pc.lossy_case(f, fh.read()), printed_bits(buf.value))
                e["kind"] = f["kind"]
                out["cases"].append(e)
                print(e["name"], buf.value.decode(), e["prdn"], "path", e["path"], flush=True)
        finally:
            os.chdir(cwd)
    refrecord.write_record("prdn_record.json", out)


if __name__ == "__main__":
    main()
