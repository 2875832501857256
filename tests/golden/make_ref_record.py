#!/usr/bin/env python3
"""Generate tests/golden/ref_record.json: the compiled reference's answers to the seeded inputs of the tests that pin the
restatement to it (test_oracle_vs_ref.py, the big-endian ingest of test_host_side.py, test_iir_prefilter.py,
test_oracle_dct_big.py, test_oracle_golden.py).

Needs oracle/_ref/librspt_ref.so, which oracle/Makefile compiles from the reference's own sources where they are present;
the tests themselves then run anywhere.  The record is data: per input its crc32 (drift check) and the reference's outputs
in the same call order the tests use, as cases.digest() of the bytes (the full stream where a test decodes it).

    python tests/golden/make_ref_record.py
"""
import json
import os
import struct
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cases  # noqa: E402
from cases import digest  # noqa: E402
from oracle.oracle import Ref  # noqa: E402


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def chunk_count(stream):
    pos, k = 1, 0
    while pos < len(stream):
        pos += 4 + struct.unpack_from("<I", stream, pos)[0]
        k += 1
    return k


def main():
    ref = Ref()
    out = {"generator": "tests/golden/make_ref_record.py (oracle/_ref: the reference compiled by oracle/Makefile)",
           "digest": "first 32 hex digits of the sha256 of the bytes (tests/cases.py: digest)"}

    out["hzr_encode"] = []
    for seed in range(cases.HZR_SOUP_SEEDS):
        d = cases.hzr_soup_block(seed)
        out["hzr_encode"].append([crc(d), digest(ref.hzr_encode(d))])

    pb = {"in_crc32": {}, "streams": {}}
    for n in cases.PAYLOAD_BOUNDARY_SIZES:
        blocks = [cases.payload_boundary_block(n, seed) for seed in range(cases.PAYLOAD_BOUNDARY_SEEDS)]
        pb["in_crc32"][str(n)] = crc(np.concatenate(blocks))
        pb["streams"][str(n)] = [digest(ref.hzr_encode(d)) for d in blocks]
    out["hzr_payload_boundary"] = pb

    out["packers"] = []
    for seed in range(cases.RANDOM_PACKER_SEEDS):
        c = cases.random_packer_case(seed)
        pr = ref.packer(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"])
        calls = []
        for rep in range(2):  # second call exercises the persisted nb
            s = pr.compress(c["data"])
            dec, used, _ = pr.decompress(s)
            calls.append([digest(s), digest(dec), used])
        pr.close()
        out["packers"].append({"in_crc32": crc(c["data"]), "calls": calls})

    nb = {"in_crc32": [], "nb": []}
    for seed in range(cases.NEEDED_NB_SEEDS):
        c = cases.needed_nb_case(seed)
        pr = ref.packer("xdelta_hzr", c["bps"], c["nch"], c["ns"], c["nb"])
        nb["in_crc32"].append(crc(c["data"]))
        nb["nb"].append(chunk_count(pr.compress(c["data"])))
        pr.close()
    out["needed_nb"] = nb

    be_rec = {}
    nch, ns = cases.BIG_ENDIAN_SHAPE
    for bps in (1, 2, 3, 4):
        le = cases.big_endian_block(bps)
        be = cases.reverse_samples(le, bps)
        a = ref.native_to_i32(le, ns, nch, bps, reverse_byte_order=False)
        b = ref.native_to_i32(be, ns, nch, bps, reverse_byte_order=True)
        be_rec[str(bps)] = {"in_crc32": crc(le), "le_i32": digest(a), "be_i32": digest(b),
                            "be_native": digest(ref.i32_to_native(a, bps, reverse_byte_order=True))}
    out["big_endian"] = be_rec

    out["iir"] = {}
    for c in cases.iir_cases():
        f = ref.iir_prefilter(c["data"], c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"])
        out["iir"][c["name"]] = {"in_crc32": crc(c["data"]), "filtered": digest(f)}

    data = cases.iir_full_scale_data()
    nch, ns, bps = cases.IIR_FULL_SCALE_SHAPE
    out["iir_full_scale"] = {"in_crc32": crc(data)}
    for name, coef in cases.IIR_FULL_SCALE_COEFS.items():
        out["iir_full_scale"][name] = digest(ref.iir_prefilter(data, bps, nch, ns, coef[0], coef[1], 2000))

    out["dct_vs_fp64"] = {}
    for bps, nch, ns, ecg in cases.DCT_VS_FP64_SHAPES:
        data = cases.dct_vs_fp64_data(bps, nch, ns, ecg)
        pr = ref.packer("dct", bps, nch, ns)
        s = pr.compress(data)
        dec, used, _ = pr.decompress(s)
        assert used == len(s)
        pr.close()
        out["dct_vs_fp64"]["%d_%d_%d" % (bps, nch, ns)] = {"in_crc32": crc(data), "stream": s.hex(), "decoded": digest(dec)}

    out["dct_out_of_range"] = {}
    for bps, nch, ns, amp in cases.DCT_OUT_OF_RANGE_SHAPES:
        rows = []
        for seed in range(cases.DCT_OUT_OF_RANGE_SEEDS):
            x = cases.dct_out_of_range_data(bps, nch, ns, amp, seed)
            pr = ref.packer("dct", bps, nch, ns)
            s = pr.compress(x)
            rows.append([crc(x), digest(s), digest(pr.decompress(s)[0])])
            pr.close()
        out["dct_out_of_range"]["%d_%d_%d_%d" % (bps, nch, ns, amp)] = rows

    path = os.path.join(HERE, "ref_record.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=False)
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
