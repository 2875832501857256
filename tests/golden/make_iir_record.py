#!/usr/bin/env python3
"""Generate tests/golden/iir_record.json: the reference's IIR pre-filter (lib_rspt/lib_filter/iir_filter.cpp, compiled into
oracle/_ref by oracle/Makefile and driven as its test harness drives it: oracle/ref_shim.cpp ref_iir_prefilter_native) on
the inputs of tests/iir_cases.py.

Per case the record holds the shape, the coefficients bit for bit (64-bit hex words: NaN signs included), the crc32 of the
input and the digest (tests/cases.py) of the filtered block in both drivings:
    shared        one filter object for all channels of the block (Ref.iir_prefilter on the block), as the harness does;
    per_channel   a fresh filter per channel (the reference on each channel as a block of one channel).

    python tests/golden/make_iir_record.py          (needs oracle/_ref/librspt_ref.so: python -c "from oracle import oracle; oracle.build()")
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))  # (tests/test_iir_edges.py loads this file by its path)

import refrecord  # noqa: E402

refrecord.repo_paths()

import iir_cases as ic  # noqa: E402
from cases import digest  # noqa: E402
from casetools import record_text as _text  # noqa: E402


def per_channel(filt, c):
    """the block filtered channel by channel, each channel a block of its own (a fresh filter object each)"""
    bps, nch, ns = c["bps"], c["nch"], c["ns"]
    blk = np.asarray(c["data"], dtype=np.uint8).reshape(ns, nch, bps)
    out = np.empty_like(blk)
    for ch in range(nch):
        one = np.ascontiguousarray(blk[:, ch, :]).reshape(-1)
        out[:, ch, :] = np.frombuffer(filt(one, bps, 1, ns, c["n"], c["d"], c["init"]), dtype=np.uint8).reshape(ns, bps)
    return out.reshape(-1)


def record_text(filt):
    """the record's text, filt(native, bps, nch, ns, n, d, init) -> bytes being the harness's driving of the reference (the tests
    pass the restatement, which the record pins to the reference, to check that the text is reproduced byte for byte)"""
    recs = []
    for c in ic.all_cases():
        rec = {"name": c["name"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "init": c["init"], "n": ic.to_bits(c["n"]),
               "d": ic.to_bits(c["d"]), "in_crc32": ic.crc(c["data"])}
        rec["shared"] = digest(np.frombuffer(bytes(filt(c["data"], c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"])), dtype=np.uint8))
        rec["per_channel"] = digest(per_channel(filt, c))
        recs.append(rec)
    return _text({"generator": "tests/golden/make_iir_record.py (lib_filter/iir_filter.cpp + oracle/ref_shim.cpp, g++ -O2 -std=gnu++11)",
                  "digest": "first 32 hex digits of the sha256 of the filtered native bytes (tests/cases.py: digest)", "cases": recs})


def main():
    from oracle.oracle import Ref

    text = record_text(Ref().iir_prefilter)
    with open(os.path.join(refrecord.HERE, "iir_record.json"), "w") as f:
        f.write(text)
    print("%d cases" % text.count('"name"'))


if __name__ == "__main__":
    main()
