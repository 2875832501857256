#!/usr/bin/env python3
"""Generate tests/golden/hadamard_rows_record.json: what the reference's hadamard packer writes and decodes at every row length
2^1 .. 2^16, for the shapes, the ladder and the blocks of tests/hadamard_rows_cases.py.

The reference is the one of make_lossy_quantizer_record.py -- its build() and roundtrip(): the temporary copy outside the
repository whose `quality` / nr_bytes_to_compress_ constants are read when a packer is constructed, run with the stack limit
lifted -- and nothing of its text is kept.  Per case, ladder entry and block:
  in_crc32, size, crc32, dec_crc32   of the input, the stream, the decoded block
  stream, decoded                    in full (base64) where the native block is at most lossy_quantizer_cases.FULL_LIMIT bytes

    python tests/golden/make_hadamard_rows_record.py [--ref DIR]
"""
import shutil
import tempfile

import make_lossy_quantizer_record as mlq
import refrecord

refrecord.repo_paths()

import hadamard_rows_cases as hr  # noqa: E402
import lossy_quantizer_cases as lq  # noqa: E402


def main():
    ref = refrecord.ref_root()
    out = {"generator": "tests/golden/make_hadamard_rows_record.py (build() and roundtrip() of tests/golden/make_lossy_quantizer_record.py)",
           "ladder": [float(q).hex() for q in hr.LADDER], "cases": []}
    tmp = tempfile.mkdtemp(prefix="hadamard_rows_ref_")
    try:
        L = mlq.build(ref, tmp)
        for k in hr.KS:
            kind, bps, nch, ns, nb = hr.shapes()[k]
            e = dict(k=k, kind=kind, bps=bps, nch=nch, ns=ns, nb=nb, entries=[])
            full = bps * nch * ns <= lq.FULL_LIMIT
            for q in hr.LADDER:
                blocks = []
                for data in hr.natives(k):
                    s, dec = mlq.roundtrip(L, kind, q, nb, data, bps, nch, ns)
                    b = {"in_crc32": lq.crc(data), "size": len(s), "crc32": lq.crc(s), "dec_crc32": lq.crc(dec)}
                    if full:
                        b["stream"], b["decoded"] = lq.pack(s), lq.pack(dec)
                    blocks.append(b)
                e["entries"].append({"q_hex": float(q).hex(), "blocks": blocks})
            out["cases"].append(e)
            print("%-28s sizes %s" % (hr.case_id(k), [[b["size"] for b in x["blocks"]] for x in e["entries"]]), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    refrecord.write_record("hadamard_rows_record.json", out)


if __name__ == "__main__":
    mlq.with_the_stack_limit_lifted(main)
