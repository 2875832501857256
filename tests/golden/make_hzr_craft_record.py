#!/usr/bin/env python3
"""Generate tests/golden/hzr_craft_record.json: the compiled reference's verdict on every crafted stream of tests/hzr_craft.py
that may be given to it (libhzr's hzr_decode and hzr_verify through oracle/_ref: oracle/ref_shim.cpp).  Per case: the name, the
crc32 and length of the stream, whether hzr_decode succeeded and the digest (tests/cases.py) of what it wrote, hzr_verify's verdict
and the size it reports.  A case that is not for the compiled reference (more than 261 leaves: its node array is not bounded) is
listed with "reference": false and no verdict.

    python tests/golden/make_hzr_craft_record.py     (needs oracle/_ref/librspt_ref.so: python -c "from oracle import oracle; oracle.build()")
"""
import refrecord

refrecord.repo_paths()

import hzr_craft as hc  # noqa: E402
from cases import digest  # noqa: E402


def verdict(lib, c):
    """(decoded?, digest of the output, verified?, size): of lib.hzr_decode / lib.hzr_verify, the reference's or the restatement's"""
    try:
        out = lib.hzr_decode(c["stream"], c["n"])
        out = out[0] if isinstance(out, tuple) else out
        ok = True
    except RuntimeError:
        out, ok = b"", False
    v, size = lib.hzr_verify(c["stream"])
    return {"decode": ok, "digest": digest(out) if ok else None, "verify": v, "size": size}


def main():
    from oracle.oracle import Ref

    ref = Ref()
    out = {"generator": "tests/golden/make_hzr_craft_record.py (lib_hzr/hzr_decode.c through oracle/ref_shim.cpp)",
           "digest": "first 32 hex digits of the sha256 of the decoded bytes (tests/cases.py: digest)", "cases": []}
    for c in hc.craft_cases():
        r = {"name": c["name"], "crc32": c["crc32"], "len": len(c["stream"]), "reference": c["ref_safe"]}
        if c["ref_safe"]:
            assert c.get("tree", {}).get("leaves", 0) <= hc.MAX_LEAVES, c["name"]
            r.update(verdict(ref, c))
        out["cases"].append(r)
    refrecord.write_record("hzr_craft_record.json", out)
    print(len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
