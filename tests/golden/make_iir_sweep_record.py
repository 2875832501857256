#!/usr/bin/env python3
"""Generate tests/golden/iir_sweep_record.json: the reference's IIR filter (lib_rspt/lib_filter/iir_filter.cpp) on every case of
the seeded sweep of tests/iir_sweep_cases.py, driven per leg as the stage's own record generator drives it:
    single          make_iir_record.py's drivings of oracle/_ref (oracle/ref_shim.cpp ref_iir_prefilter_native): a block with one
                    shared filter object, or channel by channel as blocks of one channel
    single_stream   tests/golden/stream_filter_shim.cpp (make_stream_filter_record.py): one object per channel over all blocks
    cascade         tests/golden/iir_cascade_shim.cpp (make_iir_cascade_record.py), a fresh chain for every block
    cascade_stream  the same shim, one chain per channel living on from block to block
    zero_phase      tests/golden/iir_zero_phase_shim.cpp (make_iir_zero_phase_record.py)

The shims are compiled with the oracle's reference flags (g++ -O2 -std=gnu++11, plain x86-64: no fused multiply-add) into
temporary directories outside the repository, which go when the run ends.  The record holds per case the name, the leg, the
handle's shape and the block count, the crc32 of the input, and the crc32 and digest (tests/cases.py) of the answer in the native
width.  The coefficients are the named sets of the case modules, so the cases restate them exactly.

    python tests/golden/make_iir_sweep_record.py [--ref DIR]     (needs oracle/_ref/librspt_ref.so: python -c "from oracle import oracle; oracle.build()")
"""
import numpy as np
import refrecord

refrecord.repo_paths()

import fir_cases as fc  # noqa: E402
import iir_sweep_cases as sw  # noqa: E402
import make_iir_cascade_record as casc  # noqa: E402
import make_iir_record as single  # noqa: E402
import make_iir_zero_phase_record as zp  # noqa: E402
import make_stream_filter_record as stream  # noqa: E402
from cases import digest  # noqa: E402

IIR = ["lib_rspt/lib_filter/iir_filter.cpp"]


def run_single(ref, c):
    """block by block: the harness's driving (one object for the block's channels), or a fresh object per channel"""
    bb = c["bps"] * c["nch"] * c["ns"]
    out = np.empty_like(c["data"])
    for b in range(c["nblocks"]):
        blk = dict(c, data=c["data"][b * bb : (b + 1) * bb])
        if c["shared"]:
            y = np.frombuffer(bytes(ref.iir_prefilter(blk["data"], c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"])), dtype=np.uint8)
        else:
            y = single.per_channel(ref.iir_prefilter, blk)
        out[b * bb : (b + 1) * bb] = y
    return out


def main():
    from oracle.oracle import Ref

    ref = Ref()
    S = sw.sweep_cases()
    with refrecord.ref_library("stream_filter", IIR + ["lib_rspt/lib_filter/fir_filter.cpp"], ["lib_rspt"]) as Ls, \
            refrecord.ref_library("iir_cascade", IIR, ["lib_rspt"]) as Lc, refrecord.ref_library("iir_zero_phase", IIR, ["lib_rspt"]) as Lz:
        stream.bind(Ls)
        casc.bind(Lc)
        zp.bind(Lz)
        drive = {"single": lambda c: run_single(ref, c), "single_stream": lambda c: stream.run(Ls, dict(c, kind="iir")),
                 "cascade": lambda c: casc.run(Lc, c, 0), "cascade_stream": lambda c: casc.run(Lc, c, 1), "zero_phase": lambda c: zp.run(Lz, c)}
        out = {"generator": "tests/golden/make_iir_sweep_record.py (lib_filter/iir_filter.cpp + oracle/ref_shim.cpp, tests/golden/stream_filter_shim.cpp, "
                            "iir_cascade_shim.cpp, iir_zero_phase_shim.cpp, g++ -O2 -std=gnu++11)",
               "digest": "first 32 hex digits of the sha256 of the filtered native bytes (tests/cases.py: digest)",
               "cases": []}
        for leg in sw.LEGS:
            for c in S[leg]:
                y = np.ascontiguousarray(drive[leg](c), dtype=np.uint8).reshape(-1)
                assert y.size == c["data"].size, c["name"]
                out["cases"].append({"name": c["name"], "leg": leg, "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "nblocks": c["nblocks"],
                                     "in_crc32": fc.crc(c["data"]), "crc32": fc.crc(y), "digest": digest(y)})
            print(leg, len(S[leg]), "cases", flush=True)
    refrecord.write_record("iir_sweep_record.json", out)


if __name__ == "__main__":
    main()
