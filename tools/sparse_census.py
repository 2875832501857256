#!/usr/bin/env python3
"""What the sparse segments of k_hist's "medium" blocks hold (CPU only): the census behind the compacted row of
hist_segment_sparse (profiles/sparse_segments_notes.md).

The benchmark's signal blocks (synth.synth_i32, 64 ch x 65536 x int32) go through the oracle's xdelta transform; planes 1 and 2
are cut into hzr blocks (64 KiB), 4 KiB segments, 1 KiB rows and 16-byte granules as k_hist sees them.  A block is k_hist's
when more than two of its segments are non-zero.  Per plane: blocks taken, non-zero segments, dense rows (49 or more non-zero
granules), all-zero rows, non-zero granules per segment (what the compaction must fit into 64 lanes) and literals per segment
(what the 512-entry queue must hold).

usage: sparse_census.py [block_index ...]      (default: 0 37)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def planes_of(orc, block_index, nch=64, ns=65536):
    from rspt_amd import synth

    native = synth.synth_native(nch, ns, block_index).numpy()
    v = orc.xdelta_forward(orc.native_to_i32(native, ns, nch, 4))
    return v.view(np.uint8).reshape(-1, 4)


def census(plane):
    n = plane.size // 65536 * 65536
    nz = plane[:n].reshape(-1, 16, 4, 64, 16) != 0  # [block][segment][row][granule][byte]
    gran = nz.any(axis=4)
    seg_nz = gran.any(axis=(2, 3))
    taken = seg_nz.sum(axis=1) > 2
    g, lits, segs = gran[taken], nz[taken].sum(axis=(2, 3, 4)), seg_nz[taken]
    per_seg = g.sum(axis=(2, 3))[segs]
    per_row = g.sum(axis=3)[segs]
    lit_seg = lits[segs]
    return {
        "blocks": int(taken.size), "taken": int(taken.sum()), "segments": int(segs.size), "nonzero_segments": int(segs.sum()),
        "dense_rows": int((per_row >= 49).sum()), "zero_rows_pct": 100.0 * float((per_row == 0).mean()) if per_row.size else 0.0,
        "granules_mean": float(per_seg.mean()) if per_seg.size else 0.0, "granules_max": int(per_seg.max()) if per_seg.size else 0,
        "le32_pct": 100.0 * float((per_seg <= 32).mean()) if per_seg.size else 0.0,
        "le64_pct": 100.0 * float((per_seg <= 64).mean()) if per_seg.size else 0.0,
        "literals_mean": float(lit_seg.mean()) if lit_seg.size else 0.0, "literals_max": int(lit_seg.max()) if lit_seg.size else 0,
    }


def main(argv):
    from oracle.oracle import Oracle

    orc = Oracle()
    for b in [int(a) for a in argv] or [0, 37]:
        p = planes_of(orc, b)
        for k in (1, 2):
            c = census(np.ascontiguousarray(p[:, k]))
            print("block %2d plane %d: %d of %d hzr blocks are k_hist's, %d of %d segments non-zero; rows: %d dense, %.1f %% all zero; "
                  "non-zero granules per segment: mean %.1f, max %d, <= 32: %.1f %%, <= 64: %.1f %%; literals per segment: mean %.1f, max %d"
                  % (b, k, c["taken"], c["blocks"], c["nonzero_segments"], c["segments"], c["dense_rows"], c["zero_rows_pct"], c["granules_mean"],
                     c["granules_max"], c["le32_pct"], c["le64_pct"], c["literals_mean"], c["literals_max"]))


if __name__ == "__main__":
    main(sys.argv[1:])
