#!/usr/bin/env python3
"""Time the carried-state rolling median (rspt_hip_median_filter_stream_dev) against the stateless stage of
another build of the library -- the parent commit's -- and print one JSON line.

The other build is loaded beside this one in the same process (--parent-lib: a librspt_hip.so built from the parent commit,
bound by api.bind; only its packer_create / destroy and rspt_hip_median_filter_batch_dev are called), so that both sides see the
same buffers and their runs alternate: parent, branch, parent, branch, ...  Per side: the median ms per call over the runs and
the spread (max - min).

  shape  64 ch x 4,194,304 rows of int32: 64 blocks of 64 ch x 65536 as ONE stream call on a state that has started, against
         the parent's stateless call on the same bytes as 64 blocks; out of place and in place; W = 3, 7, 31, 101, 1001, 8191,
         65536
  W <= 32   `margin_ok`: the branch's median is not above the parent's by more than twice the parent's spread
  W > 32    the stream call sorts (L + W - 1) / L rows per output row (L: the new rows of a segment): `yardstick_ms` is the
            parent's time times that overlap factor, `over_yardstick` the branch's ratio to it, and `margin_ok` whether the
            branch is within twice the parent's spread of the yardstick
Without --parent-lib only the branch's side is timed.  After the timed region the stream result of a fresh state on the first
4 blocks is compared with this build's stateless result on a one-block handle of 4 x 65536 rows.

    python tools/median_stream_rate.py [--parent-lib FILE] [--runs N] [--iters N] [--ws 3,7,...] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rspt_amd import api, synth  # noqa: E402
from stream_filter_rate import versus  # noqa: E402


class Parent:
    """the stateless median entry of another build"""

    def __init__(self, path):
        self.L = api.bind(C.CDLL(path), missing_ok=True)  # (a parent build lacks this build's newer entries)

    def packer(self, bps, nch, ns):
        h = C.c_void_p()
        assert self.L.rspt_hip_packer_create(C.byref(h), api.KIND_HZR, bps, nch, ns, 3, 0) == 0
        return h

    def median(self, h, src, dst, nblocks, W):
        st = torch.cuda.current_stream().cuda_stream
        assert self.L.rspt_hip_median_filter_batch_dev(h, src.data_ptr(), dst.data_ptr(), nblocks, W, st) == 0


def segment_rows(W, rows):
    """median_segment_rows of host_stages.hip: the segment capacity S = W - 1 + L"""
    want = 8 * (W - 1)
    S = (1 << 16) if want <= (1 << 16) else (1 << 17) if want <= (1 << 17) else (1 << 18)
    return min(S, W - 1 + rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--ws", default="3,7,31,101,1001,8191,65536")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    parent = Parent(a.parent_lib) if a.parent_lib else None
    bps, nch, ns, B = 4, 64, 65536, 64
    pk = api.new_hzr(bps, nch, ns)
    one = api.new_hzr(bps, nch, ns * 4)
    ph = parent.packer(bps, nch, ns) if parent else None
    pristine = synth.synth_batch_native(B, nch, ns, bps=bps, ecg=True, device="cuda").reshape(-1)
    src, dst = pristine.clone(), torch.empty_like(pristine)
    res = []
    for W in (int(w) for w in a.ws.split(",")):
        state = pk.median_state(W)
        pk.median_filter_batch(pristine, W, d_dst=dst, state=state)  # the state has started
        for in_place in (False, True):
            out = src if in_place else dst
            r = versus((lambda: parent.median(ph, src, out, B, W)) if parent else None,
                       lambda: pk.median_filter_batch(src, W, d_dst=None if in_place else dst, state=state), a.runs, a.iters)
            src.copy_(pristine)
            x = pk.median_filter_batch(src[: 4 * pk.block_bytes].clone(), W, state=pk.median_state(W))
            y = one.median_filter_batch(src[: 4 * pk.block_bytes].clone(), W)
            torch.cuda.synchronize()
            r.update(shape="64ch x 4194304 rows i32 (64 blocks of 65536, one stream call)", W=W, in_place=in_place, checked_ok=bool(torch.equal(x, y)))
            if W > 32:
                S = segment_rows(W, B * ns)
                L = S - (W - 1)
                r.update(segment_rows=S, overlap_factor=round(S / L, 4))
                if parent:
                    r["yardstick_ms"] = round(r["parent_ms"] * S / L, 4)
                    r["over_yardstick"] = round(r["branch_ms"] / r["yardstick_ms"], 4)
                    r["margin_ok"] = bool(r["branch_ms"] <= r["yardstick_ms"] + 2 * r["parent_spread_ms"])
            res.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    if parent:
        parent.L.rspt_hip_packer_destroy(ph)
    pk.close()
    one.close()
    line = json.dumps(dict(tool="median_stream_rate", device=torch.cuda.get_device_name(0), runs_per_side=a.runs, iters=a.iters,
                           parent=bool(parent), results=res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
