#!/usr/bin/env python3
"""Time the rolling-median stage (rspt_hip_median_filter_batch_dev) and print one JSON line.

Runs: W in {1, 3, 5, 7, 31, 101, 1001, 8191, 65536} on 64 x (64 ch x 65536 int32), and on 1024 x (3 ch x 20000 int24), in place
and out of place.  Per run: ms per call (device events around back-to-back calls), GSamples/s, and the copy floor measured in
the same process (copy_frac: a device copy of the batch, read + write of every byte, over the call's time).  After the timed
region blocks 0 and B-1 of a fresh call are checked against the restatement (tests/median_cases.py) where it is quick (W up to
1001), and against the record's crc32 for the full-size block at W = 101 and 65536.

    python tools/median_rate.py [--iters N] [--ws 1,3,...] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import median_cases as mc  # noqa: E402
from rspt_amd import api, synth  # noqa: E402


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def shape_runs(name, bps, nch, ns, nblocks, block_fn, ws, iters, res, crcs=None):
    pk = api.new_hzr(bps, nch, ns)
    host = np.stack([block_fn(b) for b in range(nblocks)])
    pristine = torch.from_numpy(host).cuda()
    src = pristine.clone()
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), iters)
    samples = nblocks * nch * ns
    for W in ws:
        for in_place in (False, True):
            call = (lambda: pk.median_filter_batch(src, W)) if in_place else (lambda: pk.median_filter_batch(src, W, d_dst=dst))
            ms = timed(call, iters)
            src.copy_(pristine)
            out = pk.median_filter_batch(src, W, d_dst=None if in_place else dst)
            torch.cuda.synchronize()
            check = None
            if crcs and str(W) in crcs:
                check = all(mc.crc(out[b].cpu().numpy()) == crcs[str(W)] for b in (0, nblocks - 1))
            elif W <= 1001:
                check = all(np.array_equal(out[b].cpu().numpy(), mc.median_filter(host[b], bps, nch, ns, W)) for b in (0, nblocks - 1))
            src.copy_(pristine)
            res.append(dict(shape=name, W=W, in_place=in_place, ms=round(ms, 4), gsamples_per_s=round(samples / (ms * 1e-3) / 1e9, 2),
                            copy_ms=round(copy_ms, 4), copy_frac=round(copy_ms / ms, 3), checked_blocks_ok=check, bytes=nblocks * bps * nch * ns))
            print(json.dumps(res[-1]), file=sys.stderr, flush=True)
    pk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ws", default="1,3,5,7,31,101,1001,8191,65536")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    ws = [int(v) for v in a.ws.split(",")]
    with open(os.path.join(ROOT, "tests", "golden", "median_record.json")) as f:
        big = json.load(f)["big"]
    res = []
    # every block of the big shape is the record's block, so the record's crc32 checks blocks 0 and B-1
    shape_runs("64x(64ch x 65536 i32)", 4, 64, 65536, 64, lambda b: mc.big_data(), ws, a.iters, res, crcs=big["crc32"])
    ds = np.frombuffer(synth.data_stream_3ch_i24(), dtype=np.uint8)
    shape_runs("1024x(3ch x 20000 i24)", 3, 3, 20000, 1024, lambda b: ds, ws, a.iters, res)
    line = json.dumps(dict(tool="median_rate", device=torch.cuda.get_device_name(0), iters=a.iters, runs=res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
