#!/usr/bin/env python3
"""Time the PRDN stage (rspt_hip_prdn_batch_dev) on 64 x (64 ch x 65536 int32) of the bench's synthetic blocks and
print one JSON line.

    --mode fast   small errors: every block takes the exact-integer path.  Also times a device copy of the batch in the same
                  process; the byte floor of the stage is 3 x the batch (o twice, d once) at that rate = 1.5 x the copy's time
    --mode seq    errors up to 2^28: every block takes the sequential path
    --mode orc    the reference-side figure: orc.prdn (the CPU restatement of the reference's loop) over the same batch
Blocks 0 and B-1 are checked against orc.prdn by bit pattern after the timed region.  tools/prdn_rate.sh runs the three modes,
each under its own time limit, and merges the lines into profiles/prdn_bench.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NB, BPS, NCH, NS = 64, 4, 64, 65536


def batch(mode):
    """(orig, dec) uint8 [NB, block_bytes] on the host"""
    import prdn_cases as pc
    from rspt_amd import synth

    o = np.stack([synth.synth_native(NCH, NS, b).numpy().reshape(-1) for b in range(NB)])
    amp = (1 << 28) if mode == "seq" else 16
    d = np.stack([pc._noisy(o[b], BPS, NCH, NS, 2000 + b, amp) for b in range(NB)])
    return o, d


def timed(fn, iters, warmup=2):
    import torch

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["fast", "seq", "orc"], required=True)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import prdn_cases as pc
    from oracle.oracle import Oracle

    orc = Oracle()
    o, d = batch("fast" if a.mode == "orc" else a.mode)
    nbytes = o.size
    res = dict(tool="prdn_rate", mode=a.mode, shape="64x(64ch x 65536 i32)", bytes=nbytes)
    if a.mode == "orc":
        t0 = time.perf_counter()
        v = [orc.prdn(o[b], d[b], NS, NCH, BPS) for b in range(NB)]
        res.update(ms=round((time.perf_counter() - t0) * 1e3, 1), prdn0=pc.hexbits(v[0]))
    else:
        import torch

        from rspt_amd import api

        assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
        pk = api.new_hzr(BPS, NCH, NS)
        do, dd = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        pk.reserve(NB)
        iters = a.iters if a.mode == "fast" else max(2, a.iters // 5)
        ms = timed(lambda: pk.prdn_batch(do.reshape(-1), dd.reshape(-1)), iters)
        p, mse, ref, path = pk.prdn_batch(do.reshape(-1), dd.reshape(-1), parts=True)
        torch.cuda.synchronize()
        ok = all(int(p[b : b + 1].cpu().numpy().view(np.uint64)[0]) == pc.bits(orc.prdn(o[b], d[b], NS, NCH, BPS)) for b in (0, NB - 1))
        res.update(device=torch.cuda.get_device_name(0), iters=iters, ms=round(ms, 4), sequential_blocks=int(path.sum()), checked_blocks_ok=ok,
                   gsamples_per_s=round(NB * NCH * NS / (ms * 1e-3) / 1e9, 2))
        if a.mode == "fast":
            tmp = torch.empty_like(do)
            copy_ms = timed(lambda: tmp.copy_(do), a.iters)
            res.update(copy_ms=round(copy_ms, 4), copy_tb_per_s=round(2 * nbytes / (copy_ms * 1e-3) / 1e12, 3), floor_ms=round(1.5 * copy_ms, 4),
                       x_floor=round(ms / (1.5 * copy_ms), 2))
        pk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
