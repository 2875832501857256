#!/usr/bin/env python3
"""Time the raw hzr byte-buffer codec (RSPT_HIP_KIND_BYTES) beside the emulation it replaces, and print one JSON line.

Input: 64 buffers of 16 MiB, two contents -- the raw bytes of the synthetic 64 x (64 ch x 65536 int32) batch, and plane 0 of
its xdelta transform (of blocks 0..15, four planes to a buffer, in turns) -- each through
  bytes      a RSPT_HIP_KIND_BYTES handle (new_bytes(16 MiB)): compress_batch and decompress_batch
  emulation  a RSPT_HIP_KIND_HZR handle with bps = 1, nch = 1: the same calls, four planes of work per buffer and a stream
             no libhzr reader takes
all four timed in this process with device events after a warm-up call.  After the timed region buffers 0, 21, 42 and 63
of each content are checked: the bytes stream against the oracle's hzr_encode, plane 0 of the emulation's stream too, and
both decodes against the input.  The record also holds the ingest kernel's own time (the handle's `preprocess` stage)
beside its byte floor -- bytes read plus bytes written at the device-copy rate this run measures.

    python tools/hzr_bytes_rate.py [--iters N] [--out FILE]
"""
import argparse
import json
import os
import struct
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.oracle import Oracle  # noqa: E402
from rspt_amd import api, synth  # noqa: E402

NBUF, SIZE = 64, 16 << 20
CHECKED = (0, 21, 42, 63)


def timed(fn, iters, warmup=1):
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


def contents(orc):
    raw = synth.synth_batch_native(NBUF, 64, 65536).numpy()  # [64, 16 MiB]
    planes = []
    for b in range(16):
        v = orc.xdelta_forward(orc.native_to_i32(raw[b], 65536, 64, 4))
        planes.append(np.ascontiguousarray(v.view(np.uint8).reshape(-1, 4)[:, 0]))
    xd0 = np.stack([np.concatenate([planes[(4 * i + q) % 16] for q in range(4)]) for i in range(NBUF)])
    return {"raw_int32": raw, "xdelta_plane0": xd0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    orc = Oracle()
    # device-copy rate: bytes read + bytes written per second of a 1 GiB device-to-device copy
    x = torch.empty(NBUF * SIZE, dtype=torch.uint8, device="cuda")
    y = torch.empty_like(x)
    copy_ms = timed(lambda: y.copy_(x), 5)
    copy_rate = 2 * x.numel() / (copy_ms * 1e-3)
    del x, y
    runs = []
    for cname, host in contents(orc).items():
        d_src = torch.from_numpy(host).cuda()
        want = {i: orc.hzr_encode(host[i]) for i in CHECKED}
        rec = dict(content=cname, buffers=NBUF, buffer_bytes=SIZE)
        for side in ("bytes", "emulation"):
            pk = api.new_bytes(SIZE) if side == "bytes" else api.new_hzr(1, 1, SIZE)
            pk.reserve(NBUF)
            stride = (pk.max_compressed_size + 255) // 256 * 256
            d_dst = torch.empty((NBUF, stride), dtype=torch.uint8, device="cuda")
            d_sizes = torch.empty(NBUF, dtype=torch.int64, device="cuda")
            d_out = torch.empty((NBUF, SIZE), dtype=torch.uint8, device="cuda")
            d_used = torch.empty(NBUF, dtype=torch.int64, device="cuda")
            c_ms = timed(lambda: pk.compress_batch(d_src, d_dst=d_dst, d_sizes=d_sizes, dst_stride=stride), a.iters)
            d_ms = timed(lambda: pk.decompress_batch(d_dst, NBUF, stride, d_out=d_out, d_consumed=d_used), a.iters)
            # ---- behind the timed region: the streams and the decode ----
            sizes = d_sizes.cpu().numpy()
            ok = bool((d_used.cpu().numpy() == sizes).all()) and bool(torch.equal(d_out, d_src))
            for i in CHECKED:
                s = d_dst[i, : int(sizes[i])].cpu().numpy().tobytes()
                if side == "emulation":  # [method 0][u32 len of plane 0][plane 0 = hzr_encode of the buffer] ...
                    s = s[5 : 5 + struct.unpack_from("<I", s, 1)[0]]
                ok = ok and s == want[i]
            r = dict(compress_ms=round(c_ms, 3), decompress_ms=round(d_ms, 3), compress_gbytes_per_s=round(NBUF * SIZE / (c_ms * 1e-3) / 1e9, 2),
                     decompress_gbytes_per_s=round(NBUF * SIZE / (d_ms * 1e-3) / 1e9, 2), stream_bytes=int(sizes.sum()), checked_ok=ok)
            if side == "bytes":
                pk.set_profiling(True)
                ing = []
                for _ in range(a.iters):
                    pk.compress_batch(d_src, d_dst=d_dst, d_sizes=d_sizes, dst_stride=stride)
                    torch.cuda.synchronize()
                    ing.append(pk.stage_times()["preprocess"])
                pk.set_profiling(False)
                nz = int((host != 0).any(axis=1).sum())  # (every line of these contents holds a non-zero byte: all of it is written)
                floor_ms = 2 * NBUF * SIZE / copy_rate * 1e3
                r["ingest"] = dict(ms=round(float(np.median(ing)), 3), bytes_read=NBUF * SIZE, bytes_written=NBUF * SIZE, floor_ms=round(floor_ms, 3),
                                   nonzero_buffers=nz)
            rec[side] = r
            print(json.dumps({cname: {side: r}}), file=sys.stderr, flush=True)
            pk.close()
            del d_dst, d_out
        rec["bytes_faster"] = dict(compress=rec["bytes"]["compress_ms"] < rec["emulation"]["compress_ms"],
                                   decompress=rec["bytes"]["decompress_ms"] < rec["emulation"]["decompress_ms"])
        runs.append(rec)
        del d_src
    line = json.dumps(dict(tool="hzr_bytes_rate", device=torch.cuda.get_device_name(0), iters=a.iters, device_copy_gbytes_per_s=round(copy_rate / 1e9, 1),
                           runs=runs))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0 if all(r["bytes"]["checked_ok"] and r["emulation"]["checked_ok"] for r in runs) else 1)


if __name__ == "__main__":
    main()
