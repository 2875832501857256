#!/usr/bin/env python3
"""Time the two converter stages (rspt_hip_native_to_i32_batch_dev / rspt_hip_i32_to_native_batch_dev) on
device-resident batches, and batched decompress of the wide shape; one JSON line per figure.

    shapes   64 x (64 ch x 65536) int32 and int24, 1024 x (12 ch x 8192) int32, 8 x (16384 ch x 4096) int32 (a wide handle)
    floor    every figure beside its byte floor: bytes read + bytes written at the device-copy rate measured in the same process
             (a copy of N bytes moves 2 N), the yardstick of profiles/peak_rate.json and the PRDN figures
    method   warm-up, then `iters` back-to-back calls between two events on one stream
Both outputs are checked after the timed region: the round trip gives back the input.

    python tools/convert_bench.py [--iters 20] [--out profiles/convert_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(64, 4, 64, 65536), (64, 3, 64, 65536), (1024, 4, 12, 8192), (8, 4, 16384, 4096)]  # nblocks, bps, nch, ns


def timed(fn, iters, warmup=3):
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from rspt_amd import api, synth

    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    lines = []
    # the device-copy rate: 256 MiB, read once and written once
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), a.iters)
    rate = 2 * src.numel() / (copy_ms * 1e-3)  # bytes per second
    lines.append(dict(tool="convert_bench", what="device_copy", bytes=src.numel(), ms=round(copy_ms, 4), tb_per_s=round(rate / 1e12, 3),
                      device=torch.cuda.get_device_name(0)))
    del src, dst
    for nb, bps, nch, ns in SHAPES:
        pk = api.new_hzr(bps, nch, ns)
        x = synth.synth_batch_native(nb, nch, ns, bps=bps, device="cuda")
        x = x.reshape(nb, -1).contiguous()
        planar = torch.empty((nb, nch, ns), dtype=torch.int32, device="cuda")
        back = torch.empty_like(x)
        nat_bytes, pl_bytes = x.numel(), 4 * planar.numel()
        floor = (nat_bytes + pl_bytes) / rate * 1e3
        shape = "%dx(%dch x %d i%d)" % (nb, nch, ns, 8 * bps)
        for what, fn in (("native_to_i32", lambda: pk.to_planar_i32(x, d_out=planar)), ("i32_to_native", lambda: pk.from_planar_i32(planar, d_out=back))):
            ms = timed(fn, a.iters)
            lines.append(dict(tool="convert_bench", what=what, shape=shape, bytes_moved=nat_bytes + pl_bytes, ms=round(ms, 4), floor_ms=round(floor, 4),
                              x_floor=round(ms / floor, 2), gsamples_per_s=round(nb * nch * ns / (ms * 1e-3) / 1e9, 2)))
        torch.cuda.synchronize()
        lines[-1]["round_trip_ok"] = lines[-2]["round_trip_ok"] = bool(torch.equal(back, x))
        if nch > 8192:  # batched decompress of the wide shape
            d_dst, d_sizes = pk.compress_batch(x)
            d_out, d_used = pk.decompress_batch(d_dst, nb, d_dst.shape[1])
            ms = timed(lambda: pk.decompress_batch(d_dst, nb, d_dst.shape[1], d_out=d_out, d_consumed=d_used), max(3, a.iters // 4))
            torch.cuda.synchronize()
            lines.append(dict(tool="convert_bench", what="decompress_batch", shape=shape, ms=round(ms, 4), lossless_ok=bool(torch.equal(d_out, x)),
                              gsamples_per_s=round(nb * nch * ns / (ms * 1e-3) / 1e9, 2)))
        pk.close()
        del x, planar, back
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
