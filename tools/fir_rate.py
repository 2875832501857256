#!/usr/bin/env python3
"""Time the FIR pre-filter stage (rspt_hip_fir_prefilter_batch_dev) and print one JSON line.

Runs: K in {1, 5, 31, 101, 255, 1001} on 64 x (64 ch x 65536 int32) and on 1024 x (3 ch x 20000 int24), in place and out of
place.  Per run: ms per call (device events around back-to-back calls), GSamples/s, and two floors measured in the same
process:
  copy_frac   a device copy of the batch (torch copy_, read + write of every byte) over the call's time: the floor at small K
  valu_frac   outputs x K x (one v_mul_f64 + one v_add_f64) at the rate tools/fir_floor.hip measures, over the call's time:
              the floor at large K
After the timed region blocks 0 and B-1 of a fresh call are checked against the restatement (tests/fir_cases.py).

    python tools/fir_rate.py [--iters N] [--ks 1,5,...] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fir_cases as fc  # noqa: E402
from rspt_amd import api, synth  # noqa: E402

FLOOR_SRC = os.path.join(ROOT, "tools", "fir_floor.hip")
FLOOR_SO = os.path.join(ROOT, "tools", "fir_floor.so")


def floor_lib():
    if not os.path.exists(FLOOR_SO) or os.path.getmtime(FLOOR_SO) < os.path.getmtime(FLOOR_SRC):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-o", FLOOR_SO, FLOOR_SRC])
    L = C.CDLL(FLOOR_SO)
    L.fir_floor_launch.restype = C.c_int
    L.fir_floor_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return L


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


def f64_rate():
    """f64 operations per second (one mul or one add each) of k_fir_floor over the whole device"""
    L = floor_lib()
    st = torch.cuda.current_stream().cuda_stream
    grid, it = 256 * 8, 4096
    out = torch.empty(grid * 256, dtype=torch.float64, device="cuda")
    coef = torch.linspace(0.5, 1.5, 16, dtype=torch.float64, device="cuda")
    ms = timed(lambda: L.fir_floor_launch(out.data_ptr(), coef.data_ptr(), grid, it, st), 10)
    return grid * 256 * it * 16 * 2 / (ms * 1e-3)


def shape_runs(name, bps, nch, ns, nblocks, block_fn, ks, iters, rate, res):
    pk = api.new_hzr(bps, nch, ns)
    host = np.stack([block_fn(b) for b in range(nblocks)])
    pristine = torch.from_numpy(host).cuda()
    src = pristine.clone()
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), iters)
    samples = nblocks * nch * ns
    for K in ks:
        k = fc.windowed_sinc_lowpass(K, 0.05)
        for in_place in (False, True):
            call = (lambda: pk.fir_prefilter_batch(src, k)) if in_place else (lambda: pk.fir_prefilter_batch(src, k, d_dst=dst))
            ms = timed(call, iters)
            src.copy_(pristine)
            out = pk.fir_prefilter_batch(src, k, d_dst=None if in_place else dst)
            torch.cuda.synchronize()
            bb = bps * nch * ns
            ok = all(np.array_equal(out[b].cpu().numpy(), fc.fir_prefilter(host[b], bps, nch, ns, k)) for b in (0, nblocks - 1))
            src.copy_(pristine)
            valu_ms = samples * K * 2 / rate * 1e3
            res.append(dict(shape=name, K=K, in_place=in_place, ms=round(ms, 4), gsamples_per_s=round(samples / (ms * 1e-3) / 1e9, 2),
                            copy_ms=round(copy_ms, 4), copy_frac=round(copy_ms / ms, 3), valu_floor_ms=round(valu_ms, 4),
                            valu_frac=round(valu_ms / ms, 3), checked_blocks_ok=bool(ok), bytes=nblocks * bb))
            print(json.dumps(res[-1]), file=sys.stderr, flush=True)
    pk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--ks", default="1,5,31,101,255,1001")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    ks = [int(v) for v in a.ks.split(",")]
    rate = f64_rate()
    res = []
    shape_runs("64x(64ch x 65536 i32)", 4, 64, 65536, 64, lambda b: synth.synth_native(64, 65536, b, bps=4, ecg=True).numpy(), ks, a.iters, rate, res)
    ds = np.frombuffer(synth.data_stream_3ch_i24(), dtype=np.uint8)
    shape_runs("1024x(3ch x 20000 i24)", 3, 3, 20000, 1024, lambda b: ds, ks, a.iters, rate, res)
    line = json.dumps(dict(tool="fir_rate", device=torch.cuda.get_device_name(0), f64_ops_per_s=rate, iters=a.iters, runs=res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
