#!/usr/bin/env python3
"""Time the zero-phase offline R-peak detector (rspt_hip_peak_detect_offline_batch_dev) and print one JSON line.

Runs at fs = 2000: 64 x (64 ch x 65536 int32) fresh and stateful, with and without traces; 1024 x (12 ch x 8192 int32) fresh;
and, on the large batch, OFFLINE_FW (detect_fw) fresh without traces beside it, timed in the same process.  Per run: ms per call
(device events around back-to-back calls; the workspace is allocated once, outside the timed calls), GSamples/s, and the bytes
the workspace passes move.  From the device assembly (hipcc -S) of k_peak_offline<4, false>: the instruction count of every
innermost loop in program order, and per sample for the chunked passes (a loop's count over its chunk).  After the timed region
the events of blocks 0 and B-1 of a fresh call are checked against the restatement (tests/peak_offline_cases.py).

    python tools/peak_offline_rate.py [--iters N] [--out FILE] [--no-asm]
"""
import argparse
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import devasm  # noqa: E402
import peak_offline_cases as oc  # noqa: E402
import peak_cases as pc  # noqa: E402
from rspt_amd import api, synth  # noqa: E402

# the chunked passes of peak_offline_block in program order, with their chunk lengths (peak.hip)
PASSES = [("asc baseline fw + band-pass fw", 16), ("desc baseline bw + band-pass bw", 8), ("asc integrator fw", 16), ("desc integrator bw", 16),
          ("asc threshold fw", 16), ("desc threshold bw", 16), ("asc state machine", 8), ("asc events", 16)]
WS_BYTES_PER_SAMPLE = 4 + 8 + (4 + 8 + 8 + 8) + 16 + 16 + 8 + 16 + 24 + 8  # x and workspace loads / stores of the passes above


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


def innermost_loops():
    """instruction counts of the innermost loops of k_peak_offline<4, false>, in program order (tests/devasm.py)"""
    return next((devasm.innermost_loops(body) for name, body in devasm.functions().items() if re.match(r"^_Z\w*14k_peak_offlineILi4ELb0E", name)), [])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-asm", action="store_true")
    a = ap.parse_args()
    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    loops = None if a.no_asm else innermost_loops()
    res = []
    fs = 2000.0
    for name, nch, ns, nblocks, modes in (("64x(64ch x 65536 i32)", 64, 65536, 64, ("fresh", "stateful")), ("1024x(12ch x 8192 i32)", 12, 8192, 1024, ("fresh",))):
        pk = api.new_hzr(4, nch, ns)
        blocks = [synth.synth_native(nch, ns, b % 4, bps=4, ecg=True).numpy() for b in range(4)]
        src = torch.from_numpy(np.stack([blocks[b % 4] for b in range(nblocks)])).cuda()
        if nblocks == 64:
            ms = timed(lambda: pk.peak_detect_batch(src, variant="offline_fw", sampling_rate=fs, max_peaks=128), a.iters)
            res.append(dict(shape=name, entry="offline_fw (detect_fw)", mode="fresh", traces=False, ms=round(ms, 3)))
            print(json.dumps(res[-1]), file=sys.stderr, flush=True)
        for traces in (False, True):
            for mode in modes:
                if traces and nblocks == 1024:
                    continue
                st = pk.peak_state() if mode == "stateful" else None
                L = api.lib()
                wb = pk.peak_offline_work_bytes(nblocks, mode == "stateful")
                work = torch.empty(wb // 8 + 1, dtype=torch.float64, device="cuda")
                count = torch.empty((nblocks, nch), dtype=torch.int32, device="cuda")
                index = torch.empty((nblocks, nch, 128), dtype=torch.int32, device="cuda")
                value = torch.empty((nblocks, nch, 128), dtype=torch.float64, device="cuda")
                sig = torch.empty((nblocks, ns, nch), dtype=torch.float64, device="cuda") if traces else None
                thr = torch.empty_like(sig) if traces else None
                stream = torch.cuda.current_stream().cuda_stream

                def call():
                    rc = L.rspt_hip_peak_detect_offline_batch_dev(pk._h, src.data_ptr(), nblocks, fs, 1.0, st.data_ptr() if st is not None else None,
                                                                  work.data_ptr(), count.data_ptr(), index.data_ptr(), value.data_ptr(), 128,
                                                                  sig.data_ptr() if traces else None, thr.data_ptr() if traces else None, stream)
                    assert rc == 0, rc

                ms = timed(call, a.iters)
                check = None
                if mode == "fresh" and not traces:
                    if st is None:
                        call()
                    torch.cuda.synchronize()
                    check = True
                    for b in (0, nblocks - 1):
                        want = oc.detect(pc.native_to_i32(blocks[b % 4], 4, nch, ns)[None], fs)
                        cnt = count[b].cpu().numpy()
                        check &= cnt.tolist() == want["count"][0] and all(
                            index[b, c, : cnt[c]].cpu().numpy().tolist() == want["index"][0][c][:128] for c in range(nch))
                samples = nblocks * nch * ns
                res.append(dict(shape=name, entry="offline (detect)", mode=mode, traces=traces, ms=round(ms, 3),
                                gsamples_per_s=round(samples / (ms * 1e-3) / 1e9, 3), lanes=nch if mode == "stateful" else nblocks * nch,
                                work_bytes=wb, pass_bytes=samples * WS_BYTES_PER_SAMPLE, checked_blocks_ok=check))
                print(json.dumps(res[-1]), file=sys.stderr, flush=True)
                del work, sig, thr
        pk.close()
    asm = None
    if loops is not None:
        asm = dict(innermost_loops=loops)
    line = json.dumps(dict(tool="peak_offline_rate", device=torch.cuda.get_device_name(0), iters=a.iters, passes=[p for p, _ in PASSES], asm=asm, runs=res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
