#!/usr/bin/env python3
"""Time the R-peak detector stage (rspt_hip_peak_detect_batch_dev) and print one JSON line.

Runs: 64 x (64 ch x 65536 int32) at fs = 2000, each variant, with and without traces, fresh and stateful; 1024 x (12 ch x 8192
int32) fresh, each variant.  Per run: ms per call (device events around back-to-back calls), GSamples/s, and the serial-instruction
floor of the busiest wave: its steps (samples per lane, plus the band-pass history calls) times the instructions it issues per
step times 2.2 ns (the issue interval of a lone wave, profiles/r03_issue_rate.txt).  Instructions per sample: the main chunk
loop of the k_peak instance in the device assembly (hipcc -S), divided by its 16 samples; per history call: the history loop.
After the timed region the events of blocks 0 and B-1 of a fresh call are checked against the restatement (tests/peak_cases.py).

    python tools/peak_rate.py [--iters N] [--out FILE] [--no-asm]
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
import peak_cases as pc  # noqa: E402
from rspt_amd import api, synth  # noqa: E402

ISSUE_NS = 2.2
CH = 16  # samples of the chunk loop in peak.hip


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


def loop_sizes():
    """{(bps, variant, traces): (instructions of the largest innermost loop / CH, instructions of the smallest)} per k_peak
    instance (tests/devasm.py: innermost_loops)"""
    out = {}
    for name, body in devasm.functions().items():
        m = re.match(r"^_Z\w*6k_peakILi(\d)ELi(\d)ELb(\d)E", name)
        loops = devasm.innermost_loops(body) if m else None
        if loops:
            out[(int(m.group(1)), int(m.group(2)), bool(int(m.group(3))))] = (max(loops) / CH, min(loops))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-asm", action="store_true")
    a = ap.parse_args()
    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    sizes = {} if a.no_asm else loop_sizes()
    res = []
    fs = 2000.0
    for name, nch, ns, nblocks, modes in (("64x(64ch x 65536 i32)", 64, 65536, 64, ("fresh", "stateful")), ("1024x(12ch x 8192 i32)", 12, 8192, 1024, ("fresh",))):
        pk = api.new_hzr(4, nch, ns)
        blocks = [synth.synth_native(nch, ns, b % 4, bps=4, ecg=True).numpy() for b in range(4)]
        src = torch.from_numpy(np.stack([blocks[b % 4] for b in range(nblocks)])).cuda()
        for vname, v in pc.VARIANTS.items():
            k = pc.detector_constants(v, fs)
            for traces in (False, True):
                for mode in modes:
                    if traces and nblocks * ns * nch * 16 > (8 << 30):
                        continue
                    st = pk.peak_state() if mode == "stateful" else None
                    call = lambda: pk.peak_detect_batch(src, variant=vname, sampling_rate=fs, max_peaks=128, state=st, traces=traces)  # noqa: E731
                    ms = timed(call, a.iters)
                    # steps of the busiest lane: its samples, and the band-pass history calls (once per detector; OFFLINE_FW per block)
                    nb_lane = nblocks if mode == "stateful" else 1
                    hist = k["hist"] * (nb_lane if v == pc.OFFLINE_FW else 1)
                    steps = nb_lane * ns
                    per_sample, per_hist = sizes.get((4, v, traces), (None, None))
                    floor = (steps * per_sample + hist * per_hist) * ISSUE_NS * 1e-6 if per_sample else None
                    check = None
                    if mode == "fresh" and not traces:
                        count, index, _ = pk.peak_detect_batch(src, variant=vname, sampling_rate=fs, max_peaks=128)
                        torch.cuda.synchronize()
                        check = True
                        for b in (0, nblocks - 1):
                            x = pc.native_to_i32(blocks[b % 4], 4, nch, ns)[None]
                            want = pc.detect(x, v, fs)
                            cnt = count[b].cpu().numpy()
                            check &= cnt.tolist() == want["count"][0] and all(
                                index[b, c, : cnt[c]].cpu().numpy().tolist() == want["index"][0][c][:128] for c in range(nch))
                    res.append(dict(shape=name, variant=vname, mode=mode, traces=traces, ms=round(ms, 3),
                                    gsamples_per_s=round(nblocks * nch * ns / (ms * 1e-3) / 1e9, 3), lanes=nch if mode == "stateful" else nblocks * nch,
                                    busiest_wave_steps=steps + hist, instr_per_sample=per_sample, instr_per_history_call=per_hist,
                                    floor_ms=round(floor, 3) if floor else None, x_floor=round(ms / floor, 2) if floor else None,
                                    checked_blocks_ok=check))
                    print(json.dumps(res[-1]), file=sys.stderr, flush=True)
        pk.close()
    line = json.dumps(dict(tool="peak_rate", device=torch.cuda.get_device_name(0), iters=a.iters, issue_ns=ISSUE_NS, runs=res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
