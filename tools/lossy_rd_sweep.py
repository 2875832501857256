#!/usr/bin/env python3
"""The size / distortion ladder of a lossy packer: for every setting of a ladder one JSON line with the compression ratio and
PRDN[%] of SignalPacker.roundtrip_quality (compress -> decompress -> PRDN on the device) under that setting
(SignalPacker.set_quantizer; rspt_hip.h: rspt_hip_set_quantizer).

    quality   dct: larger is COARSER (the reference's constant is 128); hadamard: larger is FINER (the reference's is 1)
    nb        the low bytes of every stored value that reach the stream (dct 2, hadamard 3); values beyond them are cut, as in
              the reference -- a fine quality with a small nb shows as a PRDN that jumps up, not as an error

    python tools/lossy_rd_sweep.py --packer dct|hadamard [--qualities 512,128,32] [--nb 2,3] [--blocks 4 --nch 12 --ns 8192 --bps 4]
                                   [--out FILE (appended to)]
The input is the ECG-like synthetic batch (synth.synth_batch_native(..., ecg=True)); figures are means over its blocks.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LADDERS = {"dct": ([1024.0, 512.0, 256.0, 128.0, 64.0, 32.0, 16.0, 8.0, 4.0], [2, 3]),
           "hadamard": ([1 / 64, 1 / 16, 0.25, 0.5, 1.0, 2.0, 4.0, 16.0, 64.0], [2, 3])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--packer", required=True, choices=sorted(LADDERS))
    ap.add_argument("--qualities", default=None, help="comma-separated; default: a ladder around the reference's constant")
    ap.add_argument("--nb", default=None, help="comma-separated plane counts 1..4")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--nch", type=int, default=12)
    ap.add_argument("--ns", type=int, default=8192)
    ap.add_argument("--bps", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from rspt_amd import api, synth

    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: there is no CPU path"
    qualities = [float(v) for v in a.qualities.split(",")] if a.qualities else LADDERS[a.packer][0]
    nbs = [int(v) for v in a.nb.split(",")] if a.nb else LADDERS[a.packer][1]
    x = synth.synth_batch_native(a.blocks, a.nch, a.ns, bps=a.bps, ecg=True, device="cuda")
    pk = api.SignalPacker(a.packer, a.bps, a.nch, a.ns, 3)
    q0, nb0 = pk.quantizer()
    lines = []
    for nb in nbs:
        for q in qualities:
            pk.set_quantizer(q, nb)
            prdn, cr = pk.roundtrip_quality(x)
            torch.cuda.synchronize()
            lines.append(dict(tool="lossy_rd_sweep", packer=a.packer, quality=q, nb=nb, reference_constants=(q, nb) == (q0, nb0),
                              shape="%dx(%dch x %d i%d)" % (a.blocks, a.nch, a.ns, 8 * a.bps), cr=round(float(cr.mean()), 3),
                              prdn=round(float(prdn.mean()), 4)))
    pk.close()
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
