#!/usr/bin/env python3
"""Time the lossy packers at the reference's quantiser constants and at other settings (rspt_hip_set_quantizer),
on a device-resident batch; one JSON line per figure.

    shape      16 x (64 ch x 65536) int32, ECG-like synthetic (synth.synth_batch_native)
    settings   hadamard: the default (quality 1), quality 2, quality 3 -- anything but 1 takes the kernels with an fp64 division
               per coefficient (transforms.hip: k_fwht64k_q); dct: the default (quality 128) and quality 8 with nb = 3 (two
               planes would cut its coefficients) -- the same kernels with other scalars
    figures    compress_batch and decompress_batch, best of `rounds` rounds and every round (the spread), each round `iters`
               back-to-back calls (dct: iters / 4) between two events on one stream (tools/convert_bench.py); per non-default
               setting the ratio to the default of the same run; `iters` is in every line
    --parent   an older build of the library (loaded beside this one, bind(missing_ok=True)): the default settings are then
               timed on BOTH libraries, alternating within every round of this one process -- the default kernels are the
               parent's instruction for instruction (tools/isa_diff.py), so a difference beyond the spread is a finding

    python tools/lossy_quantizer_bench.py [--iters 20] [--rounds 5] [--parent old/librspt_hip.so] [--out profiles/lossy_quantizer_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from convert_bench import timed  # noqa: E402

NBLOCKS, BPS, NCH, NS = 16, 4, 64, 65536
SETTINGS = {"hadamard": [None, (2.0, 3), (3.0, 3)], "dct": [None, (8.0, 3)]}  # (quality, nb); None: the reference's constants


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from rspt_amd import api, synth

    this = api.lib()
    assert this.rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    parent = api.bind(C.CDLL(os.path.abspath(a.parent)), missing_ok=True) if a.parent else None
    x = synth.synth_batch_native(NBLOCKS, NCH, NS, bps=BPS, ecg=True, device="cuda").reshape(NBLOCKS, -1).contiguous()
    shape = "%dx(%dch x %d i%d)" % (NBLOCKS, NCH, NS, 8 * BPS)
    lines = []
    for kind, ladder in SETTINGS.items():
        iters = a.iters if kind != "dct" else max(3, a.iters // 4)
        runs = []  # (label, lib name, packer)
        for setting in ladder:
            pk = api.SignalPacker(kind, BPS, NCH, NS, 3)
            if setting is not None:
                pk.set_quantizer(*setting)
            runs.append(("default" if setting is None else "quality %g nb %d" % setting, "this", pk))
        if parent is not None:
            runs.insert(0, ("default", "parent", api.SignalPacker(kind, BPS, NCH, NS, 3, library=parent)))
        stride = (max(pk.max_compressed_size for _, _, pk in runs) + 255) // 256 * 256
        d_dst = {i: torch.empty((NBLOCKS, stride), dtype=torch.uint8, device="cuda") for i in range(len(runs))}
        d_sizes = torch.empty(NBLOCKS, dtype=torch.int64, device="cuda")
        back = torch.empty_like(x)
        used = torch.empty(NBLOCKS, dtype=torch.int64, device="cuda")
        t = {}
        for r in range(a.rounds):
            for i, (label, lib, pk) in enumerate(runs):
                t.setdefault((i, "compress"), []).append(timed(lambda: pk.compress_batch(x, d_dst[i], d_sizes, stride), iters))
                t.setdefault((i, "decompress"), []).append(timed(lambda: pk.decompress_batch(d_dst[i], NBLOCKS, stride, back, used), iters))
        # behind the timed region: what the setting buys (PRDN, CR), and that the two builds write the same default streams
        base = {}
        for i, (label, lib, pk) in enumerate(runs):
            prdn, cr = pk.roundtrip_quality(x)
            s_dst, s_sizes = pk.compress_batch(x)
            torch.cuda.synchronize()
            digest = (int(s_sizes.sum()), int(s_dst[0, : int(s_sizes[0])].to(torch.int64).sum()))
            q, nb = pk.quantizer() if lib == "this" else (None, None)
            for what in ("compress", "decompress"):
                v = t[i, what]
                e = dict(tool="lossy_quantizer_bench", lib=lib, packer=kind, setting=label, quality=q, nb=nb, what=what, shape=shape, iters=iters,
                         ms=round(min(v), 4), ms_rounds=[round(u, 4) for u in v], gsamples_per_s=round(NBLOCKS * NCH * NS / (min(v) * 1e-3) / 1e9, 2),
                         prdn=round(float(prdn.mean()), 4), cr=round(float(cr.mean()), 3), stream_digest=digest)
                if label == "default":
                    base[lib, what] = min(v)
                else:
                    e["ratio_to_default"] = round(min(v) / base["this", what], 3)
                lines.append(e)
        if parent is not None:
            for what in ("compress", "decompress"):
                lines.append(dict(tool="lossy_quantizer_bench", packer=kind, what=what, setting="default", this_over_parent=round(
                    base["this", what] / base["parent", what], 4)))
        for _, _, pk in runs:
            pk.close()
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
