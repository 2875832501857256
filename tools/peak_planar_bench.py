#!/usr/bin/env python3
"""Time the planar R-peak entries (rspt_hip_peak_detect_planar_batch_dev, rspt_hip_peak_detect_offline_planar_batch_dev;
DESIGN.md 4e) against what a caller with planar samples had to do before them, on device-resident batches; one JSON line per
figure.

    detectors    ONLINE (variant 0) and the zero-phase offline detector, 2 kHz, fresh detectors, no traces, max_peaks 64
    figures      (a) the planar entry
                 (b) from_planar_i32 + the native entry: the route a planar caller had -- the yardstick
                 (c) the native entry alone
    shapes       64 x (64 ch x 65536) and 1024 x (12 ch x 8192), int32
    method       warm-up, then `iters` back-to-back calls between two events on one stream (tools/convert_bench.py); the three
                 figures interleaved, `rounds` times in this one process; per figure the median and max - min over the rounds.
                 Every route writes into the same output buffers and, offline, uses the same workspace.
Behind the timed regions the planar entry's counts, indices and values are compared with route (b)'s (events: how many there
were; the offline detector finds none in the four seconds of the short shape).
The entries earn their place if (a) <= (b), the margin being the spread of the rounds; (a) - (c), the planar kernel against the
native one, is reported and not gated.

    python tools/peak_planar_bench.py [--iters 10] [--rounds 7] [--out profiles/peak_planar_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from convert_bench import timed  # noqa: E402

SHAPES = [(64, 64, 65536), (1024, 12, 8192)]  # nblocks, nch, ns (int32)
FS, MAX_PEAKS = 2000.0, 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from rspt_amd import api, synth

    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    lines = []
    for nb, nch, ns in SHAPES:
        shape = "%dx(%dch x %d i32)" % (nb, nch, ns)
        x = synth.synth_batch_native(nb, nch, ns, bps=4, device="cuda").reshape(nb, -1).contiguous()
        pk = api.new_hzr(4, nch, ns)
        P = pk.to_planar_i32(x)
        tmp = torch.empty_like(x)
        st = torch.cuda.current_stream().cuda_stream
        count = torch.zeros((nb, nch), dtype=torch.int32, device="cuda")
        index = torch.zeros((nb, nch, MAX_PEAKS), dtype=torch.int32, device="cuda")
        value = torch.zeros((nb, nch, MAX_PEAKS), dtype=torch.float64, device="cuda")
        work = torch.empty(pk.peak_offline_work_bytes(nb) // 8, dtype=torch.float64, device="cuda")
        outs = (count.data_ptr(), index.data_ptr(), value.data_ptr(), MAX_PEAKS, None, None, st)

        def online(entry, src):
            pk._call(entry, src.data_ptr(), nb, 0, FS, -1.0, None, *outs)

        def offline(entry, src):
            pk._call(entry, src.data_ptr(), nb, FS, -1.0, None, work.data_ptr(), *outs)

        def converted(run, entry):
            pk.from_planar_i32(P, d_out=tmp)
            run(entry, tmp)

        for det, run, native, planar in (("online", online, "rspt_hip_peak_detect_batch_dev", "rspt_hip_peak_detect_planar_batch_dev"),
                                         ("offline", offline, "rspt_hip_peak_detect_offline_batch_dev", "rspt_hip_peak_detect_offline_planar_batch_dev")):
            routes = {
                "planar": lambda: run(planar, P),
                "convert+native": lambda: converted(run, native),
                "native": lambda: run(native, x),
            }
            t = {what: [] for what in routes}
            for r in range(a.rounds):
                for what, fn in routes.items():
                    t[what].append(timed(fn, a.iters))
            # behind the timed regions: one call of the yardstick and one of the planar entry, compared
            res = []
            for what in ("convert+native", "planar"):
                for o in (count, index, value):
                    o.zero_()
                routes[what]()
                torch.cuda.synchronize()
                res.append((count.clone(), index.clone(), value.clone()))
            same = all(bool(torch.equal(p, q)) for p, q in zip(*res))
            for what, v in t.items():
                lines.append(dict(tool="peak_planar_bench", detector=det, what=what, shape=shape, fs=FS, traces=False, max_peaks=MAX_PEAKS, iters=a.iters,
                                  ms_median=round(statistics.median(v), 4), ms_spread=round(max(v) - min(v), 4), ms_rounds=[round(q, 4) for q in v],
                                  planar_equals_native_route=same, events=int(res[0][0].sum())))
        pk.close()
        del x, P, tmp, work, count, index, value
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
