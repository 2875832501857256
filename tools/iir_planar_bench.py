#!/usr/bin/env python3
"""Time the planar IIR entries (rspt_hip_iir_prefilter_planar_*_dev, rspt_hip_iir_cascade_planar_*_dev) against
what a caller with planar samples had to do before them, on device-resident batches; one JSON line per figure.

    stages       the harness's band-pass through the IIR pre-filter, per channel; the README pair (HP 0.4 Hz, LP 100 Hz) through
                 the cascade
    figures      (a) the native entry, (b) from_planar_i32 + native entry + to_planar_i32, (c) the planar entry;
                 and the stream forms on one block of 64 ch x 65536 per call, native against planar
    shapes       64 x (64 ch x 65536) and 1024 x (12 ch x 8192), int32
    --parent     an older build of the library without the planar IIR entries (loaded beside this one, bind(missing_ok=True)):
                 (a) and (b) are then timed on that library, (c) on this one, alternating `rounds` times in this one process
    method       warm-up, then `iters` back-to-back calls between two events on one stream (tools/convert_bench.py); per figure
                 the median and max - min over the rounds.  The calls filter in place, so every timed region starts from a fresh
                 copy of the input and the samples of later calls are those the earlier ones left (the kernels' time does not depend
                 on the values short of full-scale overshoot).
Behind the timed region the planar entry's output on the input is compared with from_planar_i32 + native entry + to_planar_i32.

    python tools/iir_planar_bench.py [--iters 20] [--rounds 3] [--parent old/librspt_hip.so] [--out profiles/iir_planar_bench.json]
                                     [--form lane_sample] [--append]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from convert_bench import timed  # noqa: E402

SHAPES = [(64, 64, 65536), (1024, 12, 8192)]  # nblocks, nch, ns (int32)
STREAM_SHAPE = (64, 65536)  # one block per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--form", default=None, help="a name for this build's planar kernels, written into every line (DESIGN.md 4b: a second form of k_iir_pipe_planar was timed and taken out; its lines are in profiles/iir_planar_bench.json)")
    ap.add_argument("--append", action="store_true", help="add the lines to --out instead of replacing it")
    a = ap.parse_args()
    import torch

    import cases
    import iir_cascade_cases as icc
    from rspt_amd import api, synth

    this = api.lib()
    assert this.rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    base = ("parent", api.bind(C.CDLL(os.path.abspath(a.parent)), missing_ok=True)) if a.parent else ("this", this)
    bn, bd = cases.IIR_BANDPASS
    stages = {
        "prefilter_bandpass_per_channel": (lambda q, buf, st=None: q.iir_prefilter_batch(buf, bn, bd, init_nr_samples=2000, per_channel=True, state=st),
                                           lambda q, P, st=None: q.iir_prefilter_planar_batch(P, bn, bd, init_nr_samples=2000, per_channel=True, state=st),
                                           lambda q: q.iir_state()),
        "cascade_readme_pair": (lambda q, buf, st=None: q.iir_cascade_batch(buf, icc.README_PAIR, state=st),
                                lambda q, P, st=None: q.iir_cascade_planar_batch(P, icc.README_PAIR, state=st),
                                lambda q: q.iir_cascade_state(2)),
    }
    lines = []

    def figure(what, stage, shape, lib, v, **kw):
        if a.form:
            kw["form"] = a.form
        lines.append(dict(tool="iir_planar_bench", stage=stage, what=what, shape=shape, lib=lib, ms_median=round(statistics.median(v), 4),
                          ms_spread=round(max(v) - min(v), 4), ms_rounds=[round(x, 4) for x in v], **kw))

    for nb, nch, ns in SHAPES:
        shape = "%dx(%dch x %d i32)" % (nb, nch, ns)
        x0 = synth.synth_batch_native(nb, nch, ns, bps=4, device="cuda").reshape(nb, -1).contiguous()
        old, new = api.SignalPacker("hzr", 4, nch, ns, 4, library=base[1]), api.SignalPacker("hzr", 4, nch, ns, 4, library=this)
        P0 = new.to_planar_i32(x0)
        x, P, tmp = torch.empty_like(x0), torch.empty_like(P0), torch.empty_like(x0)
        for stage, (native, planar, _) in stages.items():
            t = {"native": [], "convert+native+convert": [], "planar": []}

            def route_b():
                old.from_planar_i32(P, d_out=tmp)
                native(old, tmp)
                old.to_planar_i32(tmp, d_out=P)

            for r in range(a.rounds):
                x.copy_(x0)
                t["native"].append(timed(lambda: native(old, x), a.iters))
                P.copy_(P0)
                t["convert+native+convert"].append(timed(route_b, a.iters))
                P.copy_(P0)
                t["planar"].append(timed(lambda: planar(new, P), a.iters))
            # behind the timed region: one call of each route on the input
            P.copy_(P0)
            route_b()
            want = P.clone()
            P.copy_(P0)
            planar(new, P)
            torch.cuda.synchronize()
            same = bool(torch.equal(P, want))
            for what, v in t.items():
                figure(what, stage, shape, "this" if what == "planar" else base[0], v, planar_equals_native_route=same)
        old.close()
        new.close()
        del x0, P0, x, P, tmp
    # the stream forms: one block per call on a carried state
    nch, ns = STREAM_SHAPE
    shape = "1x(%dch x %d i32) per call" % (nch, ns)
    x0 = synth.synth_batch_native(1, nch, ns, bps=4, device="cuda").reshape(1, -1).contiguous()
    old, new = api.SignalPacker("hzr", 4, nch, ns, 4, library=base[1]), api.SignalPacker("hzr", 4, nch, ns, 4, library=this)
    P0 = new.to_planar_i32(x0)
    x, P = torch.empty_like(x0), torch.empty_like(P0)
    for stage, (native, planar, new_state) in stages.items():
        t = {"native_stream": [], "planar_stream": []}
        for r in range(a.rounds):
            x.copy_(x0)
            st = new_state(old)
            t["native_stream"].append(timed(lambda: native(old, x, st), a.iters))
            P.copy_(P0)
            st2 = new_state(new)
            t["planar_stream"].append(timed(lambda: planar(new, P, st2), a.iters))
        x.copy_(x0)
        P.copy_(P0)
        s1, s2 = new_state(old), new_state(new)
        native(old, x, s1)
        planar(new, P, s2)
        torch.cuda.synchronize()
        same = bool(torch.equal(new.to_planar_i32(x), P)) and bool(torch.equal(s1, s2))
        for what, v in t.items():
            figure(what, stage, shape, "this" if what == "planar_stream" else base[0], v, planar_equals_native=same)
    old.close()
    new.close()
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
