#!/usr/bin/env python3
"""Time the planar FIR entries (rspt_hip_fir_prefilter_planar_batch_dev / _stream_dev; DESIGN.md 4c, "planar form") against what
a caller with planar samples had to do before them, on device-resident batches; one JSON line per figure.

    kernels      K = 1 (a gain), 5, 101, 1001 (windowed-sinc low-passes, unit gain)
    modes        in place and out of place
    figures      (a) the native entry, (b) from_planar_i32 + native entry + to_planar_i32, (c) the planar entry;
                 and the stream forms on one block of 64 ch x 65536 per call on a started state, native against planar
    shapes       64 x (64 ch x 65536) and 1024 x (12 ch x 8192), int32
    --parent     an older build of the library without the planar FIR entries (loaded beside this one, bind(missing_ok=True)):
                 (a) and (b) are then timed on that library, (c) on this one, alternating `rounds` times in this one process
    method       warm-up, then `iters` back-to-back calls between two events on one stream (tools/convert_bench.py), a quarter of
                 them from K = 1001 on; per figure the median and max - min over the rounds.  An in-place region starts from a
                 fresh copy of the input and later calls filter what the earlier ones left (unit-gain kernels: the values stay in
                 range, and the kernels' time does not depend on them).
Behind the timed regions the planar entry's output on the input is compared with from_planar_i32 + native entry + to_planar_i32.

    python tools/fir_planar_bench.py [--iters 20] [--rounds 3] [--parent old/librspt_hip.so] [--out profiles/fir_planar_bench.json]
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
TAPS = (1, 5, 101, 1001)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--taps", default=",".join(map(str, TAPS)))
    a = ap.parse_args()
    import torch

    import fir_cases as fc
    from rspt_amd import api, synth

    this = api.lib()
    assert this.rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    base = ("parent", api.bind(C.CDLL(os.path.abspath(a.parent)), missing_ok=True)) if a.parent else ("this", this)
    taps = [int(k) for k in a.taps.split(",")]
    kernels = {K: ([0.75] if K == 1 else fc.windowed_sinc_lowpass(K, 0.05)) for K in taps}
    lines = []

    def iters(K):
        return max(3, a.iters // 4) if K >= 1001 else a.iters

    def figure(what, K, mode, shape, lib, v, **kw):
        lines.append(dict(tool="fir_planar_bench", K=K, mode=mode, what=what, shape=shape, lib=lib, ms_median=round(statistics.median(v), 4),
                          ms_spread=round(max(v) - min(v), 4), ms_rounds=[round(x, 4) for x in v], **kw))
        print(json.dumps(lines[-1]), flush=True)

    for nb, nch, ns in SHAPES:
        shape = "%dx(%dch x %d i32)" % (nb, nch, ns)
        x0 = synth.synth_batch_native(nb, nch, ns, bps=4, device="cuda").reshape(nb, -1).contiguous()
        old, new = api.SignalPacker("hzr", 4, nch, ns, 4, library=base[1]), api.SignalPacker("hzr", 4, nch, ns, 4, library=this)
        P0 = new.to_planar_i32(x0)
        x, y, tmp = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
        P, Q = torch.empty_like(P0), torch.empty_like(P0)
        for K, k in kernels.items():
            for mode in ("in_place", "out_of_place"):
                oop = mode == "out_of_place"
                t = {"native": [], "convert+native+convert": [], "planar": []}

                def route_a():
                    old.fir_prefilter_batch(x, k, d_dst=y if oop else None)

                def route_b():
                    old.from_planar_i32(P, d_out=tmp)
                    old.fir_prefilter_batch(tmp, k, d_dst=y if oop else None)
                    old.to_planar_i32(y if oop else tmp, d_out=Q if oop else P)

                def route_c():
                    new.fir_prefilter_planar_batch(P, k, d_out=Q if oop else None)

                for r in range(a.rounds):
                    x.copy_(x0)
                    t["native"].append(timed(route_a, iters(K)))
                    P.copy_(P0)
                    t["convert+native+convert"].append(timed(route_b, iters(K)))
                    P.copy_(P0)
                    t["planar"].append(timed(route_c, iters(K)))
                # behind the timed regions: one call of each route on the input
                P.copy_(P0)
                route_b()
                want = (Q if oop else P).clone()
                P.copy_(P0)
                Q.zero_()
                route_c()
                torch.cuda.synchronize()
                same = bool(torch.equal(Q if oop else P, want))
                del want
                for what, v in t.items():
                    figure(what, K, mode, shape, "this" if what == "planar" else base[0], v, planar_equals_native_route=same)
        old.close()
        new.close()
        del x0, P0, x, y, tmp, P, Q
    # the stream forms: one block per call on a started state, in place
    nch, ns = STREAM_SHAPE
    shape = "1x(%dch x %d i32) per call" % (nch, ns)
    x0 = synth.synth_batch_native(1, nch, ns, bps=4, device="cuda").reshape(1, -1).contiguous()
    old, new = api.SignalPacker("hzr", 4, nch, ns, 4, library=base[1]), api.SignalPacker("hzr", 4, nch, ns, 4, library=this)
    P0 = new.to_planar_i32(x0)
    x, P = torch.empty_like(x0), torch.empty_like(P0)
    for K, k in kernels.items():
        t = {"native_stream": [], "planar_stream": []}
        for r in range(a.rounds):
            x.copy_(x0)
            st = old.fir_state(K)
            t["native_stream"].append(timed(lambda: old.fir_prefilter_batch(x, k, state=st), iters(K)))  # (the warm-up starts the state)
            P.copy_(P0)
            st2 = new.fir_planar_state(K)
            t["planar_stream"].append(timed(lambda: new.fir_prefilter_planar_batch(P, k, state=st2), iters(K)))
        s1, s2 = old.fir_state(K), new.fir_planar_state(K)
        for _ in range(2):  # a fresh and a started call
            x.copy_(x0)
            P.copy_(P0)
            old.fir_prefilter_batch(x, k, state=s1)
            new.fir_prefilter_planar_batch(P, k, state=s2)
        torch.cuda.synchronize()
        same = bool(torch.equal(new.to_planar_i32(x), P)) and bool(torch.equal(s1, s2))
        for what, v in t.items():
            figure(what, K, "in_place", shape, "this" if what == "planar_stream" else base[0], v, planar_equals_native=same)
    old.close()
    new.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
