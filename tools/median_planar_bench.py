#!/usr/bin/env python3
"""Time the planar median entries (rspt_hip_median_filter_planar_batch_dev / _stream_dev; DESIGN.md 4d, "planar form") against
what a caller with planar samples had to do before them, on device-resident batches; one JSON line per figure.

    windows      W = 1 (a copy), 3, 7, 31 (the short kernel's buckets 4, 8, 32), 101, 1001 (the generic path)
    modes        in place and out of place
    figures      (a) the planar entry, (b) from_planar_i32 + native entry + to_planar_i32 on a bps = 4 handle, (c) the native
                 entry alone, and a device copy of the batch as the floor; (a)/(b) and (a)/(c) of the medians;
                 and the stream forms on one block of 64 ch x 65536 per call on a started state, native against planar
    shapes       64 x (64 ch x 65536) and 1024 x (12 ch x 8192), int32
    method       one process; warm-up, then `iters` back-to-back calls between two events on one stream (tools/convert_bench.py),
                 a quarter of them above W = 32; the routes alternate `rounds` times; per figure the median and max - min over
                 the rounds.  An in-place region starts from a fresh copy of the input and later calls filter what the earlier
                 ones left, on every route alike.
Behind the timed regions the planar entry's output on the input is compared with from_planar_i32 + native entry + to_planar_i32.

    python tools/median_planar_bench.py [--iters 20] [--rounds 5] [--out profiles/median_planar_bench.json]
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
STREAM_SHAPE = (64, 65536)  # one block per call
WINDOWS = (1, 3, 7, 31, 101, 1001)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", default=",".join(map(str, WINDOWS)))
    a = ap.parse_args()
    import torch

    from rspt_amd import api, synth

    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    windows = [int(w) for w in a.windows.split(",")]
    lines = []

    def iters(W):
        return max(3, a.iters // 4) if W > 32 else a.iters

    def figure(what, W, mode, shape, v, **kw):
        lines.append(dict(tool="median_planar_bench", W=W, mode=mode, what=what, shape=shape, ms_median=round(statistics.median(v), 4),
                          ms_spread=round(max(v) - min(v), 4), ms_rounds=[round(x, 4) for x in v], **kw))
        print(json.dumps(lines[-1]), flush=True)

    for nb, nch, ns in SHAPES:
        shape = "%dx(%dch x %d i32)" % (nb, nch, ns)
        x0 = synth.synth_batch_native(nb, nch, ns, bps=4, device="cuda").reshape(nb, -1).contiguous()
        pk = api.new_hzr(4, nch, ns)
        P0 = pk.to_planar_i32(x0)
        x, y, tmp = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
        P, Q = torch.empty_like(P0), torch.empty_like(P0)
        floor = [timed(lambda: Q.copy_(P0), a.iters) for _ in range(a.rounds)]
        figure("device_copy", 0, "out_of_place", shape, floor)
        for W in windows:
            for mode in ("in_place", "out_of_place"):
                oop = mode == "out_of_place"
                t = {"planar": [], "convert+native+convert": [], "native": []}

                def route_a():
                    pk.median_filter_planar_batch(P, W, d_out=Q if oop else None)

                def route_b():
                    pk.from_planar_i32(P, d_out=tmp)
                    pk.median_filter_batch(tmp, W, d_dst=y if oop else None)
                    pk.to_planar_i32(y if oop else tmp, d_out=Q if oop else P)

                def route_c():
                    pk.median_filter_batch(x, W, d_dst=y if oop else None)

                for r in range(a.rounds):
                    P.copy_(P0)
                    t["planar"].append(timed(route_a, iters(W)))
                    P.copy_(P0)
                    t["convert+native+convert"].append(timed(route_b, iters(W)))
                    x.copy_(x0)
                    t["native"].append(timed(route_c, iters(W)))
                # behind the timed regions: one call of each route on the input
                P.copy_(P0)
                route_b()
                want = (Q if oop else P).clone()
                P.copy_(P0)
                Q.zero_()
                route_a()
                torch.cuda.synchronize()
                same = bool(torch.equal(Q if oop else P, want))
                del want
                med = {k: statistics.median(v) for k, v in t.items()}
                for what, v in t.items():
                    figure(what, W, mode, shape, v, planar_equals_native_route=same, planar_over_convert_route=round(med["planar"] / med["convert+native+convert"], 4),
                           planar_over_native=round(med["planar"] / med["native"], 4))
        pk.close()
        del x0, P0, x, y, tmp, P, Q
    # the stream forms: one block per call on a started state, in place
    nch, ns = STREAM_SHAPE
    shape = "1x(%dch x %d i32) per call" % (nch, ns)
    x0 = synth.synth_batch_native(1, nch, ns, bps=4, device="cuda").reshape(1, -1).contiguous()
    pk = api.new_hzr(4, nch, ns)
    P0 = pk.to_planar_i32(x0)
    x, P = torch.empty_like(x0), torch.empty_like(P0)
    for W in windows:
        t = {"native_stream": [], "planar_stream": []}
        for r in range(a.rounds):
            x.copy_(x0)
            st = pk.median_state(W)
            t["native_stream"].append(timed(lambda: pk.median_filter_batch(x, W, state=st), iters(W)))  # (the warm-up starts the state)
            P.copy_(P0)
            st2 = pk.median_planar_state(W)
            t["planar_stream"].append(timed(lambda: pk.median_filter_planar_batch(P, W, state=st2), iters(W)))
        s1, s2 = pk.median_state(W), pk.median_planar_state(W)
        for _ in range(2):  # a fresh and a started call
            x.copy_(x0)
            P.copy_(P0)
            pk.median_filter_batch(x, W, state=s1)
            pk.median_filter_planar_batch(P, W, state=s2)
        torch.cuda.synchronize()
        same = bool(torch.equal(pk.to_planar_i32(x), P)) and bool(torch.equal(s1, s2))
        for what, v in t.items():
            figure(what, W, "in_place", shape, v, planar_equals_native=same)
    pk.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
