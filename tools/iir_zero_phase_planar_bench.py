#!/usr/bin/env python3
"""Time the planar zero-phase IIR entry (rspt_hip_iir_zero_phase_planar_batch_dev) against what a caller with
planar samples had to do before it, on device-resident batches; one JSON line per figure.

    filter       the README's band-pass, init_nr_samples = 2000, backward_init_nr_samples = 0
    figures      (a)  the planar entry in place
                 (a') the planar entry out of place
                 (b)  from_planar_i32 + the native entry + to_planar_i32: the route a planar caller had -- the yardstick
                 (c)  the native entry alone
    shapes       64 x (64 ch x 65536) and 1024 x (12 ch x 8192), int32
    --parent     a build of the parent commit's library, without the planar entry (loaded beside this one,
                 bind(missing_ok=True)): (b) and (c) are then timed on that library, (a) and (a') on this one, alternating
                 `rounds` times in this one process
    method       warm-up, then `iters` back-to-back calls between two events on one stream (tools/convert_bench.py); per figure
                 the median and max - min over the rounds.  All four routes share one workspace.  The in-place calls filter
                 what the call before left, so every timed region starts from a fresh copy of the input (the kernels' time does
                 not depend on the values).
Behind the timed regions the planar entry's output on the input, in place and out of place, is compared with route (b)'s.
The entry earns its place if (a) <= (b), the margin being (b)'s own spread; (a) - (c) is reported and not gated.

    python tools/iir_zero_phase_planar_bench.py [--iters 10] [--rounds 7] [--parent old/librspt_hip.so]
                                                [--out profiles/iir_zero_phase_planar_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import cases
    from rspt_amd import api, synth

    this = api.lib()
    assert this.rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    base = ("parent", api.bind(C.CDLL(os.path.abspath(a.parent)), missing_ok=True)) if a.parent else ("this", this)
    n, d = cases.IIR_BANDPASS
    kw = dict(init_nr_samples=2000, backward_init_nr_samples=0)
    lines = []
    for nb, nch, ns in SHAPES:
        shape = "%dx(%dch x %d i32)" % (nb, nch, ns)
        x0 = synth.synth_batch_native(nb, nch, ns, bps=4, device="cuda").reshape(nb, -1).contiguous()
        old, new = api.SignalPacker("hzr", 4, nch, ns, 4, library=base[1]), api.SignalPacker("hzr", 4, nch, ns, 4, library=this)
        P0 = new.to_planar_i32(x0)
        x, P, Q, tmp = torch.empty_like(x0), torch.empty_like(P0), torch.empty_like(P0), torch.empty_like(x0)
        work = torch.empty(new.iir_zero_phase_work_bytes(nb) // 8, dtype=torch.float64, device="cuda")

        def route_b():
            old.from_planar_i32(P, d_out=tmp)
            old.iir_zero_phase_batch(tmp, n, d, work=work, **kw)
            old.to_planar_i32(tmp, d_out=P)

        routes = {
            "planar_in_place": ("this", lambda: new.iir_zero_phase_planar_batch(P, n, d, work=work, **kw)),
            "planar_out_of_place": ("this", lambda: new.iir_zero_phase_planar_batch(P, n, d, out=Q, work=work, **kw)),
            "convert+native+convert": (base[0], route_b),
            "native": (base[0], lambda: old.iir_zero_phase_batch(x, n, d, work=work, **kw)),
        }
        t = {what: [] for what in routes}
        for r in range(a.rounds):
            for what, (_, fn) in routes.items():
                x.copy_(x0)
                P.copy_(P0)
                t[what].append(timed(fn, a.iters))
        # behind the timed regions: one call of each route on the input
        P.copy_(P0)
        route_b()
        want = P.clone()
        P.copy_(P0)
        routes["planar_out_of_place"][1]()
        routes["planar_in_place"][1]()
        torch.cuda.synchronize()
        same = bool(torch.equal(P, want)) and bool(torch.equal(Q, want))
        for what, v in t.items():
            lines.append(dict(tool="iir_zero_phase_planar_bench", what=what, shape=shape, lib=routes[what][0], work_bytes=work.numel() * 8, iters=a.iters,
                              ms_median=round(statistics.median(v), 4), ms_spread=round(max(v) - min(v), 4), ms_rounds=[round(q, 4) for q in v],
                              planar_equals_native_route=same))
        old.close()
        new.close()
        del x0, P0, x, P, Q, tmp, work, want
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
