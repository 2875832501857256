#!/usr/bin/env python3
"""Time compress-a-batch-to-one-byte-total on the planar matrix (rspt_hip_compress_total_planar_batch_dev) against what
a user of the planar matrix does without it; one JSON line per figure.  Shapes, ladder and the placement of the total are
tools/total_bench.py's, the method is tools/budget_planar_bench.py's.

    shapes     hadamard, int32, ECG-like synthetic: 1024 x (12 ch x 8192) -- the fused route -- and 16 x (64 ch x 65536) -- the
               general route; the matrix is to_planar_i32 of synth.synth_batch_native
    ladder     {1/16, 1/4, 1, 4, 64}, the handle's nb = 3; the total is the median over the levels L of cost(L)
    per route  auto (the host's pick), general and -- first shape only, the second is beyond its rows -- fused
               (rspt_hip_debug_set_total_route), each as
               (a) planar      compress_to_total_planar(P)
               (b) yardstick   from_planar_i32(P) + compress_to_total on its result
               (c) native      compress_to_total alone on the native block: the entry of profiles/total_bench.json, timed again
    timing     wall clock around `iters` back-to-back calls with a device synchronisation on either side, `rounds` rounds, all
               variants alternating within a round; every line holds the best round, all of them, and their spread
               (max - min) / min; in ms per call.  A ratio is best over best; `spread` beside it is the larger of the two
               variants' spreads.
    memory     the work area of either entry on either route, and the batch-sized native buffer the yardstick needs beside it
    steps      every shape runs in a child process of its own under a time limit (--limit seconds); the first one that fails or
               runs out of time ends the run

    python tools/total_planar_bench.py [--iters 5] [--rounds 5] [--limit 240] [--out profiles/total_planar_bench.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 12, 8192), (16, 64, 65536)]
LADDER = [1.0 / 16, 1.0 / 4, 1.0, 4.0, 64.0]
ROUTE_NAMES = {0: "auto", 1: "general", 2: "fused"}


def wall(fn, iters, warmup=1):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def median_total(cand, figs):
    """the median over the levels L of cost(L), from a call's own tables (tools/total_bench.py)"""
    import torch

    big = torch.iinfo(torch.int64).max
    rated = ~figs.isnan()
    levels = torch.cat([figs[rated], torch.full((1,), float("inf"), dtype=torch.float64, device=figs.device)]).unique()
    costs = []
    for L in levels.tolist():
        ok = torch.where(rated.any(0)[None, :], rated & (figs <= L), True)
        best = torch.where(ok, cand, big).amin(0)
        if bool((best < big).all()):
            costs.append(int(best.sum()))
    return sorted(costs)[len(costs) // 2], len(costs)


def bench_shape(a, nblocks, nch, ns):
    import torch

    from rspt_amd import api, synth

    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    K = len(LADDER)
    lines = []
    shape = "%dx(%dch x %d i32)" % (nblocks, nch, ns)
    x = synth.synth_batch_native(nblocks, nch, ns, bps=4, ecg=True, device="cuda").reshape(nblocks, -1).contiguous()
    pk = api.new_hadamard(4, nch, ns)
    P = pk.to_planar_i32(x)
    native = torch.empty_like(x)  # the yardstick's batch-sized buffer
    stride = (pk.max_compressed_size + 255) // 256 * 256
    d_dst = torch.empty((nblocks, stride), dtype=torch.uint8, device="cuda")
    fused_ok = api.lib().rspt_hip_debug_set_total_route(pk._h, 2) == 0
    routes = (0, 1, 2) if fused_ok else (0, 1)
    work_bytes = {}
    for route in routes:
        pk.debug_set_total_route(route)
        work_bytes[ROUTE_NAMES[route]] = dict(native=pk.total_work_bytes(nblocks, K), planar=pk.total_planar_work_bytes(nblocks, K))
    work = torch.empty((max(max(v.values()) for v in work_bytes.values()) + 7) // 8, dtype=torch.float64, device="cuda")
    pk.debug_set_total_route(1)
    r = pk.compress_to_total(x, 0, LADDER, work=work, d_dst=d_dst, dst_stride=stride, tables=True)
    torch.cuda.synchronize()
    total, nlevels = median_total(r[6], r[7])
    del r

    # ahead of the timed region: on every route the planar call is the yardstick bit for bit
    for route in routes:
        pk.debug_set_total_route(route)
        n = pk.compress_to_total(pk.from_planar_i32(P, native), total, LADDER, work=work, tables=True)
        p = pk.compress_to_total_planar(P, total, LADDER, work=work, tables=True)
        torch.cuda.synchronize()
        for i in range(1, 8):
            assert torch.equal(n[i].view(torch.int64) if n[i].dtype == torch.float64 else n[i],
                               p[i].view(torch.int64) if p[i].dtype == torch.float64 else p[i]), "route %d: result %d differs" % (route, i)
        keep = torch.arange(n[0].shape[1], device="cuda")[None, :] < n[1][:, None]
        assert torch.equal(torch.where(keep, p[0], 0), torch.where(keep, n[0], 0)), "route %d writes other streams" % route
        choice, sizes, level, cost = n[2].cpu().to(torch.int64), n[1].cpu(), float(n[3][0]), int(n[4][0])
        del n, p, keep
    pk.debug_set_total_route(0)

    def on(route, fn):
        def run():
            pk.debug_set_total_route(route)
            fn()
            pk.debug_set_total_route(0)
        return run

    def planar():
        pk.compress_to_total_planar(P, total, LADDER, work=work, d_dst=d_dst, dst_stride=stride)

    def yardstick():
        pk.from_planar_i32(P, native)
        pk.compress_to_total(native, total, LADDER, work=work, d_dst=d_dst, dst_stride=stride)

    def native_alone():
        pk.compress_to_total(x, total, LADDER, work=work, d_dst=d_dst, dst_stride=stride)

    variants = []
    for route in routes:
        rn = ROUTE_NAMES[route]
        variants += [("planar_" + rn, on(route, planar)), ("yardstick_" + rn, on(route, yardstick)), ("native_" + rn, on(route, native_alone))]
    t = {name: [] for name, _ in variants}
    for _ in range(a.rounds):
        for name, fn in variants:
            t[name].append(wall(fn, a.iters))

    def spread(k):
        return (max(t[k]) - min(t[k])) / min(t[k])

    for name, v in t.items():
        lines.append(dict(tool="total_planar_bench", what=name, shape=shape, ladder=LADDER, total=total, iters=a.iters, ms=round(min(v), 4),
                          ms_rounds=[round(u, 4) for u in v], spread=round(spread(name), 4)))

    def ratio(num, den):
        return dict(ratio=round(min(t[num]) / min(t[den]), 4), spread=round(max(spread(num), spread(den)), 4))

    summary = dict(tool="total_planar_bench", what="ratios", shape=shape, total=total, level=level, cost=cost, levels=nlevels,
                   host_route="fused" if fused_ok else "general", work_bytes=work_bytes, yardstick_native_buffer_bytes=native.numel(),
                   planar_matrix_bytes=P.numel() * 4, choice_counts=torch.bincount(choice, minlength=K).tolist(),
                   cr=round(nblocks * pk.block_bytes / float(sizes.sum()), 3))
    for route in routes:
        rn = ROUTE_NAMES[route]
        summary["planar_over_yardstick_" + rn] = ratio("planar_" + rn, "yardstick_" + rn)
        summary["planar_over_native_" + rn] = ratio("planar_" + rn, "native_" + rn)
    lines.append(summary)
    pk.close()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", type=int, default=None, help="(the child process of one shape) its index in SHAPES")
    a = ap.parse_args()
    if a.shape is not None:
        print("".join(json.dumps(l) + "\n" for l in bench_shape(a, *SHAPES[a.shape])), end="")
        return 0
    text = ""
    for i in range(len(SHAPES)):
        cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--shape", str(i), "--iters", str(a.iters),
               "--rounds", str(a.rounds)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        print(done.stdout, end="", flush=True)
        if done.returncode:
            print("shape %d ended with status %d: nothing more is started" % (i, done.returncode), file=sys.stderr)
            return done.returncode
        text += done.stdout
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
