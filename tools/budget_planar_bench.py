#!/usr/bin/env python3
"""Time compress-to-a-byte-budget on the planar matrix (rspt_hip_compress_budget_planar_batch_dev) against what a user
of the planar matrix does without it; one JSON line per figure.  The method is tools/budget_bench.py's and
tools/target_planar_bench.py's.

    shapes     hadamard, int32, ECG-like synthetic: 1024 x (12 ch x 8192) -- the batched route -- and 16 x (64 ch x 65536) -- the
               general route; the matrix is to_planar_i32 of synth.synth_batch_native
    ladder     {1/16, 1/4, 1, 4, 64}, the handle's nb = 3; one budget for every block, the median of all candidate sizes
    per route  auto (the host's pick), general and -- first shape only, the second is beyond its rows -- batched
               (rspt_hip_debug_set_budget_route), each as
               (a) planar      compress_to_budget_planar(P)
               (b) yardstick   from_planar_i32(P) + compress_to_budget on its result
               (c) native      compress_to_budget alone on the native block
    timing     wall clock around `iters` back-to-back calls with a device synchronisation on either side, `rounds` rounds, all
               variants alternating within a round; every line holds the best round, all of them, and their spread
               (max - min) / min; in ms per call.  A ratio is best over best; `spread` beside it is the larger of the two
               variants' spreads.
    memory     the work area of either entry, and the batch-sized native buffer the yardstick needs beside it, in bytes

    python tools/budget_planar_bench.py [--iters 5] [--rounds 5] [--out profiles/budget_planar_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 12, 8192), (16, 64, 65536)]
LADDER = [1.0 / 16, 1.0 / 4, 1.0, 4.0, 64.0]
ROUTE_NAMES = {0: "auto", 1: "general", 2: "batched"}


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from rspt_amd import api, synth

    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    K = len(LADDER)
    lines = []
    for nblocks, nch, ns in SHAPES:
        shape = "%dx(%dch x %d i32)" % (nblocks, nch, ns)
        x = synth.synth_batch_native(nblocks, nch, ns, bps=4, ecg=True, device="cuda").reshape(nblocks, -1).contiguous()
        pk = api.new_hadamard(4, nch, ns)
        P = pk.to_planar_i32(x)
        native = torch.empty_like(x)  # the yardstick's batch-sized buffer
        stride = (pk.max_compressed_size + 255) // 256 * 256
        d_dst = torch.empty((nblocks, stride), dtype=torch.uint8, device="cuda")
        work_bytes = dict(native=pk.budget_work_bytes(nblocks, K), planar=pk.budget_planar_work_bytes(nblocks, K))
        work = torch.empty((max(work_bytes.values()) + 7) // 8, dtype=torch.float64, device="cuda")
        batched_ok = api.lib().rspt_hip_debug_set_budget_route(pk._h, 2) == 0
        routes = (0, 1, 2) if batched_ok else (0, 1)
        pk.debug_set_budget_route(1)
        cand = pk.compress_to_budget(x, 0, LADDER, work=work, d_dst=d_dst, dst_stride=stride, cand_sizes=True)[3]
        torch.cuda.synchronize()
        budget = int(cand.reshape(-1).sort().values[cand.numel() // 2])

        # ahead of the timed region: on every route the planar call is the yardstick byte for byte
        keep = None
        for route in routes:
            pk.debug_set_budget_route(route)
            n_dst, n_sizes, n_choice, n_cand = pk.compress_to_budget(pk.from_planar_i32(P, native), budget, LADDER, work=work, cand_sizes=True)
            p_dst, p_sizes, p_choice, p_cand = pk.compress_to_budget_planar(P, budget, LADDER, work=work, cand_sizes=True)
            torch.cuda.synchronize()
            assert torch.equal(n_choice, p_choice) and torch.equal(n_sizes, p_sizes) and torch.equal(n_cand, p_cand), "route %d: another choice" % route
            keep = torch.arange(n_dst.shape[1], device="cuda")[None, :] < n_sizes[:, None]
            assert torch.equal(torch.where(keep, p_dst, 0), torch.where(keep, n_dst, 0)), "route %d writes other streams" % route
            choice, sizes = n_choice.cpu().to(torch.int64), n_sizes.cpu()
            del n_dst, p_dst, keep
        pk.debug_set_budget_route(0)

        def on(route, fn):
            def run():
                pk.debug_set_budget_route(route)
                fn()
                pk.debug_set_budget_route(0)
            return run

        def planar():
            pk.compress_to_budget_planar(P, budget, LADDER, work=work, d_dst=d_dst, dst_stride=stride)

        def yardstick():
            pk.from_planar_i32(P, native)
            pk.compress_to_budget(native, budget, LADDER, work=work, d_dst=d_dst, dst_stride=stride)

        def native_alone():
            pk.compress_to_budget(x, budget, LADDER, work=work, d_dst=d_dst, dst_stride=stride)

        variants = []
        for route in routes:
            r = ROUTE_NAMES[route]
            variants += [("planar_" + r, on(route, planar)), ("yardstick_" + r, on(route, yardstick)), ("native_" + r, on(route, native_alone))]
        t = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            for name, fn in variants:
                t[name].append(wall(fn, a.iters))

        def spread(k):
            return (max(t[k]) - min(t[k])) / min(t[k])

        for name, v in t.items():
            lines.append(dict(tool="budget_planar_bench", what=name, shape=shape, ladder=LADDER, budget=budget, iters=a.iters, ms=round(min(v), 4),
                              ms_rounds=[round(u, 4) for u in v], spread=round(spread(name), 4)))

        def ratio(num, den):
            return dict(ratio=round(min(t[num]) / min(t[den]), 4), spread=round(max(spread(num), spread(den)), 4))

        summary = dict(tool="budget_planar_bench", what="ratios", shape=shape, budget=budget, host_route="batched" if batched_ok else "general",
                       work_bytes=work_bytes, yardstick_native_buffer_bytes=native.numel(), planar_matrix_bytes=P.numel() * 4,
                       choice_counts=torch.bincount(choice, minlength=K).tolist(), over_budget=int((sizes > budget).sum()),
                       cr=round(nblocks * pk.block_bytes / float(sizes.sum()), 3))
        for route in routes:
            r = ROUTE_NAMES[route]
            summary["planar_over_yardstick_" + r] = ratio("planar_" + r, "yardstick_" + r)
            summary["planar_over_native_" + r] = ratio("planar_" + r, "native_" + r)
        lines.append(summary)
        pk.close()
        del x, P, native, d_dst, work
        torch.cuda.empty_cache()
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
