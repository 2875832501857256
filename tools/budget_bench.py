#!/usr/bin/env python3
"""Time compress-to-a-byte-budget (rspt_hip_compress_budget_batch_dev) against the same result by hand; one JSON line
per figure.  Shapes, ladder and method are tools/target_bench.py's.

    shapes     hadamard, int32, ECG-like synthetic (synth.synth_batch_native): 1024 x (12 ch x 8192) and 16 x (64 ch x 65536)
    ladder     {1/16, 1/4, 1, 4, 64}, the handle's nb = 3; one budget for every block, the median of all candidate sizes
    (a) by hand   the entries the tree had before this one: per ladder entry compress_batch(ladder=, choice=) at a constant choice
                  into a buffer of its own -- nladder full compressions, nladder output buffers -- then the rule and the copy of
                  each block's chosen stream on the device, in torch
    (b) general   compress_to_budget with the general route forced (rspt_hip_debug_set_budget_route)
    (c) batched   compress_to_budget with the batched route forced; first shape only (the second is beyond its rows)
    (d) auto      compress_to_budget on the route the host picks
    timing     wall clock around `iters` back-to-back calls with a device synchronisation on either side, `rounds` rounds, all
               variants alternating within a round; every line holds the best round, all of them, and their spread
               (max - min) / min; in ms per call
    memory     the call's work area against the by-hand sweep's nladder output buffers, in bytes

    python tools/budget_bench.py [--iters 5] [--rounds 5] [--out profiles/budget_bench.json]
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
        stride = (pk.max_compressed_size + 255) // 256 * 256
        d_dst = torch.empty((nblocks, stride), dtype=torch.uint8, device="cuda")
        bufs = torch.empty((K, nblocks, stride), dtype=torch.uint8, device="cuda")  # the by-hand sweep's output buffers
        sizes_k = torch.empty((K, nblocks), dtype=torch.int64, device="cuda")
        consts = [torch.full((nblocks,), k, dtype=torch.int32, device="cuda") for k in range(K)]
        rows = torch.arange(nblocks, device="cuda")
        steps = torch.arange(1, K + 1, device="cuda")[:, None]
        work = torch.empty((pk.budget_work_bytes(nblocks, K) + 7) // 8, dtype=torch.float64, device="cuda")
        batched_ok = api.lib().rspt_hip_debug_set_budget_route(pk._h, 2) == 0
        pk.debug_set_budget_route(1)
        cand = pk.compress_to_budget(x, 0, LADDER, work=work, d_dst=d_dst, dst_stride=stride, cand_sizes=True)[3]
        torch.cuda.synchronize()
        budget = int(cand.reshape(-1).sort().values[cand.numel() // 2])
        pk.debug_set_budget_route(0)
        hand = {}

        def by_hand():
            for k in range(K):
                pk.compress_batch(x, bufs[k], sizes_k[k], stride, ladder=LADDER, choice=consts[k])
            fits = sizes_k <= budget
            choice = torch.where(fits.any(0), (fits * steps).amax(0) - 1, sizes_k.argmin(0))  # the highest that fits, else the smallest
            hand["out"], hand["sizes"], hand["choice"] = bufs[choice, rows], sizes_k[choice, rows], choice

        def call(route):
            def run():
                pk.debug_set_budget_route(route)
                pk.compress_to_budget(x, budget, LADDER, work=work, d_dst=d_dst, dst_stride=stride)
                pk.debug_set_budget_route(0)
            return run

        variants = [("by_hand", by_hand), ("budget_general", call(1))]
        if batched_ok:
            variants.append(("budget_batched", call(2)))
        variants.append(("budget_auto", call(0)))
        t = {name: [] for name, _ in variants}
        for r in range(a.rounds):
            for name, fn in variants:
                t[name].append(wall(fn, a.iters))
        # behind the timed region: every route gives what the sweep by hand gives
        by_hand()
        torch.cuda.synchronize()
        for route in (1, 2, 0) if batched_ok else (1, 0):
            pk.debug_set_budget_route(route)
            s_dst, s_sizes, s_choice = pk.compress_to_budget(x, budget, LADDER, work=work)
            torch.cuda.synchronize()
            assert torch.equal(s_choice.to(torch.int64), hand["choice"]) and torch.equal(s_sizes, hand["sizes"]), "route %d differs from the sweep" % route
            keep = torch.arange(stride, device="cuda")[None, :] < s_sizes[:, None]
            assert torch.equal(torch.where(keep, s_dst, 0), torch.where(keep, hand["out"], 0)), "route %d writes other streams" % route
        pk.debug_set_budget_route(0)
        choice, sizes = hand["choice"].cpu(), hand["sizes"].cpu()
        for name, v in t.items():
            lines.append(dict(tool="budget_bench", what=name, shape=shape, ladder=LADDER, budget=budget, iters=a.iters, ms=round(min(v), 4),
                              ms_rounds=[round(u, 4) for u in v], spread=round((max(v) - min(v)) / min(v), 4)))
        best = {name: min(v) for name, v in t.items()}
        summary = dict(tool="budget_bench", what="summary", shape=shape, budget=budget, general_over_by_hand=round(best["budget_general"] / best["by_hand"], 4),
                       auto_over_by_hand=round(best["budget_auto"] / best["by_hand"], 4),
                       choice_counts=torch.bincount(choice, minlength=K).tolist(), over_budget=int((sizes > budget).sum()),
                       cr=round(nblocks * pk.block_bytes / float(sizes.sum()), 3),
                       work_bytes=pk.budget_work_bytes(nblocks, K), by_hand_buffer_bytes=bufs.numel() + sizes_k.numel() * 8)
        if batched_ok:
            summary["batched_over_general"] = round(best["budget_batched"] / best["budget_general"], 4)
            summary["batched_over_by_hand"] = round(best["budget_batched"] / best["by_hand"], 4)
        lines.append(summary)
        pk.close()
        del x, d_dst, bufs, work, hand
        torch.cuda.empty_cache()
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
