#!/usr/bin/env python3
"""Time compress-a-batch-to-one-byte-total (rspt_hip_compress_total_batch_dev) against what delivers its two tables
today and against the same result by hand; one JSON line per figure.  Shapes, ladder and method are tools/budget_bench.py's.

    shapes     hadamard, int32, ECG-like synthetic (synth.synth_batch_native): 1024 x (12 ch x 8192) and 16 x (64 ch x 65536)
    ladder     {1/16, 1/4, 1, 4, 64}, the handle's nb = 3; the total is the median over the levels L of cost(L)
    (a) auto      compress_to_total on the route the host picks
    (b) general   compress_to_total with the general route forced (rspt_hip_debug_set_total_route)
    (c) siblings  one compress_to_budget and one compress_to_prdn at the same ladder: what delivers the two answers separately today
    (d) by hand   per ladder entry compress_batch(ladder=, choice=) at a constant choice, its decompress_batch and prdn_batch; the
                  rule in torch on the device; a final compress_batch(ladder=, choice=)
    (c) and (d) run entries the tree had before this one, never the code under test.
    timing     wall clock around `iters` back-to-back calls with a device synchronisation on either side, `rounds` rounds, all
               variants alternating within a round; every line holds the best round, all of them, and their spread
               (max - min) / min; in ms per call
    (e)        --kernels BxK: no timing -- a few total, budget and target calls on B tiny blocks with K entries, to be run under
               `rocprofv3 --kernel-trace --stats`; --fold DIR then reads the kernel stats below DIR and adds the level kernels (k_total_level, or
               the launches of k_total_round) + k_total_pick and k_budget_select + k_target_select of that run to the lines

    python tools/total_bench.py [--iters 5] [--rounds 5] [--out profiles/total_bench.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/total_bench.py --kernels 65535x8
    python tools/total_bench.py --fold DIR --label 65535x8 --out profiles/total_bench.json      (appends)
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 12, 8192), (16, 64, 65536)]
LADDER = [1.0 / 16, 1.0 / 4, 1.0, 4.0, 64.0]
LADDER8 = [1.0 / 64, 1.0 / 16, 1.0 / 4, 1.0 / 2, 1.0, 2.0, 4.0, 64.0]
RULE_KERNELS = ("k_total_figs", "k_total_level", "k_total_round", "k_total_pick", "k_budget_select", "k_target_select")


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


def torch_rule(sizes, prdn, mse, path, total):
    """the rule of rspt_hip.h on the device, every level at once: sizes, prdn, mse, path [K][B] -> (choice [B], level, cost)"""
    import torch

    K, B = sizes.shape
    big = torch.iinfo(torch.int64).max
    rated = (path == 0) & ((mse == 0) | ~prdn.isnan())
    fig = torch.where(mse == 0, torch.zeros_like(prdn), prdn)
    block_rated = rated.any(0)
    inf = torch.full((1,), float("inf"), dtype=prdn.dtype, device=prdn.device)
    levels = torch.cat([fig[rated], inf]).unique()  # ascending
    ok = torch.where(block_rated[None, None, :], rated[None] & (fig[None] <= levels[:, None, None]), True)
    keyed = torch.where(ok, sizes[None] * K + torch.arange(K, device=sizes.device)[None, :, None], big)  # (size, index): the lowest index among equals
    best = keyed.amin(1)
    adm = (best < big).all(1)
    cost = torch.where(adm, torch.where(best < big, best // K, 0).sum(1), big)
    fits = adm & (cost <= total)
    at = int(torch.nonzero(fits)[0]) if bool(fits.any()) else len(levels) - 1
    return (best[at] % K).to(torch.int32), float(levels[at]) if bool(block_rated.any()) else 0.0, int(cost[at])


def kernels_run(label):
    """(e): the calls whose rule kernels a kernel trace is to time, on B tiny blocks with K entries"""
    import torch

    from rspt_amd import api, synth

    B, K = (int(v) for v in label.split("x"))
    ladder = LADDER8[:K]
    pk = api.new_hadamard(4, 3, 8)
    pk.set_quantizer(nb=2)
    x = synth.synth_batch_native(B, 3, 8, bps=4, ecg=True, device="cuda").reshape(B, -1).contiguous()
    pk.debug_set_total_route(1), pk.debug_set_budget_route(1)  # (any batch size: the rule kernels are the same on either route)
    cand = pk.compress_to_total(x, 0, ladder, tables=True)[6]
    torch.cuda.synchronize()
    total = int(cand.amin(0).sum() + cand.amax(0).sum()) // 2
    budget = int(cand.reshape(-1).sort().values[cand.numel() // 2])
    for _ in range(5):
        pk.compress_to_total(x, total, ladder)
        pk.compress_to_budget(x, budget, ladder)
        pk.compress_to_prdn(x, 1.0, ladder)
    torch.cuda.synchronize()
    pk.close()


def fold(where, label):
    """the rule kernels' lines of a rocprofv3 kernel stats file below `where`; level_us: all of a call's level kernels -- one
    k_total_level, or the kTotalRounds launches of k_total_round -- per call"""
    found = sorted(glob.glob(os.path.join(where, "**", "*kernel_stats.csv"), recursive=True))
    assert found, "no kernel stats below %s" % where
    rows = {}
    for r in csv.DictReader(open(found[-1])):
        for k in RULE_KERNELS:
            if k in r["Name"]:
                rows[k] = dict(calls=int(r["Calls"]), total_us=round(float(r["TotalDurationNs"]) / 1e3, 3), avg_us=round(float(r["AverageNs"]) / 1e3, 3),
                               min_us=round(float(r["MinNs"]) / 1e3, 3), max_us=round(float(r["MaxNs"]) / 1e3, 3))
    level = [k for k in ("k_total_level", "k_total_round") if k in rows]
    assert len(level) == 1 and set(rows) == set(RULE_KERNELS[:1] + RULE_KERNELS[3:]) | set(level), sorted(rows)
    level_us = rows[level[0]]["total_us"] / rows["k_total_pick"]["calls"]
    return [dict(tool="total_bench", what="rule_kernels", table=label, kernels=rows, level_kernel=level[0], level_us=round(level_us, 3),
                 total_level_plus_pick_us=round(level_us + rows["k_total_pick"]["avg_us"], 3), total_figs_us=rows["k_total_figs"]["avg_us"],
                 budget_select_plus_target_select_us=round(rows["k_budget_select"]["avg_us"] + rows["k_target_select"]["avg_us"], 3))]


def bench(a):
    import torch

    from rspt_amd import api, synth

    K = len(LADDER)
    lines = []
    for nblocks, nch, ns in SHAPES:
        shape = "%dx(%dch x %d i32)" % (nblocks, nch, ns)
        x = synth.synth_batch_native(nblocks, nch, ns, bps=4, ecg=True, device="cuda").reshape(nblocks, -1).contiguous()
        pk = api.new_hadamard(4, nch, ns)
        stride = (pk.max_compressed_size + 255) // 256 * 256
        d_dst = torch.empty((nblocks, stride), dtype=torch.uint8, device="cuda")
        hand_dst = torch.empty((nblocks, stride), dtype=torch.uint8, device="cuda")
        hand_out = torch.empty((nblocks, pk.block_bytes), dtype=torch.uint8, device="cuda")
        sizes_k = torch.empty((K, nblocks), dtype=torch.int64, device="cuda")
        consts = [torch.full((nblocks,), k, dtype=torch.int32, device="cuda") for k in range(K)]
        fused_ok = api.lib().rspt_hip_debug_set_total_route(pk._h, 2) == 0
        work_bytes = {}
        for route in (1, 0):
            pk.debug_set_total_route(route)
            work_bytes[route] = pk.total_work_bytes(nblocks, K)
        work = torch.empty((max(work_bytes.values()) + 7) // 8, dtype=torch.float64, device="cuda")
        b_work = torch.empty((pk.budget_work_bytes(nblocks, K) + 7) // 8, dtype=torch.float64, device="cuda")
        t_work = torch.empty((pk.target_work_bytes(nblocks, K) + 7) // 8, dtype=torch.float64, device="cuda")
        pk.debug_set_total_route(1)
        r = pk.compress_to_total(x, 0, LADDER, work=work, d_dst=d_dst, dst_stride=stride, tables=True)
        torch.cuda.synchronize()
        cand, figs = r[6], r[7]
        # the total: the median over the levels of cost(L), from the call's own tables through the rule in torch
        levels = torch.cat([figs[~figs.isnan()], torch.full((1,), float("inf"), dtype=torch.float64, device="cuda")]).unique()
        rated = ~figs.isnan()
        costs = []
        for L in levels.tolist():
            ok = torch.where(rated.any(0)[None, :], rated & (figs <= L), True)
            best = torch.where(ok, cand, torch.iinfo(torch.int64).max).amin(0)
            if bool((best < torch.iinfo(torch.int64).max).all()):
                costs.append(int(best.sum()))
        total = sorted(costs)[len(costs) // 2]
        budget = int(cand.reshape(-1).sort().values[cand.numel() // 2])
        hand = {}

        def by_hand():
            prdn_k, mse_k, path_k = [], [], []
            for k in range(K):
                pk.compress_batch(x, hand_dst, sizes_k[k], stride, ladder=LADDER, choice=consts[k])
                pk.decompress_batch(hand_dst, nblocks, stride, d_out=hand_out, ladder=LADDER, choice=consts[k])
                f = pk.prdn_batch(x.reshape(-1), hand_out.reshape(-1), parts=True)
                prdn_k.append(f[0]), mse_k.append(f[1]), path_k.append(f[3])
            choice, level, cost = torch_rule(sizes_k, torch.stack(prdn_k), torch.stack(mse_k), torch.stack(path_k), total)
            pk.compress_batch(x, hand_dst, sizes_k[0], stride, ladder=LADDER, choice=choice)
            hand["choice"], hand["level"], hand["cost"] = choice, level, cost

        def call(route):
            def run():
                pk.debug_set_total_route(route)
                pk.compress_to_total(x, total, LADDER, work=work, d_dst=d_dst, dst_stride=stride)
                pk.debug_set_total_route(0)
            return run

        def siblings():
            pk.compress_to_budget(x, budget, LADDER, work=b_work, d_dst=d_dst, dst_stride=stride)
            pk.compress_to_prdn(x, 1.0, LADDER, work=t_work, d_dst=d_dst, dst_stride=stride)

        variants = [("total_auto", call(0)), ("total_general", call(1)), ("budget_plus_target", siblings), ("by_hand", by_hand)]
        t = {name: [] for name, _ in variants}
        for _ in range(a.rounds):
            for name, fn in variants:
                t[name].append(wall(fn, a.iters))
        # behind the timed region: every route gives what the sweep by hand gives
        by_hand()
        torch.cuda.synchronize()
        for route in (1, 2, 0) if fused_ok else (1, 0):
            pk.debug_set_total_route(route)
            s = pk.compress_to_total(x, total, LADDER, work=work)
            torch.cuda.synchronize()
            assert torch.equal(s[2], hand["choice"]) and float(s[3][0]) == hand["level"] and int(s[4][0]) == hand["cost"], "route %d differs from the sweep" % route
        pk.debug_set_total_route(0)
        choice = hand["choice"].cpu().to(torch.int64)
        for name, v in t.items():
            lines.append(dict(tool="total_bench", what=name, shape=shape, ladder=LADDER, total=total, iters=a.iters, ms=round(min(v), 4),
                              ms_rounds=[round(u, 4) for u in v], spread=round((max(v) - min(v)) / min(v), 4)))
        best = {name: min(v) for name, v in t.items()}
        lines.append(dict(tool="total_bench", what="summary", shape=shape, total=total, level=hand["level"], cost=hand["cost"], levels=len(costs),
                          host_route="fused" if fused_ok else "general", auto_over_general=round(best["total_auto"] / best["total_general"], 4),
                          auto_over_siblings=round(best["total_auto"] / best["budget_plus_target"], 4),
                          auto_over_by_hand=round(best["total_auto"] / best["by_hand"], 4), choice_counts=torch.bincount(choice, minlength=K).tolist(),
                          cr=round(nblocks * pk.block_bytes / float(hand["cost"]), 3), work_bytes_auto=work_bytes[0], work_bytes_general=work_bytes[1]))
        pk.close()
        del x, d_dst, hand_dst, hand_out, work, b_work, t_work
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", default=None, metavar="BxK")
    ap.add_argument("--fold", default=None, metavar="DIR")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if a.fold:
        lines = fold(a.fold, a.label)
    else:
        from rspt_amd import api

        assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
        if a.kernels:
            return kernels_run(a.kernels)
        lines = bench(a)
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "a" if a.fold else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
