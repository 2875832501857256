#!/usr/bin/env python3
"""Time compress-to-a-PRDN-target (rspt_hip_compress_target_batch_dev) against what a user does without it; one JSON
line per figure.

    shapes     hadamard, int32, ECG-like synthetic (synth.synth_batch_native): 1024 x (12 ch x 8192) and 16 x (64 ch x 65536)
    ladder     {1/16, 1/4, 1, 4, 64}, target 1 %, the handle's nb = 3
    (a) by hand   per ladder entry set_quantizer, compress_batch, decompress_batch, prdn_batch -- the existing entries only --
                  then the rule on the figures (torch, one read-back of the batch's quality: the quantiser is handle state, so
                  one quality is forced on the whole batch -- the finest any block needs), set_quantizer and one compress_batch
    (b) general   compress_to_prdn with the general route forced (rspt_hip_debug_set_target_route)
    (c) fused     compress_to_prdn with the fused probe forced; first shape only (the second is beyond its rows)
    (d) ladder    compress_batch(ladder=, choice=) with every block at quality 4 against plain compress_batch at quality 4:
                  what reading the quantiser from the table costs, as a ratio
    (e) plain     compress_batch at the handle's default setting; with --parent also on an older build of the library loaded
                  beside this one, alternating within every round: the plain kernels are the parent's instruction for
                  instruction (tools/isa_diff.py), so a difference beyond the spread is a finding
    timing     wall clock around `iters` back-to-back calls with a device synchronisation on either side -- (a) synchronises
               inside, so stream events alone would not see its host time --, `rounds` rounds, all variants alternating within
               a round; every line holds the best round and all of them (the spread), in ms per call

    python tools/target_bench.py [--iters 5] [--rounds 5] [--parent old/librspt_hip.so] [--out profiles/target_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(1024, 12, 8192), (16, 64, 65536)]
LADDER = [1.0 / 16, 1.0 / 4, 1.0, 4.0, 64.0]
TARGET = 1.0


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
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from rspt_amd import api, synth

    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    parent = api.bind(C.CDLL(os.path.abspath(a.parent)), missing_ok=True) if a.parent else None
    lines = []
    for nblocks, nch, ns in SHAPES:
        shape = "%dx(%dch x %d i32)" % (nblocks, nch, ns)
        x = synth.synth_batch_native(nblocks, nch, ns, bps=4, ecg=True, device="cuda").reshape(nblocks, -1).contiguous()
        pk = api.new_hadamard(4, nch, ns)
        stride = (pk.max_compressed_size + 255) // 256 * 256
        d_dst = torch.empty((nblocks, stride), dtype=torch.uint8, device="cuda")
        d_sizes = torch.empty(nblocks, dtype=torch.int64, device="cuda")
        back = torch.empty_like(x)
        used = torch.empty(nblocks, dtype=torch.int64, device="cuda")
        work = torch.empty((pk.target_work_bytes(nblocks, len(LADDER)) + 7) // 8, dtype=torch.float64, device="cuda")
        fused_ok = api.lib().rspt_hip_debug_set_target_route(pk._h, 2) == 0
        pk.debug_set_target_route(0)
        all4 = torch.full((nblocks,), LADDER.index(4.0), dtype=torch.int32, device="cuda")

        def by_hand():
            figs = []
            for q in LADDER:
                pk.set_quantizer(q)
                pk.compress_batch(x, d_dst, d_sizes, stride)
                pk.decompress_batch(d_dst, nblocks, stride, back, used)
                figs.append(pk.prdn_batch(x.reshape(-1), back.reshape(-1), parts=True))
            meets = torch.stack([(path == 0) & ((mse == 0) | (prdn <= TARGET)) for prdn, mse, ref, path in figs])  # [K, nblocks]
            first = torch.where(meets.any(0), meets.to(torch.int32).argmax(0), len(LADDER) - 1)  # the first entry that meets it, else the last
            pk.set_quantizer(LADDER[int(first.max())])  # one quality for the batch
            pk.compress_batch(x, d_dst, d_sizes, stride)
            pk.set_quantizer(1.0)

        def target(route):
            def run():
                pk.debug_set_target_route(route)
                pk.compress_to_prdn(x, TARGET, LADDER, work=work, d_dst=d_dst, dst_stride=stride)
                pk.debug_set_target_route(0)
            return run

        def at_quality_4(ladder):
            def run():
                if ladder:
                    pk.compress_batch(x, d_dst, d_sizes, stride, ladder=LADDER, choice=all4)
                else:
                    pk.compress_batch(x, d_dst, d_sizes, stride)
            return run

        variants = [("by_hand", by_hand), ("target_general", target(1))]
        if fused_ok:
            variants.append(("target_fused", target(2)))
        variants.append(("plain_default", lambda: pk.compress_batch(x, d_dst, d_sizes, stride)))
        if parent is not None:
            pp = api.SignalPacker("hadamard", 4, nch, ns, 3, library=parent)
            variants.append(("plain_default_parent", lambda: pp.compress_batch(x, d_dst, d_sizes, stride)))
        t = {name: [] for name, _ in variants}
        t["ladder_q4"], t["plain_q4"] = [], []
        for r in range(a.rounds):
            for name, fn in variants:
                t[name].append(wall(fn, a.iters))
            pk.set_quantizer(4.0)
            t["plain_q4"].append(wall(at_quality_4(False), a.iters))
            pk.set_quantizer(1.0)
            t["ladder_q4"].append(wall(at_quality_4(True), a.iters))
        # behind the timed region: what the call chose, and that both routes agree
        res = {}
        for route in (1, 2) if fused_ok else (1,):
            pk.debug_set_target_route(route)
            s_dst, s_sizes, s_choice, s_prdn = pk.compress_to_prdn(x, TARGET, LADDER, work=work)
            torch.cuda.synchronize()
            res[route] = (s_choice.cpu(), s_prdn.cpu(), s_sizes.cpu())
        pk.debug_set_target_route(0)
        if fused_ok:
            assert all(torch.equal(u, v) for u, v in zip(res[1], res[2])), "the two routes disagree"
        choice, prdn, sizes = res[1]
        chosen = dict(choice_counts=torch.bincount(choice, minlength=len(LADDER)).tolist(), prdn_max=round(float(prdn.max()), 4),
                      cr=round(nblocks * pk.block_bytes / float(sizes.sum()), 3))
        for name, v in t.items():
            lines.append(dict(tool="target_bench", what=name, shape=shape, ladder=LADDER, target=TARGET, iters=a.iters, ms=round(min(v), 4),
                              ms_rounds=[round(u, 4) for u in v]))
        best = {name: min(v) for name, v in t.items()}
        ratios = dict(tool="target_bench", what="ratios", shape=shape, general_over_by_hand=round(best["target_general"] / best["by_hand"], 4),
                      ladder_over_plain_q4=round(best["ladder_q4"] / best["plain_q4"], 4), **chosen)
        if fused_ok:
            ratios["fused_over_general"] = round(best["target_fused"] / best["target_general"], 4)
        if parent is not None:
            ratios["plain_default_this_over_parent"] = round(best["plain_default"] / best["plain_default_parent"], 4)
            pp.close()
        lines.append(ratios)
        pk.close()
        del x, d_dst, back, work
        torch.cuda.empty_cache()
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
