#!/usr/bin/env python3
"""Time the planar ladder and target entries (rspt_hip_compress_target_planar_batch_dev, rspt_hip_compress_planar_batch_ladder_dev,
rspt_hip_decompress_planar_batch_ladder_dev) against what a user of the planar matrix does without them; one JSON
line per figure.  The method is tools/target_bench.py's.

    shapes     hadamard, int32, ECG-like synthetic: 1024 x (12 ch x 8192) -- the fused route -- and 16 x (64 ch x 65536) -- the
               general route; the matrix is to_planar_i32 of synth.synth_batch_native
    ladder     {1/16, 1/4, 1, 4, 64}, target 1 %, the handle's nb = 3
    target     (a) target_planar      compress_to_prdn_planar(P)
               (b) target_yardstick   from_planar_i32(P) + compress_to_prdn on its result
               (c) target_native      compress_to_prdn alone on the native block
    compress   compress_planar_batch(ladder=, choice=) against from_planar_i32 + compress_batch(ladder=, choice=); the choice is
               what the target call picked
    decompress decompress_planar_batch(ladder=, choice=) against decompress_batch(ladder=, choice=) + to_planar_i32
    timing     wall clock around `iters` back-to-back calls with a device synchronisation on either side, `rounds` rounds, all
               variants alternating within a round; every line holds the best round and all of them (the spread), in ms per call.
               A ratio is best over best; `spread` beside it is the larger of the two variants' (max - min) / min over the rounds.

    python tools/target_planar_bench.py [--iters 5] [--rounds 5] [--out profiles/target_planar_bench.json]
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from rspt_amd import api, synth

    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    lines = []
    for nblocks, nch, ns in SHAPES:
        shape = "%dx(%dch x %d i32)" % (nblocks, nch, ns)
        x = synth.synth_batch_native(nblocks, nch, ns, bps=4, ecg=True, device="cuda").reshape(nblocks, -1).contiguous()
        pk = api.new_hadamard(4, nch, ns)
        P = pk.to_planar_i32(x)
        stride = (pk.max_compressed_size + 255) // 256 * 256
        d_dst = torch.empty((nblocks, stride), dtype=torch.uint8, device="cuda")
        d_sizes = torch.empty(nblocks, dtype=torch.int64, device="cuda")
        native = torch.empty_like(x)
        back = torch.empty_like(x)
        backP = torch.empty_like(P)
        used = torch.empty(nblocks, dtype=torch.int64, device="cuda")
        K = len(LADDER)
        fused = api.lib().rspt_hip_debug_set_target_route(pk._h, 2) == 0
        pk.debug_set_target_route(0)
        work_bytes = dict(native=pk.target_work_bytes(nblocks, K), planar=pk.target_planar_work_bytes(nblocks, K))
        work = torch.empty((work_bytes["native"] + 7) // 8, dtype=torch.float64, device="cuda")
        workP = torch.empty((work_bytes["planar"] + 7) // 8, dtype=torch.float64, device="cuda")

        # what the calls choose, and that the planar call is the yardstick bit for bit
        r_n = pk.compress_to_prdn(x, TARGET, LADDER, work=work)
        r_p = pk.compress_to_prdn_planar(P, TARGET, LADDER, work=workP)
        torch.cuda.synchronize()
        assert torch.equal(r_n[2], r_p[2]) and torch.equal(r_n[1], r_p[1]) and torch.equal(r_n[3].view(torch.int64), r_p[3].view(torch.int64))
        choice = r_p[2].clone()
        streams = r_p[0].clone()
        sstride = streams.shape[1]

        def yardstick():
            pk.from_planar_i32(P, native)
            pk.compress_to_prdn(native, TARGET, LADDER, work=work, d_dst=d_dst, dst_stride=stride)

        def ladder_yardstick():
            pk.from_planar_i32(P, native)
            pk.compress_batch(native, d_dst, d_sizes, stride, ladder=LADDER, choice=choice)

        def decode_yardstick():
            pk.decompress_batch(streams, nblocks, sstride, back, used, ladder=LADDER, choice=choice)
            pk.to_planar_i32(back, backP)

        variants = [
            ("target_planar", lambda: pk.compress_to_prdn_planar(P, TARGET, LADDER, work=workP, d_dst=d_dst, dst_stride=stride)),
            ("target_yardstick", yardstick),
            ("target_native", lambda: pk.compress_to_prdn(x, TARGET, LADDER, work=work, d_dst=d_dst, dst_stride=stride)),
            ("ladder_compress_planar", lambda: pk.compress_planar_batch(P, d_dst, d_sizes, stride, ladder=LADDER, choice=choice)),
            ("ladder_compress_yardstick", ladder_yardstick),
            ("ladder_decompress_planar", lambda: pk.decompress_planar_batch(streams, nblocks, sstride, backP, used, ladder=LADDER, choice=choice)),
            ("ladder_decompress_yardstick", decode_yardstick),
        ]
        t = {name: [] for name, _ in variants}
        for r in range(a.rounds):
            for name, fn in variants:
                t[name].append(wall(fn, a.iters))
        for name, v in t.items():
            lines.append(dict(tool="target_planar_bench", what=name, shape=shape, route="fused" if fused else "general", ladder=LADDER, target=TARGET,
                              iters=a.iters, ms=round(min(v), 4), ms_rounds=[round(u, 4) for u in v]))

        def ratio(num, den):
            spread = max((max(t[k]) - min(t[k])) / min(t[k]) for k in (num, den))
            return dict(ratio=round(min(t[num]) / min(t[den]), 4), spread=round(spread, 4))

        lines.append(dict(tool="target_planar_bench", what="ratios", shape=shape, route="fused" if fused else "general",
                          target_planar_over_yardstick=ratio("target_planar", "target_yardstick"),
                          target_planar_over_native=ratio("target_planar", "target_native"),
                          ladder_compress_planar_over_yardstick=ratio("ladder_compress_planar", "ladder_compress_yardstick"),
                          ladder_decompress_planar_over_yardstick=ratio("ladder_decompress_planar", "ladder_decompress_yardstick"),
                          work_bytes=work_bytes, planar_copy_bytes=nblocks * nch * ns * 4,
                          choice_counts=torch.bincount(choice, minlength=K).tolist()))
        pk.close()
        del x, P, d_dst, native, back, backP, work, workP, streams
        torch.cuda.empty_cache()
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
