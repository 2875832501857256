#!/usr/bin/env python3
"""Time the planar int32 entries (rspt_hip_compress_planar_batch_dev / rspt_hip_decompress_planar_batch_dev)
against what a caller with planar samples had to do before them, on device-resident batches; one JSON line per figure.

    compress     (a) native compress_batch, (b) from_planar_i32 + compress_batch, (c) compress_planar_batch
    decompress   (a) native decompress_batch, (b) decompress_batch + to_planar_i32, (c) decompress_planar_batch
    shapes       64 x (64 ch x 65536) int32 and int24, 1024 x (12 ch x 8192) int32, 8 x (16384 ch x 4096) int32 (xdelta_hzr);
                 hadamard and dct (64 ch x 65536 int32) at 16 blocks, compress only
    --parent     an older build of the library without the planar entries (loaded beside this one, bind(missing_ok=True)):
                 (a) and (b) are then timed on BOTH libraries, alternating `rounds` times in this one process, so that (c) stands
                 beside (b) of the parent commit from the same run
    floor        the device-copy rate measured in the same process (a copy of N bytes moves 2 N)
    method       warm-up, then `iters` back-to-back calls between two events on one stream (tools/convert_bench.py)
Behind the timed region the planar streams are compared with the native entry's and, one block per shape, with the CPU oracle;
the decoded matrix with the input.

    python tools/planar_bench.py [--iters 20] [--rounds 3] [--parent old/librspt_hip.so] [--out profiles/planar_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from convert_bench import timed  # noqa: E402

LOSSLESS_SHAPES = [(64, 4, 64, 65536), (64, 3, 64, 65536), (1024, 4, 12, 8192), (8, 4, 16384, 4096)]  # nblocks, bps, nch, ns
LOSSY_SHAPES = [("hadamard", 16, 4, 64, 65536), ("dct", 16, 4, 64, 65536)]


def packer_on(api, L, kind, bps, nch, ns, nb):
    """a SignalPacker whose calls go to the library L (this build's, or the parent's loaded beside it)"""
    return api.SignalPacker(kind, bps, nch, ns, nb, library=L)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from oracle.oracle import Oracle
    from rspt_amd import api, synth

    import convert_cases as cc

    this = api.lib()
    assert this.rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    libs = [("this", this)]
    if a.parent:
        libs.insert(0, ("parent", api.bind(C.CDLL(os.path.abspath(a.parent)), missing_ok=True)))
    orc = Oracle()
    lines = []
    src = torch.empty(256 << 20, dtype=torch.uint8, device="cuda").random_(0, 256)
    dst = torch.empty_like(src)
    copy_ms = timed(lambda: dst.copy_(src), a.iters)
    rate = 2 * src.numel() / (copy_ms * 1e-3)
    lines.append(dict(tool="planar_bench", what="device_copy", bytes=src.numel(), ms=round(copy_ms, 4), tb_per_s=round(rate / 1e12, 3),
                      device=torch.cuda.get_device_name(0)))
    del src, dst

    def spread(v):
        return dict(ms=round(min(v), 4), ms_rounds=[round(x, 4) for x in v])

    for kind, nb, bps, nch, ns in [("xdelta_hzr",) + s for s in LOSSLESS_SHAPES] + LOSSY_SHAPES:
        shape = "%dx(%dch x %d i%d)" % (nb, nch, ns, 8 * bps)
        iters = a.iters if kind != "dct" else max(3, a.iters // 4)
        x = synth.synth_batch_native(nb, nch, ns, bps=bps, device="cuda").reshape(nb, -1).contiguous()
        pks = {name: packer_on(api, L, kind, bps, nch, ns, 3) for name, L in libs}
        pk = pks["this"]
        planar = pk.to_planar_i32(x)
        stride = (pk.max_compressed_size + 255) // 256 * 256
        d_dst = torch.empty((nb, stride), dtype=torch.uint8, device="cuda")
        d_sizes = torch.empty(nb, dtype=torch.int64, device="cuda")
        native = torch.empty_like(x)
        out = torch.empty_like(planar)
        used = torch.empty(nb, dtype=torch.int64, device="cuda")
        nat_bytes, pl_bytes = x.numel(), 4 * planar.numel()
        t = {}
        for r in range(a.rounds):
            for name, q in pks.items():
                t.setdefault((name, "compress_native"), []).append(timed(lambda: q.compress_batch(x, d_dst, d_sizes, stride), iters))

                def conv_then_compress():
                    q.from_planar_i32(planar, d_out=native)
                    q.compress_batch(native, d_dst, d_sizes, stride)

                t.setdefault((name, "i32_to_native+compress"), []).append(timed(conv_then_compress, iters))
            t.setdefault(("this", "compress_planar"), []).append(timed(lambda: pk.compress_planar_batch(planar, d_dst, d_sizes, stride), iters))
        # behind the timed region: the planar streams against the native entry's and one block against the oracle
        n_dst, n_sizes = pk.compress_batch(x)
        p_dst, p_sizes = pk.compress_planar_batch(planar)
        torch.cuda.synchronize()
        same = bool(torch.equal(n_sizes, p_sizes)) and all(
            torch.equal(n_dst[b, : int(n_sizes[b])], p_dst[b, : int(p_sizes[b])]) for b in range(nb))
        oracle_ok = None
        if kind != "dct":  # (block 0 is the first call of a fresh instance; the oracle's dense dct of 65536 points is out of reach)
            po = orc.packer(kind, bps, nch, ns, 3)
            oracle_ok = po.compress(cc.i32_to_native(planar[0].cpu().numpy(), bps)) == p_dst[0, : int(p_sizes[0])].cpu().numpy().tobytes()
            po.close()
        for (name, what), v in t.items():
            moved = {"compress_native": nat_bytes, "i32_to_native+compress": pl_bytes + 2 * nat_bytes, "compress_planar": pl_bytes}[what]
            lines.append(dict(tool="planar_bench", lib=name, packer=kind, what=what, shape=shape, input_bytes_floor_ms=round(moved / rate * 1e3, 4),
                              streams_equal_native=same, stream0_equals_oracle=oracle_ok, **spread(v)))
        if kind == "xdelta_hzr":
            t = {}
            for r in range(a.rounds):
                for name, q in pks.items():
                    q.compress_batch(x, d_dst, d_sizes, stride)  # (this handle's nb state is the streams')
                    t.setdefault((name, "decompress_native"), []).append(timed(lambda: q.decompress_batch(d_dst, nb, stride, native, used), iters))

                    def decompress_then_conv():
                        q.decompress_batch(d_dst, nb, stride, native, used)
                        q.to_planar_i32(native, d_out=out)

                    t.setdefault((name, "decompress+native_to_i32"), []).append(timed(decompress_then_conv, iters))
                t.setdefault(("this", "decompress_planar"), []).append(timed(lambda: pk.decompress_planar_batch(d_dst, nb, stride, out, used), iters))
            out.zero_()
            pk.decompress_planar_batch(d_dst, nb, stride, out, used)
            torch.cuda.synchronize()
            ok = bool(torch.equal(out, planar)) and bool(torch.equal(used, d_sizes))
            for (name, what), v in t.items():
                lines.append(dict(tool="planar_bench", lib=name, packer=kind, what=what, shape=shape, output_bytes_floor_ms=round(
                    (pl_bytes if what != "decompress_native" else nat_bytes) / rate * 1e3, 4), round_trip_ok=ok, **spread(v)))
        for q in pks.values():
            q.close()
        del x, planar, d_dst, native, out
    text = "".join(json.dumps(l) + "\n" for l in lines)
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
