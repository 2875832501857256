#!/usr/bin/env python3
"""Time PRDN on the planar int32 matrix (rspt_hip_prdn_planar_batch_dev; DESIGN.md 4f, "The planar form") against what a caller
with planar samples had to do before it, on device-resident batches; one JSON line per figure.

    shapes     64 x (64 ch x 65536) and 1024 x (12 ch x 8192) int32, the bench's synthetic blocks; --extra adds
               4096 x (12 ch x 2048) and 8192 x (12 ch x 512), where the whole-row form keeps a row in registers
    values     d = o + an error in [-16, 16): every block takes the exact-integer path (the line `sequential` has errors up to
               2^28 instead: every block down the sequential path)
    figures    planar            the entry as the host picks its form
               planar_split      k_qp_sums + k_qp_accum forced      } on the diagnostic library (python -m rspt_amd.build --diag),
               planar_rows       k_qp_rows forced                   } where RSPT_QP_FORM picks the form at handle creation
               convert+native    from_planar_i32 x 2 + prdn_batch: the route before this entry
               native            prdn_batch alone on the same values in the native layout
               copy              a device copy of one buffer of the batch: the byte floors are 1.5 x its time for three reads
                                 of the batch (split) and 1.0 x for two (whole rows)
    method     warm-up, then `iters` back-to-back calls between two events on one stream (tools/convert_bench.py); the figures
               alternate `rounds` times in this one process; per figure the median and max - min over the rounds
Behind the timed regions every form's output is compared with the native entry's, and blocks 0 and B-1 with orc.prdn.

    python tools/prdn_planar_bench.py [--iters 20] [--rounds 5] [--extra] [--out profiles/prdn_planar_bench.json]
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

SHAPES = [(64, 64, 65536), (1024, 12, 8192)]  # nblocks, nch, ns
EXTRA = [(4096, 12, 2048), (8192, 12, 512)]
FORMS = {"planar_split": "1", "planar_rows": "2"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--extra", action="store_true")
    ap.add_argument("--diag", default=None, help="the diagnostic library (default: the one beside the product library, if built)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch

    import prdn_cases as pc
    from oracle.oracle import Oracle
    from rspt_amd import api, build, synth

    this = api.lib()
    assert this.rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    diag_path = a.diag or (build.DIAG_LIB if os.path.exists(build.DIAG_LIB) else None)
    diag = api.bind(C.CDLL(os.path.abspath(diag_path))) if diag_path else None
    orc = Oracle()
    lines = []

    def figure(what, shape, v, **kw):
        lines.append(dict(tool="prdn_planar_bench", what=what, shape=shape, ms_median=round(statistics.median(v), 4), ms_spread=round(max(v) - min(v), 4),
                          ms_rounds=[round(x, 4) for x in v], **kw))
        print(json.dumps(lines[-1]), flush=True)

    def bits(t):
        return t.cpu().numpy().view(np.uint64)

    for k, (nb, nch, ns) in enumerate(SHAPES + (EXTRA if a.extra else [])):
        shape = "%dx(%dch x %d i32)" % (nb, nch, ns)
        o = synth.synth_batch_native(nb, nch, ns, bps=4, device="cuda").reshape(nb, -1).contiguous()
        pk = api.SignalPacker("hzr", 4, nch, ns, 4, library=this)
        pk.reserve(nb)
        forced = {}
        for what, val in FORMS.items() if diag else ():
            os.environ["RSPT_QP_FORM"] = val
            forced[what] = api.SignalPacker("hzr", 4, nch, ns, 4, library=diag)
            forced[what].reserve(nb)
            del os.environ["RSPT_QP_FORM"]
        P = pk.to_planar_i32(o)
        gen = torch.Generator(device="cuda").manual_seed(2100 + k)

        def decoded(amp):
            return P + torch.randint(-amp, amp, P.shape, generator=gen, device="cuda", dtype=torch.int32)

        D = decoded(16)
        d = pk.from_planar_i32(D)
        tmp_o, tmp_d, tmp = torch.empty_like(o), torch.empty_like(o), torch.empty_like(P)
        routes = {"planar": lambda: pk.prdn_planar_batch(P, D)}
        for what, h in forced.items():
            routes[what] = lambda h=h: h.prdn_planar_batch(P, D)

        def parent_route():
            pk.from_planar_i32(P, d_out=tmp_o)
            pk.from_planar_i32(D, d_out=tmp_d)
            pk.prdn_batch(tmp_o.reshape(-1), tmp_d.reshape(-1))

        routes["convert+native"] = parent_route
        routes["native"] = lambda: pk.prdn_batch(o.reshape(-1), d.reshape(-1))
        routes["copy"] = lambda: tmp.copy_(P)
        t = {what: [] for what in routes}
        for r in range(a.rounds):
            for what, fn in routes.items():
                t[what].append(timed(fn, a.iters))
        # behind the timed regions: every form against the native entry, blocks 0 and B-1 against the oracle
        want = pk.prdn_batch(o.reshape(-1), d.reshape(-1), parts=True)
        got = {"planar": pk.prdn_planar_batch(P, D, parts=True)}
        for what, h in forced.items():
            got[what] = h.prdn_planar_batch(P, D, parts=True)
        torch.cuda.synchronize()
        oh, dh = o.cpu().numpy(), d.cpu().numpy()
        orc_ok = all(int(bits(want[0])[b]) == pc.bits(orc.prdn(oh[b], dh[b], ns, nch, 4)) for b in (0, nb - 1))
        copy_ms = statistics.median(t["copy"])
        for what, v in t.items():
            kw = dict(lib="diag" if what in forced else "this", iters=a.iters)
            if what in got:
                kw.update(equals_native=all(bool(torch.equal(x, y)) for x, y in zip(got[what], want)), sequential_blocks=int(got[what][3].sum()),
                          x_three_reads=round(statistics.median(v) / (1.5 * copy_ms), 3), x_two_reads=round(statistics.median(v) / copy_ms, 3))
            if what in ("native", "planar"):
                kw.update(blocks_0_and_last_equal_orc=orc_ok)
            if what == "copy":
                kw.update(bytes=P.numel() * 4, tb_per_s=round(2 * P.numel() * 4 / (copy_ms * 1e-3) / 1e12, 3))
            figure(what, shape, v, **kw)
        if k == 0:  # every block down the sequential path
            Dq = decoded(1 << 28)
            v = [timed(lambda: pk.prdn_planar_batch(P, Dq), max(2, a.iters // 10), warmup=1) for _ in range(2)]
            ps = pk.prdn_planar_batch(P, Dq, parts=True)
            dq = pk.from_planar_i32(Dq)
            torch.cuda.synchronize()
            dqh = dq.cpu().numpy()
            ok = all(int(bits(ps[0])[b]) == pc.bits(orc.prdn(oh[b], dqh[b], ns, nch, 4)) for b in (0, nb - 1))
            figure("sequential", shape, v, lib="this", sequential_blocks=int(ps[3].sum()), blocks_0_and_last_equal_orc=ok)
            del Dq, dq
        pk.close()
        for h in forced.values():
            h.close()
        del o, P, D, d, tmp_o, tmp_d, tmp
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("".join(json.dumps(l) + "\n" for l in lines))


if __name__ == "__main__":
    main()
