#!/usr/bin/env python3
"""Time the zero-phase IIR stage (rspt_hip_iir_zero_phase_batch_dev) against what it is made of, and print one JSON
line.

On 64 x (64 ch x 65536 int32) with the README's band-pass, in one process, alternating:
    (a) zero_phase    one call of the zero-phase stage
    (b) two_forward   two back-to-back calls of rspt_hip_iir_prefilter_batch_dev(per_channel = 1) with the same coefficients (NOT
                      the same answer: both run forward and the first truncates), through the library named by --parent-lib -- a
                      build of the parent commit -- where one is given, else through this build's (the single stage's kernels are
                      the same in both)
    (c) work_copy_x2  a device-to-device copy of the workspace's byte count, twice: the stage writes w once and reads it once
Every timed call of (a) and (b) starts from the same pristine batch (copied back outside the timed region) and is timed with
device events; per side the median ms over the runs and the spread (max - min).  `accepted`: (a) <= 1.25 x ((b) + (c)).  After
the timed region a block of the batch's first 1024 rows goes through the stage and through the numpy restatement
(tests/iir_zero_phase_cases.py): the backward pass starts at a block's end, so no part of a long block can be restated alone.

    python tools/iir_zero_phase_bench.py [--blocks N] [--runs N] [--parent-lib FILE] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import iir_zero_phase_cases as zc  # noqa: E402
from cases import IIR_BANDPASS  # noqa: E402
from rspt_amd import api, synth  # noqa: E402

MARGIN = 1.25


def one_call_ms(fn, buf, pristine):
    if buf is not None:
        buf.copy_(pristine)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(v):
    return {"ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "runs_ms": [round(x, 4) for x in v]}


def parent_single_stage(path, bps, nch, ns):
    """the single stage through another build of the library: (call(buf), close())"""
    L = api.bind(C.CDLL(path), missing_ok=True)  # (a parent build lacks this build's newer entries)
    h = C.c_void_p()
    assert L.rspt_hip_packer_create(C.byref(h), api.KIND_HZR, bps, nch, ns, 4, 0) == 0
    n, d = (C.c_double * 5)(*IIR_BANDPASS[0]), (C.c_double * 5)(*IIR_BANDPASS[1])

    def call(buf):
        st = torch.cuda.current_stream(buf.device).cuda_stream
        rc = L.rspt_hip_iir_prefilter_batch_dev(h, buf.data_ptr(), buf.numel() // (bps * nch * ns), n, d, 5, 2000, 1, st)
        assert rc == 0, rc

    return call, lambda: L.rspt_hip_packer_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to measure"
    bps, nch, ns, B = 4, 64, 65536, a.blocks
    n, d = IIR_BANDPASS
    pk = api.new_hzr(bps, nch, ns)
    pristine = synth.synth_batch_native(B, nch, ns, bps=bps, ecg=True, device="cuda").reshape(-1)
    buf = torch.empty_like(pristine)
    work_bytes = pk.iir_zero_phase_work_bytes(B)
    work = torch.empty(work_bytes // 8, dtype=torch.float64, device="cuda")
    work2 = torch.empty_like(work)
    if a.parent_lib:
        single, close_parent = parent_single_stage(a.parent_lib, bps, nch, ns)
    else:
        single, close_parent = (lambda b: pk.iir_prefilter_batch(b, n, d, init_nr_samples=2000, per_channel=True)), (lambda: None)

    def zero_phase():
        pk.iir_zero_phase_batch(buf, n, d, init_nr_samples=2000, backward_init_nr_samples=0, work=work)

    def two_forward():
        single(buf)
        single(buf)

    def work_copy_x2():
        work2.copy_(work)
        work.copy_(work2)

    for fn in (zero_phase, two_forward):  # warm-up: code objects
        one_call_ms(fn, buf, pristine)
    one_call_ms(work_copy_x2, None, None)
    ms = {"zero_phase": [], "two_forward": [], "work_copy_x2": []}
    for _ in range(a.runs):
        ms["two_forward"].append(one_call_ms(two_forward, buf, pristine))
        ms["work_copy_x2"].append(one_call_ms(work_copy_x2, None, None))
        ms["zero_phase"].append(one_call_ms(zero_phase, buf, pristine))
    # the stage's answer: the backward pass starts at a block's end, so no part of a 65536-row block can be restated on its own;
    # a block of the batch's first 1024 rows goes through the stage and through the restatement instead
    rows = 1024
    small = api.new_hzr(bps, nch, rows)
    head = pristine[: rows * nch * bps].clone()
    small.iir_zero_phase_batch(head, n, d, init_nr_samples=2000, backward_init_nr_samples=0)
    torch.cuda.synchronize()
    case = dict(bps=bps, nch=nch, ns=rows, nblocks=1, n=list(n), d=list(d), init=2000, binit=0, data=pristine[: rows * nch * bps].cpu().numpy())
    ok = bool(np.array_equal(head.cpu().numpy(), zc.filtered(case)))
    small.close()
    res = {"tool": "tools/iir_zero_phase_bench.py", "device": torch.cuda.get_device_name(0), "shape": {"blocks": B, "nch": nch, "ns": ns, "bps": bps},
           "runs": a.runs, "work_bytes": work_bytes,
           "two_forward_library": "parent build" if a.parent_lib else "this build",
           "zero_phase": summary(ms["zero_phase"]), "two_forward": summary(ms["two_forward"]), "work_copy_x2": summary(ms["work_copy_x2"])}
    bound = MARGIN * (res["two_forward"]["ms"] + res["work_copy_x2"]["ms"])
    res["bound_ms"] = round(bound, 4)
    res["zero_phase_over_bound"] = round(res["zero_phase"]["ms"] / bound, 4)
    res["accepted"] = bool(res["zero_phase"]["ms"] <= bound)
    res["block_of_1024_rows_equals_restatement"] = ok
    close_parent()
    pk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if res["accepted"] and ok else 1


if __name__ == "__main__":
    sys.exit(main())
