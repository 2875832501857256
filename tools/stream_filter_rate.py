#!/usr/bin/env python3
"""Time the carried-state pre-filters (rspt_hip_fir_prefilter_stream_dev, rspt_hip_iir_prefilter_stream_dev)
against the stateless stages of another build of the library -- the parent commit's -- and print one JSON line.

The other build is loaded beside this one in the same process (--parent-lib: a librspt_hip.so built from the parent commit,
bound by api.bind; only its packer_create / destroy and the two stateless entries are called), so that both sides see the same
buffers and their runs alternate: parent, branch, parent, branch, ...  Per side: the median ms per call over the runs and the
spread (max - min).  `margin_ok`: the branch's median is not above the parent's by more than twice the parent's spread.

  FIR   64 x (64 ch x 65536 int32), K in {1, 101, 1001}, in place and out of place: stream mode on a state that has started
        against the parent's stateless call on the same batch (the same multiply-add work, plus the K - 1 rows of the state)
  IIR   the harness's band-pass on 64 ch x 2^20 rows: stream mode on 256 blocks of 4096 against the parent's stateless
        per-channel call on a one-block handle of (64 ch, 2^20) -- the same work on the same lanes; and the time of one
        65536-row block at nch = 12 and 64, the latency a feed that filters block by block sees
Without --parent-lib only the branch's side is timed.  After the timed region the stream result of a fresh state is compared
with this build's stateless result on the one-block handle.

    python tools/stream_filter_rate.py [--parent-lib FILE] [--runs N] [--iters N] [--out FILE]
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

import fir_cases as fc  # noqa: E402
from cases import IIR_BANDPASS  # noqa: E402
from rspt_amd import api, synth  # noqa: E402

_dp = C.POINTER(C.c_double)


class Parent:
    """the stateless entries of another build"""

    def __init__(self, path):
        self.L = api.bind(C.CDLL(path), missing_ok=True)  # (a parent build lacks this build's newer entries)

    def packer(self, bps, nch, ns):
        h = C.c_void_p()
        assert self.L.rspt_hip_packer_create(C.byref(h), api.KIND_HZR, bps, nch, ns, 3, 0) == 0
        return h

    def fir(self, h, src, dst, nblocks, k):
        st = torch.cuda.current_stream().cuda_stream
        assert self.L.rspt_hip_fir_prefilter_batch_dev(h, src.data_ptr(), dst.data_ptr(), nblocks, k.ctypes.data_as(_dp), k.size, st) == 0

    def iir(self, h, buf, nblocks, n, d, init):
        st = torch.cuda.current_stream().cuda_stream
        assert self.L.rspt_hip_iir_prefilter_batch_dev(h, buf.data_ptr(), nblocks, n.ctypes.data_as(_dp), d.ctypes.data_as(_dp), n.size, init, 1, st) == 0


def timed(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def versus(parent_fn, branch_fn, runs, iters):
    """alternating runs -> the summary of both sides"""
    ms = {"parent": [], "branch": []}
    for _ in range(runs):
        if parent_fn is not None:
            ms["parent"].append(timed(parent_fn, iters))
        ms["branch"].append(timed(branch_fn, iters))
    out = {}
    for side, v in ms.items():
        if v:
            out[side + "_ms"] = round(statistics.median(v), 4)
            out[side + "_spread_ms"] = round(max(v) - min(v), 4)
            out[side + "_runs_ms"] = [round(x, 4) for x in v]
    if ms["parent"]:
        out["branch_over_parent"] = round(out["branch_ms"] / out["parent_ms"], 4)
        out["margin_ok"] = bool(out["branch_ms"] <= out["parent_ms"] + 2 * out["parent_spread_ms"])
    return out


def fir_runs(parent, runs, iters, res):
    bps, nch, ns, B = 4, 64, 65536, 64
    pk = api.new_hzr(bps, nch, ns)
    one = api.new_hzr(bps, nch, ns * 4)  # the check: 4 blocks against the stateless stage on one long block
    ph = parent.packer(bps, nch, ns) if parent else None
    pristine = synth.synth_batch_native(B, nch, ns, bps=bps, ecg=True, device="cuda").reshape(-1)
    src, dst = pristine.clone(), torch.empty_like(pristine)
    for K in (1, 101, 1001):
        k = np.ascontiguousarray(fc.windowed_sinc_lowpass(K, 0.05))
        state = pk.fir_state(K)
        for in_place in (False, True):
            out = src if in_place else dst
            r = versus((lambda: parent.fir(ph, src, out, B, k)) if parent else None,
                       lambda: pk.fir_prefilter_batch(src, k, d_dst=None if in_place else dst, state=state), runs, iters)
            src.copy_(pristine)
            a = pk.fir_prefilter_batch(src[: 4 * pk.block_bytes].clone(), k, state=pk.fir_state(K))
            b = one.fir_prefilter_batch(src[: 4 * pk.block_bytes].clone(), k)
            torch.cuda.synchronize()
            r.update(stage="fir", shape="64x(64ch x 65536 i32)", K=K, in_place=in_place, checked_ok=bool(torch.equal(a, b)))
            res.append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
    if parent:
        parent.L.rspt_hip_packer_destroy(ph)
    pk.close()
    one.close()


def iir_runs(parent, runs, iters, res):
    n, d = (np.ascontiguousarray(v, dtype=np.float64) for v in IIR_BANDPASS)
    bps, nch, ns, B = 4, 64, 4096, 256
    pk = api.new_hzr(bps, nch, ns)
    one = api.new_hzr(bps, nch, ns * B)
    ph = parent.packer(bps, nch, ns * B) if parent else None
    pristine = synth.synth_batch_native(B, nch, ns, bps=bps, ecg=True, device="cuda").reshape(-1)
    buf = pristine.clone()
    state = pk.iir_state()
    r = versus((lambda: parent.iir(ph, buf, 1, n, d, 2000)) if parent else None,
               lambda: pk.iir_prefilter_batch(buf, n, d, init_nr_samples=2000, per_channel=True, state=state), runs, iters)
    a = pk.iir_prefilter_batch(pristine.clone(), n, d, init_nr_samples=2000, per_channel=True, state=pk.iir_state())
    b = one.iir_prefilter_batch(pristine.clone(), n, d, init_nr_samples=2000, per_channel=True)
    torch.cuda.synchronize()
    r.update(stage="iir", shape="64ch x 2^20 rows i32 (stream: 256 blocks of 4096)", checked_ok=bool(torch.equal(a, b)))
    res.append(r)
    print(json.dumps(r), file=sys.stderr, flush=True)
    if parent:
        parent.L.rspt_hip_packer_destroy(ph)
    pk.close()
    one.close()
    for nch in (12, 64):  # one 65536-row block per call on a state that has started
        pk = api.new_hzr(4, nch, 65536)
        blk = synth.synth_batch_native(1, nch, 65536, bps=4, ecg=True, device="cuda").reshape(-1)
        state = pk.iir_state()
        r = versus(None, lambda: pk.iir_prefilter_batch(blk, n, d, init_nr_samples=2000, per_channel=True, state=state), runs, iters)
        r.update(stage="iir", shape="one block of %dch x 65536 i32 per call" % nch)
        res.append(r)
        print(json.dumps(r), file=sys.stderr, flush=True)
        pk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to time"
    parent = Parent(a.parent_lib) if a.parent_lib else None
    res = []
    fir_runs(parent, a.runs, a.iters, res)
    iir_runs(parent, a.runs, a.iters, res)
    line = json.dumps(dict(tool="stream_filter_rate", device=torch.cuda.get_device_name(0), runs_per_side=a.runs, iters=a.iters,
                           parent=bool(parent), results=res))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
