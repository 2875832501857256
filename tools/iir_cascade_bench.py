#!/usr/bin/env python3
"""Time the IIR cascade stage (rspt_hip_iir_cascade_batch_dev) against the same sections run as successive calls
of the single-section stage (rspt_hip_iir_prefilter_batch_dev, per_channel = 1), and print one JSON line.

On 64 x (64 ch x 65536 int32), for the README's pair (HP 0.4 Hz, then LP 100 Hz: S = 2) and a four-section chain (the pair, the
harness's band-pass, an order-3 low-pass: S = 4), in one process, alternating:
    cascade      one call of the cascade stage
    successive   S calls of the single-section stage with the same sections (NOT the same answer: every call truncates)
    successive_init2000   the same S calls with init_nr_samples = 2000 in every one, for information: a section whose
                 init_nr_samples is 0 sends the single-section stage to its one-thread-per-channel kernel (k_iir), this
                 variant keeps every call on its pipelined kernel (k_iir_pipe)
Every timed call starts from the same pristine batch (copied back outside the timed region) and is timed with device events;
per side the median ms over the runs and the spread (max - min).  `no_slower`: the cascade's median is not above the
successive calls' median.  After the timed region the head of block 0 of the cascade's result is compared with the numpy
restatement (tests/iir_cascade_cases.py).

    python tools/iir_cascade_bench.py [--blocks N] [--runs N] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import iir_cascade_cases as cc  # noqa: E402
import iir_cases as ic  # noqa: E402
from cases import IIR_BANDPASS  # noqa: E402
from rspt_amd import api, synth  # noqa: E402

SINGLE_STAGE_MS = 2.5  # the single-section stage on this batch (README.md)

CHAINS = {
    "readme_pair_s2": cc.README_PAIR,
    "four_sections_s4": cc.README_PAIR + [(IIR_BANDPASS[0], IIR_BANDPASS[1], 0, False), (ic.STABLE[4][0], ic.STABLE[4][1], 0, False)],
}


def one_call_ms(fn, buf, pristine):
    buf.copy_(pristine)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def summary(v):
    return {"ms": round(statistics.median(v), 4), "spread_ms": round(max(v) - min(v), 4), "runs_ms": [round(x, 4) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert api.lib().rspt_hip_device_count() > 0, "no gfx950 device: nothing to measure"
    bps, nch, ns, B = 4, 64, 65536, a.blocks
    pk = api.new_hzr(bps, nch, ns)
    pristine = synth.synth_batch_native(B, nch, ns, bps=bps, ecg=True, device="cuda").reshape(-1)
    buf = torch.empty_like(pristine)
    res = {"tool": "tools/iir_cascade_bench.py", "device": torch.cuda.get_device_name(0), "shape": {"blocks": B, "nch": nch, "ns": ns, "bps": bps},
           "runs": a.runs, "single_stage_ms": SINGLE_STAGE_MS, "chains": {}}
    for name, sections in CHAINS.items():
        S = len(sections)

        def cascade():
            pk.iir_cascade_batch(buf, sections)

        def successive():
            for n, d, init, _ in sections:
                pk.iir_prefilter_batch(buf, n, d, init_nr_samples=init, per_channel=True)

        def successive_init2000():
            for n, d, _, _ in sections:
                pk.iir_prefilter_batch(buf, n, d, init_nr_samples=2000, per_channel=True)

        for fn in (cascade, successive, successive_init2000):  # warm-up: code objects
            one_call_ms(fn, buf, pristine)
        ms = {"cascade": [], "successive": [], "successive_init2000": []}
        for _ in range(a.runs):
            ms["successive"].append(one_call_ms(successive, buf, pristine))
            ms["successive_init2000"].append(one_call_ms(successive_init2000, buf, pristine))
            ms["cascade"].append(one_call_ms(cascade, buf, pristine))
        # the cascade's answer (buf holds it): the head of block 0 against the restatement
        rows = 1024
        got = buf[: rows * nch * bps].cpu().numpy()
        head = dict(bps=bps, nch=nch, ns=rows, nblocks=1, sections=sections, data=pristine[: rows * nch * bps].cpu().numpy())
        ok = bool(np.array_equal(got, cc.filtered(head, "stateless")))
        r = {"sections": S, "cascade": summary(ms["cascade"]), "successive": summary(ms["successive"]),
             "successive_init2000": summary(ms["successive_init2000"])}
        r["cascade_over_successive"] = round(r["cascade"]["ms"] / r["successive"]["ms"], 4)
        r["cascade_over_successive_init2000"] = round(r["cascade"]["ms"] / r["successive_init2000"]["ms"], 4)
        r["cascade_ms_per_section"] = round(r["cascade"]["ms"] / S, 4)
        r["no_slower"] = bool(r["cascade"]["ms"] <= r["successive"]["ms"])
        r["head_of_block0_equals_restatement"] = ok
        res["chains"][name] = r
    pk.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if all(r["no_slower"] and r["head_of_block0_equals_restatement"] for r in res["chains"].values()) else 1


if __name__ == "__main__":
    sys.exit(main())
