#!/usr/bin/env python3
"""Generate tests/golden/dct_fft_exact_record.json: what the long-double reference of tests/dct_fft_cases.py says about every
case the FFT kernels are held to -- CPU only, no reference tree, no GPU.  Per case (the largest over its blocks):
  fwd_share / inv_share      share of the reference's values inside the comparator's band (dct_fft_cases.band_of)
  fwd_err_eps / inv_err_eps  largest difference between scipy's fp64 DCT and its long-double DCT, in units of eps * max|v| of the row
  fwd_digest / inv_digest    per block, a digest of trunc(v)
  inverse_share_not_run      for a case without an inverse leg whose inverse was measured all the same: why it has none
The inverse is taken of the reference's own truncated coefficients and 24-bit means.  A case whose share exceeds the cap is not
written: the script stops.

    python tests/golden/make_dct_fft_exact_record.py
"""
import numpy as np
import refrecord

refrecord.repo_paths()

import dct_fft_cases as dc  # noqa: E402


def err_eps(v64, v):
    a = np.abs(v)
    return float((np.abs(v64.astype(dc.LD) - v).max(axis=1) / (a.max(axis=1) * dc.LD(dc.EPS))).max())


def measure(c):
    e = {"name": c["name"], "src": c["src"], "bps": c["bps"], "nch": c["nch"], "ns": c["ns"], "nblocks": c["nblocks"], "q": c["q"], "nb": c["nb"],
         "fwd_share": 0.0, "fwd_err_eps": 0.0, "fwd_digest": []}
    inv = c["inverse"] or c["src"] == "full"
    if inv:
        e.update(inv_share=0.0, inv_err_eps=0.0, inv_digest=[])
    for i in range(c["nblocks"]):
        x = dc.block_i32(c, i)
        v, means = dc.exact_forward(x, c["ns"], c["q"])
        e["fwd_share"] = max(e["fwd_share"], float(dc.band_of(v).mean()))
        e["fwd_err_eps"] = max(e["fwd_err_eps"], err_eps(dc.fp64_forward(x, c["ns"], c["q"]), v))
        e["fwd_digest"].append(dc.digest(v))
        if inv:
            co = np.trunc(v).astype(np.int64).astype(np.int32)
            w = dc.exact_inverse(co, dc.means24_of(means), c["ns"], c["q"])
            e["inv_share"] = max(e["inv_share"], float(dc.band_of(w).mean()))
            e["inv_err_eps"] = max(e["inv_err_eps"], err_eps(dc.fp64_inverse(co, c["ns"], c["q"]), w))
            e["inv_digest"].append(dc.digest(w))
    assert e["fwd_share"] <= dc.CAP, (c["name"], e["fwd_share"])
    if inv and not c["inverse"]:
        e["inverse_share_not_run"] = e.pop("inv_share")
        del e["inv_digest"], e["inv_err_eps"]
    elif inv:
        assert e["inv_share"] <= dc.CAP, (c["name"], e["inv_share"])
    return e


def main():
    out = {"generator": "tests/golden/make_dct_fft_exact_record.py (numpy long double through scipy.fft.dct; CPU only)",
           "band": "2^14 * 2^-52 * max|v| of a row, around the non-zero integers", "cap": dc.CAP, "cases": []}
    for c in dc.all_cases():
        e = measure(c)
        out["cases"].append(e)
        print("%-26s fwd share %.3g err %.2f eps%s" % (c["name"], e["fwd_share"], e["fwd_err_eps"],
              "  inv share %.3g err %.2f eps" % (e["inv_share"], e["inv_err_eps"]) if "inv_share" in e else
              "  (inverse not run: share %.3g)" % e["inverse_share_not_run"] if "inverse_share_not_run" in e else ""), flush=True)
    refrecord.write_record("dct_fft_exact_record.json", out)


if __name__ == "__main__":
    main()
