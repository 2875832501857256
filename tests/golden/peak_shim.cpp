// peak_shim.cpp -- drives the reference's R-peak detectors (lib_rspt/peak_detector.h) and its filter designer
// (lib_rspt/lib_filter/iir_filter_design.cpp, create_filter_iir) as the GPU stage restates them, for
// tests/golden/make_peak_record.py.  Every detector is fed (double) of each int32 sample.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>
using namespace std;  // (the reference's headers name vector unqualified)

#include "filter.h"
#include "iir_filter_opt.h"
#include "peak_detector.h"

// create_filter_iir into num / den (5 doubles each); returns the coefficient count, or -1 where it returns false
extern "C" int peak_shim_design(int type, int order, double fs, double lo, double hi, double* num, double* den) {
    vector<double> n, d;
    if (!create_filter_iir(n, d, butterworth, (filter_type)type, order, fs, lo, hi)) return -1;
    for (size_t i = 0; i < n.size(); ++i) num[i] = n[i];
    for (size_t i = 0; i < d.size(); ++i) den[i] = d[i];
    return (int)n.size();
}

// x: [nblocks][ns][nch] int32.  ret, sig, thr: [nblocks][ns][nch] doubles -- what detect() returns (for the offline object:
// peak_signal) and its peak_sample / threshold_sample (filt_signal / threshold_signal).  variant: 0 peak_detector::detect,
// 1 peak_detector_1st_order::detect, 2 peak_detector_offline::detect_fw (one call per block).  stateful != 0: one detector per
// channel runs through the blocks in order; else a fresh one per (block, channel).
template <class D>
static void run_online(const int32_t* x, int nblocks, int nch, int ns, double fs, double marker, int stateful, double* ret, double* sig,
                       double* thr) {
    for (int c = 0; c < nch; ++c) {
        D* det = nullptr;
        for (int b = 0; b < nblocks; ++b) {
            if (!det || !stateful) {
                delete det;
                det = new D(fs, marker);
            }
            for (int t = 0; t < ns; ++t) {
                const size_t i = ((size_t)b * ns + t) * nch + c;
                ret[i] = det->detect((double)x[i], &sig[i], &thr[i]);
            }
        }
        delete det;
    }
}

static void run_offline_fw(const int32_t* x, int nblocks, int nch, int ns, double fs, double marker, int stateful, double* ret, double* sig,
                           double* thr) {
    vector<double> in(ns), p(ns), f(ns), th(ns);
    for (int c = 0; c < nch; ++c) {
        peak_detector_offline* det = nullptr;
        for (int b = 0; b < nblocks; ++b) {
            if (!det || !stateful) {
                delete det;
                det = new peak_detector_offline(fs, marker);
            }
            for (int t = 0; t < ns; ++t) in[t] = (double)x[((size_t)b * ns + t) * nch + c];
            det->detect_fw(in.data(), (unsigned)ns, p.data(), f.data(), th.data());
            for (int t = 0; t < ns; ++t) {
                const size_t i = ((size_t)b * ns + t) * nch + c;
                ret[i] = p[t];
                sig[i] = f[t];
                thr[i] = th[t];
            }
        }
        delete det;
    }
}

extern "C" void peak_shim_run(int variant, const int32_t* x, int nblocks, int nch, int ns, double fs, double marker, int stateful, double* ret,
                              double* sig, double* thr) {
    if (variant == 0) run_online<peak_detector>(x, nblocks, nch, ns, fs, marker, stateful, ret, sig, thr);
    else if (variant == 1) run_online<peak_detector_1st_order>(x, nblocks, nch, ns, fs, marker, stateful, ret, sig, thr);
    else run_offline_fw(x, nblocks, nch, ns, fs, marker, stateful, ret, sig, thr);
}
