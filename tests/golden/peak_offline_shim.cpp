// peak_offline_shim.cpp -- drives the reference's zero-phase offline R-peak detector (peak_detector_offline::detect of
// lib_rspt/peak_detector.h) as the GPU stage restates it, for tests/golden/make_peak_offline_record.py.  Every object is fed
// (double) of each int32 sample, and detect() is called with peak_indexes = nullptr.
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <cmath>
#include <vector>
using namespace std;  // (the reference's headers name vector unqualified)

#include "filter.h"
#include "iir_filter_opt.h"
#include "peak_detector.h"

// x: [nblocks][ns][nch] int32.  ret, sig, thr: [nblocks][ns][nch] doubles -- peak_signal, filt_signal and threshold_signal of
// each call.  stateful != 0: one object per channel runs through the blocks in order, block b taking detect_fw where
// calls[b] is 1 and detect where it is 0 (calls may be NULL: all detect); else a fresh object per (block, channel) and detect.
extern "C" void peak_offline_shim_run(const int32_t* x, int nblocks, int nch, int ns, double fs, double marker, int stateful, const int* calls,
                                      double* ret, double* sig, double* thr) {
    vector<double> in(ns), p(ns), f(ns), th(ns);
    for (int c = 0; c < nch; ++c) {
        peak_detector_offline* det = nullptr;
        for (int b = 0; b < nblocks; ++b) {
            if (!det || !stateful) {
                delete det;
                det = new peak_detector_offline(fs, marker);
            }
            for (int t = 0; t < ns; ++t) in[t] = (double)x[((size_t)b * ns + t) * nch + c];
            if (stateful && calls && calls[b]) det->detect_fw(in.data(), (unsigned)ns, p.data(), f.data(), th.data());
            else det->detect(in.data(), (unsigned)ns, p.data(), f.data(), th.data(), nullptr);
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
