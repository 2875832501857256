// iir_zero_phase_shim.cpp -- drives the reference's IIR filter forward and then backward over the SAME object, the way
// peak_detector_offline::detect drives its filters, for tests/golden/make_iir_zero_phase_record.py: per (block, channel) one
// fresh object f = i_filter::new_iir(n, d, nc),
//     f->init_history_values((double)x[0], init);           for t = 0 .. ns-1:  w[t] = f->filter_opt((double)x[t]);
//     f->init_history_values(w[ns-1], backward_init);       for t = ns-1 .. 0:  w[t] = f->filter_opt(w[t]);
//     y[t] = (int32_t)w[t]
// Only i_filter::new_iir / init_history_values / filter_opt / delete_iir are used.
#include <stddef.h>
#include <stdint.h>

#include <vector>
using namespace std;  // (filter.h names vector unqualified, as the reference's own sources expect)

#include "filter.h"

// x, y: nblocks blocks of [ns][nch] int32 (interleaved), back to back.  n, d: nc doubles each.
extern "C" void iir_zero_phase_shim_run(const int32_t* x, int32_t* y, int nch, int ns, int nblocks, const double* n, const double* d, int nc, int init,
                                        int backward_init) {
    vector<double> w((size_t)ns);
    for (int blk = 0; blk < nblocks; ++blk) {
        const int32_t* xb = x + (size_t)blk * ns * nch;
        int32_t* yb = y + (size_t)blk * ns * nch;
        for (int c = 0; c < nch; ++c) {
            i_filter* f = i_filter::new_iir(n, d, (size_t)nc);
            f->init_history_values((double)xb[c], init);
            for (int t = 0; t < ns; ++t) w[t] = f->filter_opt((double)xb[(size_t)t * nch + c]);
            f->init_history_values(w[ns - 1], backward_init);
            for (int t = ns - 1; t >= 0; --t) w[t] = f->filter_opt(w[t]);
            for (int t = 0; t < ns; ++t) yb[(size_t)t * nch + c] = (int32_t)w[t];
            i_filter::delete_iir(f);
        }
    }
}
