// iir_cascade_shim.cpp -- drives the reference's IIR filters the way a user who chains them drives them, for
// tests/golden/make_iir_cascade_record.py: per channel S objects i_filter::new_iir(n_k, d_k, nc_k), every one initialised with
// init_history_values on the channel's RAW first sample, then per sample v = x; v = f_k->filter(v) or f_k->filter_opt(v) for
// k = 0 .. S-1; y = (int32_t)v.  carry != 0: one chain per channel living on from block to block; carry == 0: a fresh chain for
// every block.  Only i_filter::new_iir / init_history_values / filter / filter_opt / delete_iir are used.
#include <stddef.h>
#include <stdint.h>

#include <vector>
using namespace std;  // (filter.h names vector unqualified, as the reference's own sources expect)

#include "filter.h"

// x, y: nblocks blocks of [ns][nch] int32 (interleaved), back to back.  n, d: 5 * nsections doubles, section k at 5k, nc[k] of
// them used; init[k] = init_nr_samples; use_filter[k] != 0: filter() instead of filter_opt().
extern "C" void iir_cascade_shim_run(const int32_t* x, int32_t* y, int nch, int ns, int nblocks, int nsections, const double* n, const double* d,
                                     const uint32_t* nc, const int32_t* init, const uint8_t* use_filter, int carry) {
    vector<i_filter*> f((size_t)nch * nsections, (i_filter*)0);
    for (int blk = 0; blk < nblocks; ++blk) {
        const int32_t* xb = x + (size_t)blk * ns * nch;
        int32_t* yb = y + (size_t)blk * ns * nch;
        for (int c = 0; c < nch; ++c) {
            i_filter** fc = &f[(size_t)c * nsections];
            if (blk == 0 || !carry) {
                for (int k = 0; k < nsections; ++k) {
                    if (fc[k]) i_filter::delete_iir(fc[k]);
                    fc[k] = i_filter::new_iir(n + 5 * k, d + 5 * k, nc[k]);
                    fc[k]->init_history_values((double)xb[c], init[k]);
                }
            }
            for (int t = 0; t < ns; ++t) {
                double v = (double)xb[(size_t)t * nch + c];
                for (int k = 0; k < nsections; ++k) v = use_filter[k] ? fc[k]->filter(v) : fc[k]->filter_opt(v);
                yb[(size_t)t * nch + c] = (int32_t)v;
            }
        }
    }
    for (size_t i = 0; i < f.size(); ++i) i_filter::delete_iir(f[i]);
}
