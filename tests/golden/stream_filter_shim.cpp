// stream_filter_shim.cpp -- drives the reference's filters the way a user with a recording that arrives in blocks drives them, for
// tests/golden/make_stream_filter_record.py: one i_filter per channel, init_history_values once on the channel's first sample,
// then filter_opt on every sample of every block in order, the object living on from block to block.  Only i_filter::new_iir /
// new_fir / init_history_values / filter_opt / delete_iir / delete_fir are used.
#include <stddef.h>
#include <stdint.h>

#include <vector>
using namespace std;  // (filter.h names vector unqualified, as the reference's own sources expect)

#include "filter.h"

// x, y: nblocks blocks of [ns][nch] int32 (interleaved), back to back.  fir != 0: a = the kernel of `count` taps (b unused);
// else a = n, b = d, `count` coefficients each, init = init_nr_samples.
extern "C" void stream_filter_shim_run(const int32_t* x, int32_t* y, int nch, int ns, int nblocks, int fir, const double* a, const double* b,
                                       size_t count, int init) {
    vector<i_filter*> f(nch);
    for (int c = 0; c < nch; ++c) {
        f[c] = fir ? i_filter::new_fir(a, count) : i_filter::new_iir(a, b, count);
        f[c]->init_history_values((double)x[c], init);
    }
    for (int blk = 0; blk < nblocks; ++blk) {
        const int32_t* xb = x + (size_t)blk * ns * nch;
        int32_t* yb = y + (size_t)blk * ns * nch;
        for (int c = 0; c < nch; ++c)
            for (int t = 0; t < ns; ++t) yb[(size_t)t * nch + c] = (int32_t)f[c]->filter_opt((double)xb[(size_t)t * nch + c]);
    }
    for (int c = 0; c < nch; ++c) {
        if (fir) i_filter::delete_fir(f[c]);
        else i_filter::delete_iir(f[c]);
    }
}
