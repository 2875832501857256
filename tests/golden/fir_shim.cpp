// fir_shim.cpp -- drives the reference's FIR filter the way its test harness drives a filter (lib_rspt_test/rspt_test.cpp:116-136),
// for tests/golden/make_fir_record.py.  Only i_filter::new_fir / init_history_values / filter_opt / delete_fir are used.
#include <stddef.h>
#include <stdint.h>

#include <vector>
using namespace std;  // (filter.h names vector unqualified, as the reference's own sources expect)

#include "filter.h"

// x, y: [ns][nch] int32 (interleaved).  shared != 0: one filter object for all channels, as in the harness; else one per channel.
extern "C" void fir_shim_run(const int32_t* x, int32_t* y, int nch, int ns, const double* kernel, size_t kernel_size, int shared) {
    i_filter* f = shared ? i_filter::new_fir(kernel, kernel_size) : nullptr;
    for (int c = 0; c < nch; ++c) {
        if (!shared) f = i_filter::new_fir(kernel, kernel_size);
        f->init_history_values((double)x[c], ns);
        for (int t = 0; t < ns; ++t) y[(size_t)t * nch + c] = (int32_t)f->filter_opt((double)x[(size_t)t * nch + c]);
        if (!shared) i_filter::delete_fir(f);
    }
    if (shared) i_filter::delete_fir(f);
}
