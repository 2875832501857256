// median_shim.cpp -- drives the reference's rolling_window_median<double> (lib_rspt/lib_stat/rolling_window_median.h) as the
// GPU stage restates it, for tests/golden/make_median_record.py: one fresh object per channel, insert((double)x) on every
// sample, (int32_t) of every result.  ref20_run drives it as the reference's own test does and returns the doubles.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <deque>
#include <iterator>
#include <new>
#include <set>
#include <vector>

#include "rolling_window_median.h"

// x, y: [ns][nch] int32 (interleaved)
extern "C" void median_shim_run(const int32_t* x, int32_t* y, int nch, int ns, size_t window) {
    for (int c = 0; c < nch; ++c) {
        rolling_window_median<double> rwm(window);
        for (int t = 0; t < ns; ++t) y[(size_t)t * nch + c] = (int32_t)rwm.insert((double)x[(size_t)t * nch + c]);
    }
}

extern "C" void median_shim_doubles(const double* x, double* y, int n, size_t window) {
    rolling_window_median<double> rwm(window);
    for (int t = 0; t < n; ++t) y[t] = rwm.insert(x[t]);
}
