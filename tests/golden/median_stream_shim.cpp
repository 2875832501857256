// median_stream_shim.cpp -- drives the reference's rolling_window_median<double> (lib_rspt/lib_stat/rolling_window_median.h) as a
// user does who receives a recording in blocks, for tests/golden/make_median_stream_record.py: one object per channel that
// lives across the blocks, insert((double)x) on every sample of every block in order, (int32_t) of every result.
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <deque>
#include <iterator>
#include <new>
#include <set>
#include <vector>

#include "rolling_window_median.h"

// x, y: [nblocks][ns][nch] int32 (interleaved blocks, back to back)
extern "C" void median_stream_shim_run(const int32_t* x, int32_t* y, int nch, int ns, int nblocks, size_t window) {
    std::vector<rolling_window_median<double>*> rwm;
    for (int c = 0; c < nch; ++c) rwm.push_back(new rolling_window_median<double>(window));
    for (int b = 0; b < nblocks; ++b) {
        const int32_t* xb = x + (size_t)b * ns * nch;
        int32_t* yb = y + (size_t)b * ns * nch;
        for (int t = 0; t < ns; ++t)
            for (int c = 0; c < nch; ++c) yb[(size_t)t * nch + c] = (int32_t)rwm[c]->insert((double)xb[(size_t)t * nch + c]);
    }
    for (int c = 0; c < nch; ++c) delete rwm[c];
}
