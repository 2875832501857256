// The body of k_budget_probe and k_planar_budget_probe (budget.hip), included into both so that the native kernel stays the code
// that was timed.  From the kernel: orig, g, fwd, nblocks, slots and the constant kPlanarCut -- true: orig is the caller's matrix
// and each value is cut to the sample width as it is loaded (k_target_probe_body.hpp); false: orig holds what the converter
// wrote, which is cut already.
#include "k_tp_transform_body.hpp"
    for (uint32_t k = 0; k < fwd.n; ++k) {
        const double dfwd = fwd.a[k];
        int32_t* out = slots + ((size_t)k * nblocks + b) * g.N + (size_t)c * n;
        for (uint32_t i = tid; i < n; i += nt) out[i] = fwht_quant((int32_t)W[tp_pad(i)], dfwd);
    }
