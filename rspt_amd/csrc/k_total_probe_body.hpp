// The body of k_total_probe and k_planar_total_probe (total.hip), included into both so that the native kernel stays the code that
// was timed.  From the kernel: orig, g, fwd, inv, nb, nblocks, slots, acc and the constant kPlanarCut (k_target_probe_body.hpp).  Per ladder entry it is k_budget_probe_body.hpp's store
// and k_target_probe_body.hpp's round trip on ONE fwht_quant(W, n / q_k): the coefficient goes to its slot as it is and, cut to nb
// bytes, into the second LDS buffer.  The native kernel's orig may lie inside slots (k_budget_probe): the row is in o[] and in W,
// behind a barrier, before the first store to a slot.
#include "k_tp_transform_body.hpp"

    // the reference terms once: r = (int32)((o - mean) * (o - mean)), their sum and the sum of their magnitudes
    long long sr = 0;
    unsigned long long sa = 0;
#pragma unroll
    for (uint32_t j = 0; j < kTpPer; ++j) {
        if (tid + j * nt < n) {
            int32_t t, r;
            q_terms(o[j], o[j], mean, t, r);
            sr += r;
            sa += (unsigned long long)(r < 0 ? -(long long)r : (long long)r);
        }
    }
    const int32_t mean24 = (int32_t)((uint32_t)mean << 8) >> 8;  // what the header keeps (load_mean_hdr)
    const uint32_t sx_nb = 32u - 8u * nb, sx = 32u - 8u * g.bps;
    for (uint32_t k = 0; k < fwd.n; ++k) {
        const double dfwd = fwd.a[k], dinv = inv.a[k];
        int32_t* out = slots + ((size_t)k * nblocks + b) * g.N + (size_t)c * n;
        for (uint32_t i = tid; i < n; i += nt) {
            const int32_t y = fwht_quant((int32_t)W[tp_pad(i)], dfwd);
            out[i] = y;  // what k_fwht_l leaves for a block of choice k
            T[tp_pad(i)] = (uint32_t)((int32_t)((uint32_t)y << sx_nb) >> sx_nb);  // the low nb bytes, sign-extended: what the planes keep
        }
        __syncthreads();
        tp_fwht(T, n, tid, nt);
        QTerms q;
#pragma unroll
        for (uint32_t j = 0; j < kTpPer; ++j) {
            const uint32_t i = tid + j * nt;
            if (i < n) {
                int32_t x = fwht_quant((int32_t)T[tp_pad(i)], dinv);
                x = (int32_t)((uint32_t)x + (uint32_t)mean24);
                x = (int32_t)((uint32_t)x << sx) >> sx;  // the cut to the sample width (k_planar_emit, the native back ends)
                q.add(o[j], x, mean);
            }
        }
        unsigned long long v[4] = {q.lo, q.hi, (unsigned long long)sr, sa};
        const unsigned long long s = block_sum4(v);  // (its last barrier: every read of T is done before the next entry's stores)
        if (tid < 4 && s) atomicAdd(&acc[((size_t)k * nblocks + b) * 4 + tid], s);
    }
