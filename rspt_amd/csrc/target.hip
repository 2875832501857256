// target.hip -- compress to a PRDN target (rspt_hip_compress_target_batch_dev): the choice of a ladder entry per block.
//
//   k_target_select   the rule, on the [nladder][nblocks] table of PRDN figures the probes left: block b takes the first entry k
//                     in ladder order with path == 0 and (mse == 0 or prdn <= target) -- a NaN compares false, a figure that
//                     needed the sequential chain (an exact sum above 2^53) never counts -- and the last entry if none does.
#include "common.hpp"

namespace rspt {

__global__ __launch_bounds__(256) void k_target_select(const double* __restrict__ prdn, const double* __restrict__ mse,
                                                      const uint32_t* __restrict__ path, uint32_t nladder, uint32_t nblocks, double target,
                                                      uint32_t* __restrict__ choice, double* __restrict__ prdn_out) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nblocks) return;
    uint32_t pick = nladder - 1u;
    for (uint32_t k = 0; k < nladder; ++k) {
        const size_t at = (size_t)k * nblocks + b;
        if (path[at] == 0u && (mse[at] == 0.0 || prdn[at] <= target)) {
            pick = k;
            break;
        }
    }
    choice[b] = pick;
    const size_t at = (size_t)pick * nblocks + b;
    if (prdn_out) prdn_out[b] = path[at] == 0u ? prdn[at] : __longlong_as_double(0x7FF0000000000000ll);  // (+inf: no exact figure)
}

// ---- the fused probe: hadamard rows of up to kTpMaxNs points, nch * ns < 2^22 ---------------------------------------------------
//   k_target_probe   one workgroup per (channel, block).  The row is read once and kept in registers (kTpPer samples a thread);
//                    its average_32 mean and W = WHT(x - mean) mod 2^32 stay in LDS for every ladder entry.  Per entry k:
//                    y = cut_nb(fwht_quant(W, n / q_k)) into the second LDS buffer, its WHT there, x' = fwht_quant(., q_k) +
//                    mean24 cut to the sample width -- what the inverse kernel and the native back end leave -- and the PRDN terms
//                    of (o, x') into the accumulators of quality.hip (QTerms: the two limbs of sum t^2, sum r, sum |r|), row
//                    [k][block] of a table that k_q_finish then finishes as it finishes a PRDN call's: the same exact sums,
//                    the same conditions, the same code for the figure.  mean24 is the header's 24 bits, sign-extended: the
//                    decoder never sees more.  Under nch * ns < 2^22 every sum r is exact (rspt_hip.h: rspt_hip_prdn_batch_dev).
// LDS word i of a buffer sits at i + (i >> 5): with one spare word per 32 the eight-word and sixteen-word strides of the late
// butterfly rounds (lanes 8 or 16 words apart: 8-way and 2-way on 32 banks) spread over the banks (2-way at most); the rounds
// with strides of 32 words and more stay conflict-free, a wave's 32 consecutive words never straddle a spare.  The second buffer
// starts right behind the first: no instruction reads both.
constexpr uint32_t kTpMaxNs = 8192;
constexpr uint32_t kTpPer = 8;  // samples a thread holds: kTpMaxNs / 1024
__host__ __device__ __forceinline__ uint32_t tp_pad(uint32_t i) { return i + (i >> 5); }

// natural-order WHT of the n = 2^k words of a padded buffer, in place, by the nt threads of the workgroup; three stages at a time
// on eight values in registers as k_fwht takes them (the stages commute exactly in wrap-around arithmetic).  Ends in a barrier.
__device__ __forceinline__ void tp_fwht(uint32_t* sh, uint32_t n, uint32_t tid, uint32_t nt) {
    uint32_t w = n >> 1;
    while (w >= 4) {
        const uint32_t st = w >> 2;
        for (uint32_t q = tid; q < (n >> 3); q += nt) {
            const uint32_t base = ((q & ~(st - 1)) << 3) | (q & (st - 1));
            uint32_t v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = sh[tp_pad(base + i * st)];
#pragma unroll
            for (int d = 4; d >= 1; d >>= 1) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    if (!(i & d)) {
                        const uint32_t x = v[i], y = v[i + d];
                        v[i] = x + y;
                        v[i + d] = x - y;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) sh[tp_pad(base + i * st)] = v[i];
        }
        __syncthreads();
        w >>= 3;
    }
    for (; w >= 1; w >>= 1) {  // the one or two stages left
        for (uint32_t q = tid; q < (n >> 1); q += nt) {
            const uint32_t lo = ((q & ~(w - 1)) << 1) | (q & (w - 1));
            const uint32_t x = sh[tp_pad(lo)], y = sh[tp_pad(lo + w)];
            sh[tp_pad(lo)] = x + y;
            sh[tp_pad(lo + w)] = x - y;
        }
        __syncthreads();
    }
}

// acc: [nladder][nblocks][4] unsigned 64-bit, zero at the launch.  blockDim.x: a multiple of 64 with blockDim.x * kTpPer >= ns.
__global__ __launch_bounds__(1024) void k_target_probe(const int32_t* __restrict__ orig, Geom g, QLadder fwd, QLadder inv, uint32_t nb,
                                                      uint32_t nblocks, unsigned long long* __restrict__ acc) {
    extern __shared__ __attribute__((aligned(16))) int32_t sh_i[];
    __shared__ unsigned long long s_part[16][4];
    uint32_t* W = reinterpret_cast<uint32_t*>(sh_i);
    const uint32_t tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
    const uint32_t c = blockIdx.x, b = blockIdx.y, n = g.ns;
    uint32_t* T = W + tp_pad(n);
    const int32_t* row = orig + (size_t)b * g.N + (size_t)c * n;

    // a block-wide sum of four 64-bit values per thread, for thread 0 .. 3 the total of value tid
    auto block_sum4 = [&](unsigned long long (&v)[4]) -> unsigned long long {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q_wave_sum(v[j]);
        if ((tid & 63u) == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s_part[tid >> 6][j] = v[j];
        }
        __syncthreads();
        unsigned long long s = 0;
        if (tid < 4)
            for (uint32_t w = 0; w < nw; ++w) s += s_part[w][tid];
        __syncthreads();
        return s;
    };

    int32_t o[kTpPer];
    unsigned long long first[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < kTpPer; ++j) {
        const uint32_t i = tid + j * nt;
        o[j] = i < n ? row[i] : 0;
        if (i < n) W[tp_pad(i)] = (uint32_t)o[j];
        first[0] += (unsigned long long)(long long)o[j];
    }
    __shared__ int32_t s_mean;
    {
        const unsigned long long s = block_sum4(first);  // (its first barrier also covers the stores to W)
        if (tid == 0) s_mean = mean_from_sum((long long)s, n);
    }
    __syncthreads();
    const int32_t mean = s_mean;
    tp_fwht(W, n, tid, nt);
    if (tid == 0) W[0] -= (uint32_t)mean * n;  // WHT(x - m) = WHT(x) - m*n*delta_0 (exact mod 2^32)
    __syncthreads();

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
        for (uint32_t i = tid; i < n; i += nt) {
            const int32_t y = fwht_quant((int32_t)W[tp_pad(i)], dfwd);
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
}

}  // namespace rspt
