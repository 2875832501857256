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
    constexpr bool kPlanarCut = false;
#include "k_target_probe_body.hpp"
}

// k_planar_target_probe: the probe of rspt_hip_compress_target_planar_batch_dev -- the rows are the caller's matrix (single dwords
// at tid + j * nt: its 4-byte alignment is all they need), cut to the sample width on load
__global__ __launch_bounds__(1024) void k_planar_target_probe(const int32_t* __restrict__ orig, Geom g, QLadder fwd, QLadder inv, uint32_t nb,
                                                             uint32_t nblocks, unsigned long long* __restrict__ acc) {
    constexpr bool kPlanarCut = true;
#include "k_target_probe_body.hpp"
}

}  // namespace rspt
