// budget.hip -- compress to a byte budget (rspt_hip_compress_budget_batch_dev and its planar form,
// rspt_hip_compress_budget_planar_batch_dev): the finest ladder entry whose stream fits, per block.
//
//   k_budget_sizes    one wave per block slot: the stream size k_layout would name for the slot, from what k_tree left --
//                     1 + hdr_len + 8 nb + the sum over the slot's nb * nblk hzr blocks of (7 + payload_len).  No byte of a stream
//                     is written for it.
//   k_budget_select   the rule, on the [nladder][nblocks] table of those sizes: block b takes the HIGHEST entry k with
//                     size_k(b) <= budget(b), and where no entry fits the smallest one, the lowest index among equals.
//   k_budget_probe    the batched route's front end (hadamard rows of up to kTpMaxNs points): one workgroup per (channel, block)
//                     reads the row once, takes its mean and W = WHT(x - mean) once (k_tp_transform_body.hpp, the transform of
//                     k_target_probe) and writes, per ladder entry k, fwht_quant(W, n / q_k) -- the coefficients k_fwht_l leaves
//                     for a block of choice k -- as row c of block slot k * nblocks + b of the planar workspace.
//   k_planar_budget_probe  the same body (k_budget_probe_body.hpp) for rspt_hip_compress_budget_planar_batch_dev: the rows come
//                     from the caller's [nblocks][nch][ns] int32 matrix, cut to the sample width as they are loaded.
#include "common.hpp"

namespace rspt {

// sizes: [nslots].  Slot s of a candidate pass is block s; of the batched pass, entry s / nblocks of block s % nblocks.
__global__ __launch_bounds__(64) void k_budget_sizes(Geom g, const uint32_t* __restrict__ nbuse, const BlockMeta* __restrict__ meta,
                                                    unsigned long long* __restrict__ sizes) {
    const uint32_t s = blockIdx.x, l = threadIdx.x;
    const uint32_t nb = nbuse[s], n = nb * g.nblk;  // hzr blocks of this slot, (k, j) order: what k_layout sums
    const uint32_t hb0 = hb_index(g, s, 0, 0);
    unsigned long long sum = 0;
    for (uint32_t q = l; q < n; q += 64u) sum += 7ull + meta[hb0 + q].payload_len;
    sum = q_wave_sum(sum);
    if (l == 0) sizes[s] = 1ull + g.hdr_len + 8ull * nb + sum;
}

// budget: one limit per block, or nullptr: budget_all for every block.  cand: nullptr, or where the table is copied to.
__global__ __launch_bounds__(256) void k_budget_select(const unsigned long long* __restrict__ tab, uint32_t nladder, uint32_t nblocks,
                                                      unsigned long long budget_all, const unsigned long long* __restrict__ budget,
                                                      uint32_t* __restrict__ choice, unsigned long long* __restrict__ cand) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nblocks) return;
    const unsigned long long limit = budget ? budget[b] : budget_all;
    uint32_t pick = nladder, least = 0;
    unsigned long long least_size = tab[b];
    for (uint32_t k = 0; k < nladder; ++k) {
        const size_t at = (size_t)k * nblocks + b;
        const unsigned long long s = tab[at];
        if (cand) cand[at] = s;
        if (s <= limit) pick = k;
        if (s < least_size) least_size = s, least = k;
    }
    choice[b] = pick < nladder ? pick : least;
}

// orig: the blocks as the converter wrote them, [nblocks][nch][ns] int32; slots: [fwd.n * nblocks][nch][ns].  orig may lie inside
// slots, as the rows of the blocks of one entry: a workgroup has read its row into LDS, behind a barrier, before it writes the
// same row of any slot, and no other workgroup touches that row (neither pointer is __restrict__ for it).
// blockDim.x: a multiple of 64 with blockDim.x * kTpPer >= ns; dynamic LDS: tp_pad(ns) words.
__global__ __launch_bounds__(1024) void k_budget_probe(const int32_t* orig, Geom g, QLadder fwd, uint32_t nblocks, int32_t* slots) {
    constexpr bool kPlanarCut = false;
#include "k_budget_probe_body.hpp"
}

// k_planar_budget_probe: the probe of rspt_hip_compress_budget_planar_batch_dev -- the rows are the caller's matrix (single dwords
// at tid + j * nt: its 4-byte alignment is all they need), cut to the sample width on load.  orig is only read and lies outside
// slots: nothing but this kernel reads the matrix, and every slot of every entry is written from LDS.
__global__ __launch_bounds__(1024) void k_planar_budget_probe(const int32_t* __restrict__ orig, Geom g, QLadder fwd, uint32_t nblocks,
                                                             int32_t* __restrict__ slots) {
    constexpr bool kPlanarCut = true;
#include "k_budget_probe_body.hpp"
}

}  // namespace rspt
