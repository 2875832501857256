// total.hip -- compress a batch to one byte total (rspt_hip_compress_total_batch_dev and its planar form,
// rspt_hip_compress_total_planar_batch_dev): the lowest common PRDN level whose picks fit.
//
//   k_total_probe   the fused route's front end (hadamard rows of up to kTpMaxNs points, nch * ns < 2^22): one workgroup per
//                   (channel, block) reads the row once and does, per ladder entry, what k_budget_probe does -- the entry's
//                   coefficients into row c of block slot k * nblocks + b -- and what k_target_probe does -- the round trip in the
//                   second LDS buffer and the exact PRDN sums into acc (k_total_probe_body.hpp).
//   k_planar_total_probe  the same body for rspt_hip_compress_total_planar_batch_dev: the rows come from the caller's
//                   [nblocks][nch][ns] int32 matrix, cut to the sample width as they are loaded.
//   k_total_figs    the figure of every (entry, block) as the bit pattern of a double: +0.0 where mse == 0, the PRDN where the entry
//                   is rated, kTotalNaN where it is not.  A rated figure is never negative (100 * sqrt of a quotient whose numerator
//                   is > 0: positive, +inf or a NaN), so figures and levels order as their patterns do, and kTotalNaN lies above
//                   every level.
//   k_total_level   the rule's level, by ONE workgroup: T* is the smallest pattern in [0, kTotalInf] at which every rated block has
//                   a pick and the picks' sizes add up to at most total_bytes, found by bisection -- both conditions are monotone in
//                   the pattern, and since they change at figures only, the smallest such pattern is a figure.  A round is one pass
//                   over the blocks (the first blockDim.x of them stay in registers) and one block-wide reduction of (cost, a block
//                   without a pick): 64-bit integer sums and flags, so no launch shape changes a result.
//   k_total_round   one round of that bisection by the whole grid, for batches of more than kTotalWide blocks, where one workgroup's
//                   pass over the table is the slow part: the host launches kTotalRounds of them, the stream orders them.
//   k_total_pick    pick_{T*}(b) per block: the rated entry of smallest size among those with a figure <= T*, the lowest index
//                   among equals; an unrated block its smallest stream.  Also d_prdn, d_level, d_total and the copies of the tables.
#include "common.hpp"

namespace rspt {

constexpr unsigned long long kTotalInf = 0x7FF0000000000000ull;  // +inf: the highest level
constexpr unsigned long long kTotalNaN = 0x7FF8000000000000ull;  // an unrated entry's figure
constexpr unsigned long long kTotalNone = ~0ull;                 // no size: an entry beyond the ladder, no pick yet

// slots: [fwd.n * nblocks][nch][ns]; orig may lie inside it, as the rows of the blocks of one entry (k_budget_probe).
// acc: [nladder][nblocks][4] unsigned 64-bit, zero at the launch.  blockDim.x: a multiple of 64 with blockDim.x * kTpPer >= ns;
// dynamic LDS: 2 * tp_pad(ns) words.
__global__ __launch_bounds__(1024) void k_total_probe(const int32_t* orig, Geom g, QLadder fwd, QLadder inv, uint32_t nb, uint32_t nblocks,
                                                     int32_t* slots, unsigned long long* __restrict__ acc) {
    constexpr bool kPlanarCut = false;
#include "k_total_probe_body.hpp"
}

// k_planar_total_probe: the probe of rspt_hip_compress_total_planar_batch_dev -- the rows are the caller's matrix (single dwords at
// tid + j * nt: its 4-byte alignment is all they need), cut to the sample width on load.  orig is only read and lies outside
// slots: nothing but this kernel reads the matrix, and every slot of every entry is only written.
__global__ __launch_bounds__(1024) void k_planar_total_probe(const int32_t* __restrict__ orig, Geom g, QLadder fwd, QLadder inv, uint32_t nb,
                                                            uint32_t nblocks, int32_t* __restrict__ slots, unsigned long long* __restrict__ acc) {
    constexpr bool kPlanarCut = true;
#include "k_total_probe_body.hpp"
}

// prdn, mse: only read where path is 0 (k_q_finish leaves the cells of path 1 unwritten)
__global__ __launch_bounds__(256) void k_total_figs(const double* __restrict__ prdn, const double* __restrict__ mse, const uint32_t* __restrict__ path,
                                                   uint32_t cells, unsigned long long* __restrict__ figs) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cells) return;
    unsigned long long f = kTotalNaN;
    if (path[i] == 0u) {
        const double p = prdn[i];
        if (mse[i] == 0.0)
            f = 0ull;
        else if (p == p)
            f = (unsigned long long)__double_as_longlong(p);
    }
    figs[i] = f;
}

// One block at level T, from its kMaxLadder (figure, size) cells -- those beyond the ladder are (kTotalNaN, kTotalNone): what it
// adds to the cost, or that it is rated and has no pick.  rated: the block has a rated entry.
__device__ __forceinline__ void total_block(const unsigned long long (&f)[kMaxLadder], const unsigned long long (&s)[kMaxLadder], unsigned long long T,
                                            unsigned long long& cost, bool& unpicked, bool& rated) {
    unsigned long long best = kTotalNone, least = kTotalNone;
    bool r = false;
#pragma unroll
    for (uint32_t k = 0; k < kMaxLadder; ++k) {
        least = s[k] < least ? s[k] : least;
        if (f[k] <= kTotalInf) {
            r = true;
            if (f[k] <= T && s[k] < best) best = s[k];
        }
    }
    if (!r)
        cost += least;
    else if (best == kTotalNone)
        unpicked = true;
    else
        cost += best;
    rated |= r;
}

// sizes, figs: [nladder][nblocks].  res[0] = T* as a pattern, res[1] = cost(T*).  One workgroup of a multiple of 64 threads.
__global__ __launch_bounds__(1024) void k_total_level(const unsigned long long* __restrict__ sizes, const unsigned long long* __restrict__ figs,
                                                     uint32_t nladder, uint32_t nblocks, unsigned long long total, unsigned long long* __restrict__ res) {
    __shared__ unsigned long long s_cost[2][16];
    __shared__ uint32_t s_flag[2][16];  // bit 0: a rated block without a pick, bit 1: a rated block
    const uint32_t tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
    auto load = [&](uint32_t b, unsigned long long (&f)[kMaxLadder], unsigned long long (&s)[kMaxLadder]) {
#pragma unroll
        for (uint32_t k = 0; k < kMaxLadder; ++k) {
            const bool in = k < nladder && b < nblocks;
            f[k] = in ? figs[(size_t)k * nblocks + b] : kTotalNaN;
            s[k] = in ? sizes[(size_t)k * nblocks + b] : kTotalNone;
        }
    };
    unsigned long long f0[kMaxLadder], s0[kMaxLadder];  // block tid, for every round
    load(tid, f0, s0);
    uint32_t round = 0;
    // cost(T), and in flags what s_flag holds, for every thread alike
    auto eval = [&](unsigned long long T, uint32_t& flags) -> unsigned long long {
        unsigned long long cost = 0;
        bool unpicked = false, rated = false;
        if (tid < nblocks) total_block(f0, s0, T, cost, unpicked, rated);
        for (uint32_t b = tid + nt; b < nblocks; b += nt) {
            unsigned long long f[kMaxLadder], s[kMaxLadder];
            load(b, f, s);
            total_block(f, s, T, cost, unpicked, rated);
        }
        cost = q_wave_sum(cost);
        const uint32_t fl = (__ballot(unpicked) ? 1u : 0u) | (__ballot(rated) ? 2u : 0u);
        const uint32_t par = round++ & 1u;  // (round r + 2 writes this copy again: behind the barrier of round r + 1, so behind every read of round r)
        if ((tid & 63u) == 0) s_cost[par][tid >> 6] = cost, s_flag[par][tid >> 6] = fl;
        __syncthreads();
        cost = 0, flags = 0;
        for (uint32_t w = 0; w < nw; ++w) cost += s_cost[par][w], flags |= s_flag[par][w];
        return cost;
    };
    uint32_t flags;
    unsigned long long level = kTotalInf, cost = eval(kTotalInf, flags);  // (+inf is always admissible)
    if (!(flags & 2u)) {
        level = 0ull;  // no rated block: the cost is the same at every level
    } else if (cost <= total) {
        unsigned long long lo = 0ull;
        while (lo < level) {
            const unsigned long long mid = lo + ((level - lo) >> 1);
            const unsigned long long c = eval(mid, flags);
            if (!(flags & 1u) && c <= total)
                level = mid, cost = c;
            else
                lo = mid + 1ull;
        }
    }
    if (tid == 0) res[0] = level, res[1] = cost;
}

// One round of the same bisection for a batch of more blocks than one workgroup walks quickly: the whole grid evaluates one level,
// the workgroup that finishes last moves the bounds, and the host launches kTotalRounds of these one behind the other -- the
// stream orders the rounds, nothing waits inside a kernel.  Round 0 is the level +inf; round r > 0 the middle of the bounds round
// r - 1 left, and nothing once they have met.  res: [0] hi = T* in the end, [1] cost(hi), [2] lo; slot: this round's
// (cost, flags as in k_total_level, workgroups done), zero at the launch.
constexpr uint32_t kTotalRounds = 64;  // +inf, and the 63 halvings of [0, kTotalInf]
constexpr uint32_t kTotalWide = 4096;  // blocks above which the rounds are launches (host_total.hip)
struct TotalSlot {
    unsigned long long cost;
    uint32_t flags, done;
};
__global__ __launch_bounds__(256) void k_total_round(const unsigned long long* __restrict__ sizes, const unsigned long long* __restrict__ figs,
                                                    uint32_t nladder, uint32_t nblocks, unsigned long long total, uint32_t round,
                                                    unsigned long long* res, TotalSlot* slot) {
    __shared__ unsigned long long s_cost[4];
    __shared__ uint32_t s_flag[4];
    const uint32_t tid = threadIdx.x;
    const unsigned long long hi = res[0], lo = res[2];
    if (round && lo >= hi) return;
    const unsigned long long T = round ? lo + ((hi - lo) >> 1) : kTotalInf;
    unsigned long long cost = 0;
    bool unpicked = false, rated = false;
    for (uint32_t b = blockIdx.x * 256u + tid; b < nblocks; b += gridDim.x * 256u) {
        unsigned long long f[kMaxLadder], s[kMaxLadder];
#pragma unroll
        for (uint32_t k = 0; k < kMaxLadder; ++k) {
            f[k] = k < nladder ? figs[(size_t)k * nblocks + b] : kTotalNaN;
            s[k] = k < nladder ? sizes[(size_t)k * nblocks + b] : kTotalNone;
        }
        total_block(f, s, T, cost, unpicked, rated);
    }
    cost = q_wave_sum(cost);
    const uint32_t fl = (__ballot(unpicked) ? 1u : 0u) | (__ballot(rated) ? 2u : 0u);
    if ((tid & 63u) == 0) s_cost[tid >> 6] = cost, s_flag[tid >> 6] = fl;
    __syncthreads();
    if (tid) return;
    atomicAdd(&slot->cost, s_cost[0] + s_cost[1] + s_cost[2] + s_cost[3]);
    atomicOr(&slot->flags, s_flag[0] | s_flag[1] | s_flag[2] | s_flag[3]);
    __threadfence();
    if (atomicAdd(&slot->done, 1u) != gridDim.x - 1u) return;
    __threadfence();  // the last workgroup: every other one's sums are in the slot
    const unsigned long long c = atomicAdd(&slot->cost, 0ull);
    const uint32_t flags = atomicOr(&slot->flags, 0u);
    if (!round) {
        unsigned long long h = kTotalInf, l = 0ull;
        if (!(flags & 2u))
            h = 0ull;  // no rated block: +0.0
        else if (c > total)
            l = kTotalInf;  // a miss: the bounds have met at +inf
        res[0] = h, res[1] = c, res[2] = l;
    } else if (!(flags & 1u) && c <= total) {
        res[0] = T, res[1] = c;
    } else {
        res[2] = T + 1ull;
    }
}

// level_out, total_out, prdn_out, cand_sizes, cand_figs: nullptr, or where the result goes
__global__ __launch_bounds__(256) void k_total_pick(const unsigned long long* __restrict__ sizes, const unsigned long long* __restrict__ figs,
                                                   const uint32_t* __restrict__ path, uint32_t nladder, uint32_t nblocks,
                                                   const unsigned long long* __restrict__ res, uint32_t* __restrict__ choice,
                                                   double* __restrict__ prdn_out, double* __restrict__ level_out, unsigned long long* __restrict__ total_out,
                                                   unsigned long long* __restrict__ cand_sizes, double* __restrict__ cand_figs) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    const unsigned long long T = res[0];
    if (b == 0) {
        if (level_out) level_out[0] = __longlong_as_double((long long)T);
        if (total_out) total_out[0] = res[1];
    }
    if (b >= nblocks) return;
    uint32_t pick = nladder, least = 0;
    unsigned long long pick_size = kTotalNone, least_size = kTotalNone;
    bool rated = false;
    for (uint32_t k = 0; k < nladder; ++k) {
        const size_t at = (size_t)k * nblocks + b;
        const unsigned long long s = sizes[at], f = figs[at];
        if (cand_sizes) cand_sizes[at] = s;
        if (cand_figs) cand_figs[at] = __longlong_as_double((long long)f);
        if (s < least_size) least_size = s, least = k;
        if (f <= kTotalInf) {
            rated = true;
            if (f <= T && s < pick_size) pick_size = s, pick = k;
        }
    }
    // (a rated block has a pick: T* is admissible)
    const uint32_t k = rated && pick < nladder ? pick : least;
    choice[b] = k;
    const size_t at = (size_t)k * nblocks + b;
    if (prdn_out) prdn_out[b] = __longlong_as_double((long long)(path[at] == 0u ? figs[at] : kTotalInf));  // (+inf: no exact figure)
}

}  // namespace rspt
