// quality_planar.hip -- PRDN[%] (quality.hip) on the planar int32 matrix [nblocks][nch][ns] ("The planar form").
//
// The arithmetic, the accumulators (two limbs of sum t^2, sum r, sum |r| per block), the flag word, the wave reduction, the finish
// and the sequential chain are quality.hip's: QTerms, q_wave_sum, q_seq_chain, k_q_finish and mean_from_sum are used as
// they are.  What differs is where a channel lies: row (b, c) = b * nch + c of the matrix is ns consecutive words, so a unit of
// work is a piece of ONE row and has ONE mean:
//   k_qp_sums   the exact int64 row sums: one 64-bit atomic per unit into sums[row]
//   k_qp_accum  the second pass over o and d: one mean per unit, four atomics per workgroup and block into acc[b]
//   k_qp_seq    the chain of k_q_seq (q_seq_chain) with the row fetch
// A unit is a span of a row taken by a whole workgroup (rows longer than kQpWaveRow samples), or a whole row taken by one wave,
// four rows to a workgroup (shorter rows: a 16-sample row does not cost a workgroup).  Rows start on a 16-byte boundary only where
// the base does and ns % 4 == 0, so every unit reads a head of up to three samples up to the first 16-byte boundary of the o row,
// whole dwordx4 behind it and a tail of up to three samples.  d is read at the same sample positions, so its dwordx4 are 16-byte
// aligned only where its base is congruent with o's modulo 16; they are stated as loads from a 4-byte aligned address.
#include "common.hpp"

namespace rspt {

constexpr uint32_t kQpThreads = 256;
constexpr uint32_t kQpWaves = kQpThreads / kWave;
constexpr uint32_t kQpWaveRow = 1024;                // rows of up to this many samples take one wave each, kQpWaves rows per workgroup
constexpr uint32_t kQpU = 4;                         // dwordx4 in flight per lane and buffer
constexpr uint32_t kQpSweep = kQpThreads * 4 * kQpU; // samples of one unrolled step of a workgroup
constexpr uint32_t kQpMinSweeps = 2;                 // a span of a split row is at least this many sweeps
constexpr uint32_t kQpUnits = 4096;                  // rows are split while the call has fewer units than this
// the whole-row form (k_qp_rows): taken where the call has at least kQpFusedMinUnits units of whole rows of at most kQpFusedMaxNs
// samples; rows of up to kQpRowRegs samples (kQpWaveRow for a wave) stay in registers, longer ones are read twice
constexpr uint32_t kQpRowRegs = kQpThreads * 4 * kQpU;
constexpr uint32_t kQpFusedMinUnits = 1024;
constexpr uint32_t kQpFusedMaxNs = 8192;  // (the longest row at which the form was measured to win: DESIGN.md 4f)
static_assert(kQpWaveRow == kWave * 4 * kQpU, "a wave holds its whole row in registers");
static_assert(kQpThreads == kQThreads, "q_seq_chain is written for workgroups of kQThreads");

struct QPGeom {
    uint64_t rows;    // nblocks * nch rows of ns samples
    uint32_t nch, ns;
    uint32_t lanes;   // lanes of a unit: kWave (a row per wave) or kQpThreads (a span of a row per workgroup)
    uint32_t span;    // samples of a unit
    uint32_t nsplit;  // units of a row (1 where lanes == kWave)
};

struct QPUnit {
    uint64_t row;
    uint32_t s0, n;  // the unit's samples [s0, s0 + n) of its row
    uint32_t l;      // this thread's lane within the unit
    bool active;
};
__device__ __forceinline__ QPUnit qp_unit(const QPGeom& g) {
    QPUnit u;
    const uint32_t tid = threadIdx.x;
    if (g.lanes == (uint32_t)kWave) {
        u.row = (uint64_t)blockIdx.x * kQpWaves + tid / kWave;
        u.s0 = 0, u.n = g.ns;
        u.l = tid & (kWave - 1);
        u.active = u.row < g.rows;
        if (!u.active) u.row = g.rows - 1, u.n = 0;
    } else {
        u.row = blockIdx.x / g.nsplit;
        u.s0 = (blockIdx.x % g.nsplit) * g.span;
        u.n = g.ns - u.s0 < g.span ? g.ns - u.s0 : g.span;
        u.l = tid;
        u.active = true;
    }
    return u;
}

struct __attribute__((packed, aligned(4))) QpWords {  // four words at a 4-byte aligned address
    uint32_t x, y, z, w;
};
// ALIGNED: p is a multiple of 16.  (gfx950 takes a dwordx4 at any 4-byte aligned address: both forms are one load)
template <bool ALIGNED>
__device__ __forceinline__ uint4 qp_load4(const int32_t* p) {
    if (ALIGNED) return *reinterpret_cast<const uint4*>(p);
    const QpWords v = *reinterpret_cast<const QpWords*>(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}

// the samples in front of the first 16-byte boundary of p, at most n
__device__ __forceinline__ uint32_t qp_head(const int32_t* p, uint32_t n) {
    const uint32_t h = (4u - ((uint32_t)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u;
    return h < n ? h : n;
}

// f(o, d) on the samples [0, n) of po / pd that lane l of L takes (TWO: d is read; else d = o)
template <bool TWO, class F>
__device__ __forceinline__ void qp_walk(const int32_t* po, const int32_t* pd, uint32_t n, uint32_t l, uint32_t L, F&& f) {
    const uint32_t head = qp_head(po, n);
    const uint32_t nq = (n - head) >> 2, tail0 = head + 4u * nq;
    const int32_t* qo = po + head;
    const int32_t* qd = pd + head;
    auto four = [&](const uint4& a, const uint4& b) {
        f((int32_t)a.x, (int32_t)b.x), f((int32_t)a.y, (int32_t)b.y), f((int32_t)a.z, (int32_t)b.z), f((int32_t)a.w, (int32_t)b.w);
    };
    uint32_t q = l;
    for (; (uint64_t)q + (kQpU - 1) * L < nq; q += kQpU * L) {
        uint4 a[kQpU], b[kQpU];
#pragma unroll
        for (uint32_t k = 0; k < kQpU; ++k) {
            a[k] = qp_load4<true>(qo + 4ull * (q + k * L));
            if (TWO) b[k] = qp_load4<false>(qd + 4ull * (q + k * L));
        }
#pragma unroll
        for (uint32_t k = 0; k < kQpU; ++k) four(a[k], TWO ? b[k] : a[k]);
    }
    for (; q < nq; q += L) {
        const uint4 a = qp_load4<true>(qo + 4ull * q);
        four(a, TWO ? qp_load4<false>(qd + 4ull * q) : a);
    }
    if (l < head) f(po[l], TWO ? pd[l] : po[l]);
    if (l < n - tail0) f(po[tail0 + l], TWO ? pd[tail0 + l] : po[tail0 + l]);
}

// sums[row] += the samples of the unit (sums starts from zero)
__global__ __launch_bounds__(kQpThreads) void k_qp_sums(const int32_t* __restrict__ o, QPGeom g, unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long s_red[kQpWaves];
    const QPUnit u = qp_unit(g);
    const uint32_t tid = threadIdx.x;
    const int32_t* po = o + u.row * g.ns + u.s0;
    long long acc = 0;
    qp_walk<false>(po, po, u.n, u.l, g.lanes, [&](int32_t ov, int32_t) { acc += ov; });
    const unsigned long long s = q_wave_sum((unsigned long long)acc);
    if (g.lanes == (uint32_t)kWave) {
        if (u.l == 0 && u.active && s) atomicAdd(&sums[u.row], s);
        return;
    }
    if ((tid & (kWave - 1)) == 0) s_red[tid / kWave] = s;
    __syncthreads();
    if (tid == 0) {
        unsigned long long t = 0;
        for (uint32_t w = 0; w < kQpWaves; ++w) t += s_red[w];
        if (t) atomicAdd(&sums[u.row], t);
    }
}

// The accumulators of a workgroup's threads -> acc[b]: wave shuffle, LDS, then one atomic per accumulator for each block the
// workgroup's waves worked on (the rows of a workgroup ascend, so equal blocks are neighbours; blk = ~0: the wave had no row).
// (k_q_accum, whose waves all work on one block, keeps its plain sum over the waves: DESIGN.md 4f.)
__device__ __forceinline__ void qp_flush(const QTerms& T, uint32_t blk, unsigned long long* __restrict__ acc,
                                         unsigned long long (&s_red)[kQpWaves][4], uint32_t (&s_blk)[kQpWaves]) {
    const uint32_t tid = threadIdx.x;
    unsigned long long v[4] = {T.lo, T.hi, (unsigned long long)T.sr, T.sa};
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q_wave_sum(v[j]);
    if ((tid & (kWave - 1)) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s_red[tid / kWave][j] = v[j];
        s_blk[tid / kWave] = blk;
    }
    __syncthreads();
    if (tid < 4) {
        unsigned long long s = 0;
        uint32_t cur = s_blk[0];
        for (uint32_t w = 0; w < kQpWaves; ++w) {
            if (s_blk[w] != cur) {
                if (s && cur != ~0u) atomicAdd(&acc[(uint64_t)cur * 4 + tid], s);
                s = 0, cur = s_blk[w];
            }
            s += s_red[w][tid];
        }
        if (s && cur != ~0u) atomicAdd(&acc[(uint64_t)cur * 4 + tid], s);
    }
}

// acc[b] = {low and high 32 bits of every t^2 summed apart, sum r, sum |r|} (acc starts from zero)
__global__ __launch_bounds__(kQpThreads) void k_qp_accum(const int32_t* __restrict__ o, const int32_t* __restrict__ d, QPGeom g,
                                                        const long long* __restrict__ sums, unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long s_red[kQpWaves][4];
    __shared__ uint32_t s_blk[kQpWaves];
    const QPUnit u = qp_unit(g);
    const uint64_t at = u.row * g.ns + u.s0;
    const int32_t mean = mean_from_sum(sums[u.row], g.ns);
    QTerms T;
    qp_walk<true>(o + at, d + at, u.n, u.l, g.lanes, [&](int32_t ov, int32_t dv) { T.add(ov, dv, mean); });
    qp_flush(T, u.active ? (uint32_t)(u.row / g.nch) : ~0u, acc, s_red, s_blk);
}

// Both passes in one: a unit owns a WHOLE row (nsplit == 1).  It reads the row of o, reduces the sum, derives the mean, then
// takes the terms against d; sums[row] is stored for k_qp_seq (no atomic, no zeroing needed).  REGS: the row is at most
// lanes * 4 * kQpU samples, so every lane holds its share of o (and of d, loaded in the same go) in registers: o is read once.
// Else o is walked a second time at once, while the row is still in L2 or the Infinity Cache.
template <bool REGS>
__global__ __launch_bounds__(kQpThreads) void k_qp_rows(const int32_t* __restrict__ o, const int32_t* __restrict__ d, QPGeom g,
                                                       long long* __restrict__ sums, unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long s_red[kQpWaves][4];
    __shared__ uint32_t s_blk[kQpWaves];
    __shared__ unsigned long long s_sum[kQpWaves];
    const QPUnit u = qp_unit(g);
    const uint32_t tid = threadIdx.x, L = g.lanes, n = u.n, l = u.l;
    const int32_t* po = o + u.row * g.ns;
    const int32_t* pd = d + u.row * g.ns;
    auto row_sum = [&](long long part) -> long long {  // the sum over the unit's lanes, in every lane
        const unsigned long long s = q_wave_sum((unsigned long long)part);
        if (L == (uint32_t)kWave) return (long long)s;
        if ((tid & (kWave - 1)) == 0) s_sum[tid / kWave] = s;
        __syncthreads();
        unsigned long long t = 0;
#pragma unroll
        for (uint32_t w = 0; w < kQpWaves; ++w) t += s_sum[w];
        return (long long)t;
    };
    QTerms T;
    long long total;
    if (REGS) {
        const uint32_t head = qp_head(po, n);
        const uint32_t nq = (n - head) >> 2, tail0 = head + 4u * nq;
        uint4 a[kQpU], b[kQpU];
        int32_t ah = 0, bh = 0, at = 0, bt = 0;
#pragma unroll
        for (uint32_t k = 0; k < kQpU; ++k) {
            const uint32_t q = l + k * L;
            a[k] = b[k] = make_uint4(0, 0, 0, 0);
            if (q < nq) {
                a[k] = qp_load4<true>(po + head + 4ull * q);
                b[k] = qp_load4<false>(pd + head + 4ull * q);
            }
        }
        if (l < head) ah = po[l], bh = pd[l];
        if (l < n - tail0) at = po[tail0 + l], bt = pd[tail0 + l];
        long long part = (long long)ah + at;
#pragma unroll
        for (uint32_t k = 0; k < kQpU; ++k) part += (long long)(int32_t)a[k].x + (int32_t)a[k].y + (long long)(int32_t)a[k].z + (int32_t)a[k].w;
        total = row_sum(part);
        const int32_t mean = mean_from_sum(total, g.ns);
#pragma unroll
        for (uint32_t k = 0; k < kQpU; ++k)
            if (l + k * L < nq) {
                T.add((int32_t)a[k].x, (int32_t)b[k].x, mean), T.add((int32_t)a[k].y, (int32_t)b[k].y, mean);
                T.add((int32_t)a[k].z, (int32_t)b[k].z, mean), T.add((int32_t)a[k].w, (int32_t)b[k].w, mean);
            }
        if (l < head) T.add(ah, bh, mean);
        if (l < n - tail0) T.add(at, bt, mean);
    } else {
        long long part = 0;
        qp_walk<false>(po, po, n, l, L, [&](int32_t ov, int32_t) { part += ov; });
        total = row_sum(part);
        const int32_t mean = mean_from_sum(total, g.ns);
        qp_walk<true>(po, pd, n, l, L, [&](int32_t ov, int32_t dv) { T.add(ov, dv, mean); });
    }
    if (l == 0 && u.active) sums[u.row] = total;
    qp_flush(T, u.active ? (uint32_t)(u.row / g.nch) : ~0u, acc, s_red, s_blk);
}

// A flagged block in the reference's own order: the chain of k_q_seq (quality.hip: q_seq_chain), a chunk up to kQChunk consecutive words of a row.
__global__ __launch_bounds__(kQThreads) void k_qp_seq(const int32_t* __restrict__ o, const int32_t* __restrict__ d, uint32_t nch, uint32_t ns,
                                                     const long long* __restrict__ sums, const unsigned long long* __restrict__ acc,
                                                     const uint32_t* __restrict__ flag, double* __restrict__ prdn, double* __restrict__ mse_out,
                                                     double* __restrict__ ref_out) {
    const uint32_t b = blockIdx.x, fl = flag[b];
    if (!fl) return;
    const uint64_t row0 = (uint64_t)b * nch;
    q_seq_chain(b, nch, ns, sums + row0, acc, fl, prdn, mse_out, ref_out, [&](uint32_t c, uint32_t s) {
        const uint64_t at = (row0 + c) * ns + s;
        return QPair{o[at], d[at]};
    });
}

}  // namespace rspt
