// quality.hip -- PRDN[%], the reference's quality figure for its lossy packers (lib_rspt_test/rspt_test.cpp:98-111), on
// device-resident blocks in the interleaved native layout, bit-identical with the reference's x86-64 build.
//
//   mse = 0.0; ref = 0.0                                      one pair of doubles for the whole block
//   for c: mean = average_32(o[c])                            (int32)(int64)((uint64)sum / (uint64)ns)
//          for s: t = (int32)(o - d);  mse += (double)t * (double)t
//                 r = (int32)((o - mean) * (o - mean));  ref += (double)r        int * int: wraps, r may be negative
//   PRDN = sqrt(mse / ref) * 100.0
//
// Every term is an integer.  While no partial sum leaves +-2^53 every add is exact and the order does not matter, so
//   k_q_sums    the exact int64 channel sums, straight from the interleaved block (integer atomics: order-independent)
//   k_q_accum   the second pass over o and d: per block, exactly, S2 = sum t^2 (two limbs), SR = sum r, SA = sum |r|
//   k_q_finish  one thread per block: S2 <= 2^53 makes mse = (double)S2 what the reference's chain gives, SA <= 2^53 the same
//               for ref = (double)SR; where both hold the block is done, else it is flagged
//   k_q_seq     flagged blocks only (it exits at once for the others): one workgroup walks the block channel-outer, sample-inner,
//               three waves put the double terms of a chunk into LDS while one lane adds the chunk before in the reference's order.
// What the planar form (quality_planar.hip) shares is stated here once: the terms and a thread's accumulators (q_terms, QTerms),
// the wave reduction (q_wave_sum), the finish, and the chain itself, q_seq_chain, which k_q_seq and k_qp_seq call with the
// sample fetch of their layout -- the only place where the reference's ORDER of fp64 adds is reproduced.
//
// Layout of the two streaming passes.  A super-row is the fewest rows whose samples fill whole load groups (a group: 16 bytes,
// 48 for int24; 4 or 12 where only 4-byte alignment is given; one sample where not even that).  A thread owns one group position
// of the super-row, so each of its samples belongs to one channel for the whole walk; consecutive threads take consecutive
// groups (coalesced), and the threads left over take the super-rows that follow.
#include "common.hpp"

namespace rspt {

struct QGeom {
    uint64_t block_bytes;
    uint32_t nch, ns, be;
    uint32_t rows;      // rows of a super-row
    uint32_t qps;       // groups of a super-row
    uint32_t nsub;      // super-rows of a sweep: 256 / qps, at least 1
    uint32_t ncg;       // column groups: ceil(qps / 256)
    uint32_t nsr;       // whole super-rows of a block (the ns - nsr * rows rows behind them are read sample by sample)
    uint32_t span;      // super-rows of a workgroup, a multiple of nsub
    uint32_t nsplit;    // spans of a block
    uint32_t aligned4;  // block bases are multiples of 4
};

constexpr uint32_t kQThreads = 256;
constexpr uint32_t kQWaves = kQThreads / kWave;
constexpr uint32_t kQSlots = 4096;   // LDS accumulators of k_q_sums: groups of a super-row x samples of a group, where nsub > 1
constexpr uint32_t kQChunk = 1024;   // samples of a chunk of k_q_seq

// W: dwords of a load (4, 1) or 0 for sample-by-sample reads
template <int BPS, int W>
struct QVec {
    static constexpr int NW = W == 0 ? 1 : (BPS == 3 ? 3 : 1) * W;  // dwords of a group
    static constexpr int VS = W == 0 ? 1 : NW * 4 / BPS;            // samples of a group
    static constexpr int VB = W == 0 ? BPS : NW * 4;                // bytes of a group
};

template <int BPS, int W>
__device__ __forceinline__ void q_load(const uint8_t* p, uint32_t (&w)[QVec<BPS, W>::NW], const QGeom& g) {
    constexpr int NW = QVec<BPS, W>::NW;
    if (W == 0) {
        w[0] = (uint32_t)sample_from_bytes<BPS>(p, g.aligned4 != 0, g.be != 0);
    } else if (W == 4) {
#pragma unroll
        for (int i = 0; i < NW / 4; ++i) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[i];
            w[4 * i] = v.x, w[4 * i + 1] = v.y, w[4 * i + 2] = v.z, w[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = reinterpret_cast<const uint32_t*>(p)[i];
    }
}

// sample k of a loaded group, as convert_native_to_i32 reads it (be: the sample's bytes most significant first)
template <int BPS, int W>
__device__ __forceinline__ int32_t q_sample(const uint32_t (&w)[QVec<BPS, W>::NW], int k, bool be) {
    if (W == 0) return (int32_t)w[0];
    if (BPS == 4) return (int32_t)(be ? __builtin_amdgcn_perm(w[k], w[k], 0x00010203u) : w[k]);
    if (BPS == 2) {
        uint32_t u = (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
        if (be) u = ((u >> 8) | (u << 8)) & 0xFFFFu;
        return (int32_t)(int16_t)u;
    }
    if (BPS == 1) return (int32_t)(int8_t)(w[k >> 2] >> (8 * (k & 3)));
    const int i = (24 * k) >> 5, sh = (24 * k) & 31;  // int24: bits 24k .. 24k + 23 of the group
    uint32_t u = w[i] >> sh;
    if (sh > 8) u |= w[i + 1] << (32 - sh);
    u &= 0xFFFFFFu;
    if (be) u = ((u & 0xFFu) << 16) | (u & 0xFF00u) | (u >> 16);
    return (int32_t)(u << 8) >> 8;
}

// f(o[VS], d[VS]) on group q of the super-rows sr0, sr0 + nsub, ... below sr1 (TWO: d is read; else d = o)
template <int BPS, int W, bool TWO, class F>
__device__ __forceinline__ void q_walk(const uint8_t* o, const uint8_t* d, const QGeom& g, uint32_t q, uint64_t sr0, uint64_t sr1, F&& f) {
    using V = QVec<BPS, W>;
    constexpr int U = BPS == 3 ? 2 : 4;  // groups in flight per buffer
    const uint64_t SB = (uint64_t)g.qps * V::VB, step = SB * g.nsub;
    const bool be = g.be != 0;
    uint64_t off = sr0 * SB + (uint64_t)q * V::VB;
    uint64_t sr = sr0;
    int32_t ov[V::VS], dv[V::VS];
    for (; sr + (uint64_t)(U - 1) * g.nsub < sr1; sr += (uint64_t)U * g.nsub, off += U * step) {
        uint32_t wo[U][V::NW], wd[U][V::NW];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            q_load<BPS, W>(o + off + u * step, wo[u], g);
            if (TWO) q_load<BPS, W>(d + off + u * step, wd[u], g);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int k = 0; k < V::VS; ++k) {
                ov[k] = q_sample<BPS, W>(wo[u], k, be);
                dv[k] = TWO ? q_sample<BPS, W>(wd[u], k, be) : ov[k];
            }
            f(ov, dv);
        }
    }
    for (; sr < sr1; sr += g.nsub, off += step) {
        uint32_t wo[V::NW], wd[V::NW];
        q_load<BPS, W>(o + off, wo, g);
        if (TWO) q_load<BPS, W>(d + off, wd, g);
#pragma unroll
        for (int k = 0; k < V::VS; ++k) {
            ov[k] = q_sample<BPS, W>(wo, k, be);
            dv[k] = TWO ? q_sample<BPS, W>(wd, k, be) : ov[k];
        }
        f(ov, dv);
    }
}

// what a workgroup of the two streaming passes is and which part of it a thread takes
struct QUnit {
    uint32_t b, split, cg, q;
    uint64_t sr0, sr1;
    bool active;
};
__device__ __forceinline__ QUnit q_unit(const QGeom& g) {
    QUnit u;
    uint32_t x = blockIdx.x;
    u.split = x % g.nsplit;
    x /= g.nsplit;
    u.cg = x % g.ncg;
    u.b = x / g.ncg;
    const uint32_t tid = threadIdx.x;
    uint32_t sub;
    if (g.nsub > 1) {
        sub = tid / g.qps;
        u.q = tid - sub * g.qps;
        u.active = sub < g.nsub;
    } else {
        sub = 0;
        u.q = u.cg * kQThreads + tid;
        u.active = u.q < g.qps;
    }
    const uint64_t s0 = (uint64_t)u.split * g.span;
    u.sr0 = s0 + sub;
    u.sr1 = s0 + g.span < g.nsr ? s0 + g.span : g.nsr;
    return u;
}

__device__ __forceinline__ void q_terms(int32_t o, int32_t d, int32_t mean, int32_t& t, int32_t& r) {
    t = (int32_t)((uint32_t)o - (uint32_t)d);
    const uint32_t dm = (uint32_t)o - (uint32_t)mean;
    r = (int32_t)(dm * dm);
}

// A thread's four exact accumulators: the low and high 32 bits of every t^2 summed apart, sum r, sum |r|.
struct QTerms {
    unsigned long long lo = 0, hi = 0, sa = 0;
    long long sr = 0;
    __device__ __forceinline__ void add(int32_t ov, int32_t dv, int32_t mean) {
        int32_t t, r;
        q_terms(ov, dv, mean, t, r);
        const unsigned long long t2 = (unsigned long long)((long long)t * (long long)t);  // up to 2^62
        lo += (uint32_t)t2;
        hi += t2 >> 32;
        sr += r;
        sa += (unsigned long long)(r < 0 ? -(long long)r : (long long)r);
    }
};

__device__ __forceinline__ unsigned long long q_wave_sum(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (unsigned long long)__shfl_xor((long long)v, m);
    return v;
}


// sums[b][c] += the samples of channel c (sums starts from zero)
template <int BPS, int W>
__global__ __launch_bounds__(kQThreads) void k_q_sums(const uint8_t* __restrict__ o, QGeom g, unsigned long long* __restrict__ sums) {
    using V = QVec<BPS, W>;
    __shared__ unsigned long long s_acc[kQSlots];
    const QUnit u = q_unit(g);
    const uint32_t tid = threadIdx.x;
    const uint8_t* blk = o + (uint64_t)u.b * g.block_bytes;
    unsigned long long* bs = sums + (uint64_t)u.b * g.nch;
    const uint32_t slots = g.qps * V::VS;  // (used where nsub > 1: qps <= 128, so slots <= kQSlots / 2)
    if (g.nsub > 1) {
        for (uint32_t i = tid; i < slots; i += kQThreads) s_acc[i] = 0;
        __syncthreads();
    }
    long long acc[V::VS];
#pragma unroll
    for (int k = 0; k < V::VS; ++k) acc[k] = 0;
    if (u.active)
        q_walk<BPS, W, false>(blk, blk, g, u.q, u.sr0, u.sr1, [&](const int32_t(&ov)[V::VS], const int32_t(&)[V::VS]) {
#pragma unroll
            for (int k = 0; k < V::VS; ++k) acc[k] += ov[k];
        });
    if (g.nsub > 1) {
        if (u.active) {
#pragma unroll
            for (int k = 0; k < V::VS; ++k)
                if (acc[k]) atomicAdd(&s_acc[u.q * V::VS + k], (unsigned long long)acc[k]);
        }
        __syncthreads();
        for (uint32_t i = tid; i < slots; i += kQThreads)  // sample i of the super-row: channel i mod nch
            if (s_acc[i]) atomicAdd(&bs[i % g.nch], s_acc[i]);
    } else if (u.active) {
        uint32_t c = (uint32_t)(((uint64_t)u.q * V::VS) % g.nch);
#pragma unroll
        for (int k = 0; k < V::VS; ++k) {
            if (acc[k]) atomicAdd(&bs[c], (unsigned long long)acc[k]);
            c = c + 1 == g.nch ? 0 : c + 1;
        }
    }
    if (u.split == 0 && u.cg == 0) {  // the rows behind the last whole super-row
        const uint64_t row0 = (uint64_t)g.nsr * g.rows, n = ((uint64_t)g.ns - row0) * g.nch;
        for (uint64_t i = tid; i < n; i += kQThreads) {
            const int32_t v = sample_from_bytes<BPS>(blk + (row0 * g.nch + i) * BPS, g.aligned4 != 0, g.be != 0);
            if (v) atomicAdd(&bs[i % g.nch], (unsigned long long)(long long)v);
        }
    }
}

// acc[b] = {low and high 32 bits of every t^2 summed apart, sum r, sum |r|} (acc starts from zero)
template <int BPS, int W>
__global__ __launch_bounds__(kQThreads) void k_q_accum(const uint8_t* __restrict__ o, const uint8_t* __restrict__ d, QGeom g,
                                                      const long long* __restrict__ sums, unsigned long long* __restrict__ acc) {
    using V = QVec<BPS, W>;
    __shared__ unsigned long long s_red[kQWaves][4];
    const QUnit u = q_unit(g);
    const uint32_t tid = threadIdx.x;
    const uint8_t* bo = o + (uint64_t)u.b * g.block_bytes;
    const uint8_t* bd = d + (uint64_t)u.b * g.block_bytes;
    const long long* bs = sums + (uint64_t)u.b * g.nch;
    QTerms T;
    if (u.active && u.sr0 < u.sr1) {
        int32_t mean[V::VS];
        uint32_t c = (uint32_t)(((uint64_t)u.q * V::VS) % g.nch);
#pragma unroll
        for (int k = 0; k < V::VS; ++k) {
            mean[k] = mean_from_sum(bs[c], g.ns);
            c = c + 1 == g.nch ? 0 : c + 1;
        }
        q_walk<BPS, W, true>(bo, bd, g, u.q, u.sr0, u.sr1, [&](const int32_t(&ov)[V::VS], const int32_t(&dv)[V::VS]) {
#pragma unroll
            for (int k = 0; k < V::VS; ++k) T.add(ov[k], dv[k], mean[k]);
        });
    }
    if (u.split == 0 && u.cg == 0) {
        const uint64_t row0 = (uint64_t)g.nsr * g.rows, n = ((uint64_t)g.ns - row0) * g.nch;
        for (uint64_t i = tid; i < n; i += kQThreads) {
            const uint64_t at = (row0 * g.nch + i) * BPS;
            T.add(sample_from_bytes<BPS>(bo + at, g.aligned4 != 0, g.be != 0), sample_from_bytes<BPS>(bd + at, g.aligned4 != 0, g.be != 0),
                  mean_from_sum(bs[i % g.nch], g.ns));
        }
    }
    // (not q_flush: every wave here works on block u.b, and its walk over the waves' blocks measured slower -- DESIGN.md 4f)
    unsigned long long v[4] = {T.lo, T.hi, (unsigned long long)T.sr, T.sa};
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q_wave_sum(v[j]);
    if ((tid & (kWave - 1)) == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s_red[tid / kWave][j] = v[j];
    }
    __syncthreads();
    if (tid < 4) {
        unsigned long long s = 0;
        for (uint32_t w = 0; w < kQWaves; ++w) s += s_red[w][tid];
        if (s) atomicAdd(&acc[(uint64_t)u.b * 4 + tid], s);
    }
}

// The end of the reference's computation: correctly rounded divide, square root and product, each on its own; a NaN (sqrt of a
// negative quotient, 0 / 0) is the x86-64 build's default NaN.
__device__ __forceinline__ double q_prdn(double mse, double ref) {
    const double p = __dmul_rn(__dsqrt_rn(__ddiv_rn(mse, ref)), 100.0);
    return p != p ? __longlong_as_double((long long)0xFFF8000000000000ull) : p;
}

// S2 = sum t^2 from its two limbs, where it is at most 2^53 (else false)
__device__ __forceinline__ bool q_s2_exact(const unsigned long long* a, double& mse) {
    const unsigned long long top = a[1] + (a[0] >> 32), low = a[0] & 0xFFFFFFFFull;  // S2 = top * 2^32 + low
    if (top > (1ull << 21) || (top == (1ull << 21) && low != 0)) return false;
    mse = (double)((top << 32) | low);
    return true;
}
__device__ __forceinline__ bool q_sr_exact(const unsigned long long* a, double& ref) {
    if (a[3] > (1ull << 53)) return false;
    ref = (double)(long long)a[2];
    return true;
}

// flag[b]: bit 0 -- mse needs the sequential chain, bit 1 -- ref does; 0: the block is finished here
__global__ __launch_bounds__(256) void k_q_finish(const unsigned long long* __restrict__ acc, uint32_t nblocks, uint32_t* __restrict__ flag,
                                                 double* __restrict__ prdn, double* __restrict__ mse_out, double* __restrict__ ref_out,
                                                 uint32_t* __restrict__ path) {
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nblocks) return;
    double mse = 0, ref = 0;
    const uint32_t fl = (q_s2_exact(acc + (uint64_t)b * 4, mse) ? 0u : 1u) | (q_sr_exact(acc + (uint64_t)b * 4, ref) ? 0u : 2u);
    flag[b] = fl;
    if (path) path[b] = fl ? 1u : 0u;
    if (fl) return;
    prdn[b] = q_prdn(mse, ref);
    if (mse_out) mse_out[b] = mse;
    if (ref_out) ref_out[b] = ref;
}

struct QPair {
    int32_t o, d;
};

// A flagged block b (a workgroup of kQThreads; fl = flag[b], which the kernel has found non-zero before it set up its fetch) in the
// reference's own order, for both layouts: fetch(c, s) reads the two samples of channel c at sample s, bs points at the sums of
// the block's channels.
// Chunk k = (channel, up to kQChunk consecutive samples of it); waves 1 .. 3 put the terms of chunk k + 1 into one half of the
// LDS buffers while lane 0 adds chunk k from the other: a product is rounded on its way into LDS, so no product and add contract.
template <class Fetch>
__device__ __forceinline__ void q_seq_chain(uint32_t b, uint32_t nch, uint32_t ns, const long long* __restrict__ bs,
                                            const unsigned long long* __restrict__ acc, uint32_t fl,
                                            double* __restrict__ prdn, double* __restrict__ mse_out, double* __restrict__ ref_out, Fetch&& fetch) {
    __shared__ double s_t[2][kQChunk], s_r[2][kQChunk];
    const uint32_t tid = threadIdx.x;
    const bool need_m = (fl & 1u) != 0, need_r = (fl & 2u) != 0;
    const uint32_t cpc = (ns + kQChunk - 1) / kQChunk;  // chunks per channel
    const uint64_t nchunks = (uint64_t)nch * cpc;
    auto produce = [&](uint64_t k, uint32_t t0, uint32_t nt) {
        const uint32_t c = (uint32_t)(k / cpc), s0 = (uint32_t)(k - (uint64_t)c * cpc) * kQChunk;
        const uint32_t n = ns - s0 < kQChunk ? ns - s0 : kQChunk;
        const int32_t mean = mean_from_sum(bs[c], ns);
        double* pt = s_t[k & 1];
        double* pr = s_r[k & 1];
        for (uint32_t i = t0; i < n; i += nt) {
            const QPair x = fetch(c, s0 + i);
            int32_t t, r;
            q_terms(x.o, x.d, mean, t, r);
            if (need_m) pt[i] = __dmul_rn((double)t, (double)t);
            if (need_r) pr[i] = (double)r;
        }
    };
    produce(0, tid, kQThreads);
    __syncthreads();
    double mse = 0.0, ref = 0.0;
    for (uint64_t k = 0; k < nchunks; ++k) {
        if (tid >= kWave) {
            if (k + 1 < nchunks) produce(k + 1, tid - kWave, kQThreads - kWave);
        } else if (tid == 0) {
            const uint32_t s0 = (uint32_t)(k % cpc) * kQChunk;
            const uint32_t n = ns - s0 < kQChunk ? ns - s0 : kQChunk;
            const double* pt = s_t[k & 1];
            const double* pr = s_r[k & 1];
            if (need_m && need_r) {
#pragma unroll 8
                for (uint32_t i = 0; i < n; ++i) {
                    mse = __dadd_rn(mse, pt[i]);
                    ref = __dadd_rn(ref, pr[i]);
                }
            } else if (need_m) {
#pragma unroll 8
                for (uint32_t i = 0; i < n; ++i) mse = __dadd_rn(mse, pt[i]);
            } else {
#pragma unroll 8
                for (uint32_t i = 0; i < n; ++i) ref = __dadd_rn(ref, pr[i]);
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (!need_m) q_s2_exact(acc + (uint64_t)b * 4, mse);
        if (!need_r) q_sr_exact(acc + (uint64_t)b * 4, ref);
        prdn[b] = q_prdn(mse, ref);
        if (mse_out) mse_out[b] = mse;
        if (ref_out) ref_out[b] = ref;
    }
}

// the chain on the interleaved block (BPS = 1 is instantiated but never flagged: t^2 <= 2^16 would need 2^37 samples)
template <int BPS>
__global__ __launch_bounds__(kQThreads) void k_q_seq(const uint8_t* __restrict__ o, const uint8_t* __restrict__ d, QGeom g,
                                                    const long long* __restrict__ sums, const unsigned long long* __restrict__ acc,
                                                    const uint32_t* __restrict__ flag, double* __restrict__ prdn, double* __restrict__ mse_out,
                                                    double* __restrict__ ref_out) {
    const uint32_t b = blockIdx.x, fl = flag[b];
    if (!fl) return;
    const bool be = g.be != 0, al = g.aligned4 != 0;
    const uint8_t* bo = o + (uint64_t)b * g.block_bytes;
    const uint8_t* bd = d + (uint64_t)b * g.block_bytes;
    q_seq_chain(b, g.nch, g.ns, sums + (uint64_t)b * g.nch, acc, fl, prdn, mse_out, ref_out, [&](uint32_t c, uint32_t s) {
        const uint64_t at = ((uint64_t)s * g.nch + c) * BPS;
        return QPair{sample_from_bytes<BPS>(bo + at, al, be), sample_from_bytes<BPS>(bd + at, al, be)};
    });
}

}  // namespace rspt
