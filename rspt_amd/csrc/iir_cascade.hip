// iir_cascade.hip -- a cascade of 1 to 4 reference IIR filters per channel, chained in double and truncated once
// (rspt_hip_iir_cascade_batch_dev / _stream_dev; semantics: rspt_hip.h).
//
// The reference's filter objects return double and its users chain them per sample -- lp->filter_opt(hp->filter_opt(x)), or the
// three filters of peak_detector.h:89-91 -- so what enters section k + 1 is section k's untruncated output, NaN and inf
// included, and only the last section's result is converted to int32.  Each section is one i_filter::new_iir object
// (iir_filter.cpp:46-116), stated in iir.hpp (IirState), run through filter_opt() -- all feed-forward terms first, then the
// feedback terms -- or through filter() -- the terms interleaved -- and initialised with the channel's RAW first sample.
#include "iir.hpp"

// NO contraction in this file: iir.hpp says why.
#pragma clang fp contract(off)

namespace rspt {

constexpr uint32_t kCascMaxSections = 4;
struct CascadeArgs {
    IirCoef s[kCascMaxSections];
    uint32_t nsec;        // 1..4
    uint32_t use_filter;  // bit k: section k runs filter() instead of filter_opt()
};

// A section's rings where a kernel keeps them outside the code that knows their length (five places each, newest first, the
// places past nc - 1 zero) at the start of a run: the carried ones, or a fresh object's behind init_history_values on x0.
// (The loop is IirState::init_history written out, and the pipelined kernel's producers write their set load and their
// selection of the last inputs out as k_iir_pipe does: see there.)
__device__ __forceinline__ void casc_start(const IirCoef& c, double x0, bool started, const IirCarry* cs, double (&x)[5], double (&y)[5]) {
    if (started) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            x[i] = cs->x[i];
            y[i] = cs->y[i];
        }
    } else {
        by_nc(c.nc, [&](auto ncv) {
            IirState<decltype(ncv)::value> f;
            f.clear();
            constexpr int NC = decltype(ncv)::value;
            int32_t i = 0;
            for (; i < c.init_steps && i < NC; ++i) f.step(c.n, c.d, x0);  // (until the x ring holds nothing but x0)
            if (i < c.init_steps) {
                double P[NC];
#pragma unroll
                for (int k = 0; k < NC; ++k) P[k] = c.d[k] * x0;
#pragma unroll 4
                for (; i < c.init_steps; ++i) f.step_const(c.n, P);
            }
            f.store(x, y);
        });
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The plain kernel: one thread per (block, channel) runs the chain as written in rspt_hip.h, sample by sample.  It serves rows
// shorter than a chunk of the pipelined kernel.  CARRY: one run of ns rows (nblocks = 1), the chain of channel ch in
// state[ch * nsec ..]; `started` of section 0 decides whether the channel initialises.
// PLANAR (k_iir_cascade_planar, the same body; the int32 matrix [nblocks][nch][hns], filter.hip: PlanarRun): block_bytes is one
// block of the matrix; stateless the run is the channel's row (ns = hns), CARRY it is the channel's rows in ns / hns blocks.
template <int BPS, bool CARRY>
__global__ __launch_bounds__(64) void k_iir_cascade(uint8_t* __restrict__ buf, uint32_t nch, uint32_t ns, uint64_t block_bytes, CascadeArgs a, uint32_t nblocks,
                                                    IirCarry* __restrict__ state) {
    constexpr bool PLANAR = false;
#include "k_iir_cascade_body.hpp"
}

template <bool CARRY>
__global__ __launch_bounds__(64) void k_iir_cascade_planar(uint8_t* __restrict__ buf, uint32_t nch, uint32_t ns, uint64_t block_bytes, CascadeArgs a,
                                                           uint32_t nblocks, IirCarry* __restrict__ state) {
    constexpr int BPS = 4;
    constexpr bool PLANAR = true;
#include "k_iir_cascade_body.hpp"
}

// ---------------------------------------------------------------------------------------------------------------------------
// The pipelined kernel, in the manner of k_iir_pipe: lane <-> channel in every wave, and the wave that holds a ring issues only
// what depends on it.  A chunk of 32 samples per lane travels through 2 S + 1 stages, one stage per tick (one workgroup barrier),
// in ONE LDS tile [sample][lane] of doubles that every stage rewrites in place (a lane reads and writes its own column only):
//   tick j              two producer waves load the samples (two chunks ahead), convert them and write section 0's
//                       feed-forward sums of half a chunk each (filter(): the samples themselves, as doubles)
//   tick j + 2k + 1     section k's recurrence wave: sum -> output, its y ring in registers (filter(): both rings)
//   tick j + 2k + 2     section k + 1's feed-forward wave: outputs of section k -> feed-forward sums of section k + 1, the inputs
//                       in front of the chunk in registers (filter(): nothing to do, the tile passes as it is)
//   tick j + 2S         the store wave truncates the last section's outputs (trunc_i32_c) and stores them
// So S recurrences run at once, on chunks two ticks apart, and the time per sample is the slowest wave's, not the sum.  A chunk
// owns tile j mod 9 from its producer to its store; 2 S + 1 <= 9 chunks are under way.  Waves 0..S-1 are the recurrence waves
// (consecutive waves go to different SIMDs), then the S - 1 feed-forward waves, the two producers, the store wave.
//
// Every section starts from the channel's raw first sample x0 (init_history_values on a fresh object; all recurrence waves run it
// at once in front of the first tick), and what its x ring then holds -- x0 in the first min(init_steps, nc) places, 0.0 behind --
// stands in front of the run for the wave that forms its feed-forward sums, so any init_steps will do.  CARRY: ONE run of ns rows
// (nblocks = 1); a channel whose section 0 has started takes every section's rings from state[ch * S + k] instead, and each
// ring is written back by the wave that holds it, behind the run's last chunk.  A wave reads the state in front of the first
// barrier and writes only places that no other wave reads, or (the producers' x ring) a tick later, behind a barrier.
//
// PLANAR (k_iir_cascade_pipe_planar, the same body, a CascWavePlanar): as k_iir_pipe's -- the producers' sets through
// planar_load_set, the store wave's groups through planar_store_part.
constexpr uint32_t kCascChunk = 32, kCascProd = 2, kCascPart = kCascChunk / kCascProd;
constexpr uint32_t kCascSlots = 2 * kCascMaxSections + 1;
constexpr uint32_t kCascGroup = 16;  // samples a wave reads from the tile together, works on, and writes together
static_assert(kCascPart == kCascGroup && kCascChunk % kCascGroup == 0, "a producer takes one group of a chunk");
__host__ __device__ constexpr uint32_t casc_waves(uint32_t nsec) { return 2 * nsec + 2; }
constexpr uint32_t kCascMaxThreads = 64 * casc_waves(kCascMaxSections);
struct CascLds {
    double v[kCascSlots][kCascChunk][64];
};
// 144 KiB of static LDS: one workgroup per CU, on a part with 160 KiB per workgroup (gfx950)
static_assert(sizeof(CascLds) <= 160 * 1024, "k_iir_cascade_pipe: the tiles must fit one CU's LDS");

// section k's recurrence over one chunk, in place: feed-forward sums (filter(): inputs) -> outputs
template <int NC, bool FILTER>
__device__ __forceinline__ void casc_rec_chunk(double (*T)[64], uint32_t lane, uint32_t cnt, const IirCoef& c, IirState<NC>& f) {
    auto rec = [&](double a) { return FILTER ? f.step(c.n, c.d, a) : f.feedback(c.n, a); };
    if (cnt == kCascChunk) {
#pragma unroll 1
        for (uint32_t e0 = 0; e0 < kCascChunk; e0 += kCascGroup) {
            double v[kCascGroup];
#pragma unroll
            for (uint32_t e = 0; e < kCascGroup; ++e) v[e] = T[e0 + e][lane];
#pragma unroll
            for (uint32_t e = 0; e < kCascGroup; ++e) v[e] = rec(v[e]);
#pragma unroll
            for (uint32_t e = 0; e < kCascGroup; ++e) T[e0 + e][lane] = v[e];
        }
    } else {
        for (uint32_t e = 0; e < cnt; ++e) T[e][lane] = rec(T[e][lane]);
    }
}

// section k's feed-forward sums over one chunk, in place: inputs -> ((d0 x0 + d1 x1) + d2 x2) + ...; x = the inputs in front of
// the chunk, newest first, and behind it the chunk's last five
template <int NC>
__device__ __forceinline__ void casc_ff_chunk(double (*T)[64], uint32_t lane, uint32_t cnt, const IirCoef& c, double (&x)[5]) {
    constexpr int H = 4;
    if (cnt == kCascChunk) {
#pragma unroll 1
        for (uint32_t e0 = 0; e0 < kCascChunk; e0 += kCascGroup) {
            double xs[kCascGroup + H], o[kCascGroup];
#pragma unroll
            for (int i = 0; i < H; ++i) xs[i] = x[H - 1 - i];
#pragma unroll
            for (uint32_t e = 0; e < kCascGroup; ++e) xs[H + e] = T[e0 + e][lane];
#pragma unroll
            for (uint32_t e = 0; e < kCascGroup; ++e) o[e] = iir_ff<NC>(c.d, &xs[H + e]);
#pragma unroll
            for (uint32_t e = 0; e < kCascGroup; ++e) T[e0 + e][lane] = o[e];
#pragma unroll
            for (int i = 0; i < 5; ++i) x[i] = xs[kCascGroup + H - 1 - i];
        }
    } else {
        for (uint32_t e = 0; e < cnt; ++e) {
            const double in = T[e][lane];
            double s = c.d[0] * in;
#pragma unroll
            for (int i = 1; i < NC; ++i) s = s + c.d[i] * x[i - 1];
            T[e][lane] = s;
#pragma unroll
            for (int i = 4; i > 0; --i) x[i] = x[i - 1];
            x[0] = in;
        }
    }
}

// What every wave of the pipelined kernel knows: its lane's run, its section, and the tick at which it meets chunk 0.
struct CascWave {
    uint8_t* p;       // the lane's first sample
    size_t stride;    // bytes from one sample of the channel to the next
    uint32_t ns, nchunks, nticks, lane, off;
    bool valid;       // (lanes past the batch read block 0, channel 0 along with the others and store nothing)
    bool started;     // CARRY: section 0 of the lane's channel has started
    bool filt;        // the wave's section runs filter()
    double x0;        // the run's first sample
    IirCarry* cs;     // CARRY: the state of the wave's section of the lane's channel
    double (*tiles)[kCascChunk][64];
    __device__ __forceinline__ uint32_t count(uint32_t j) const { return min(kCascChunk, ns - j * kCascChunk); }
};

struct CascWavePlanar : CascWave {
    PlanarRun run;  // where the run's samples live in the matrix
};
// the lane's first sample and its run in the matrix (the overload on CascWave is never called: a statement under
// `if constexpr (PLANAR)` outside a template is not compiled to anything, but it has to name something)
template <bool ONE_ROW>
__device__ __forceinline__ void casc_planar_start(CascWavePlanar& w, uint8_t* buf, uint32_t nch, uint32_t ns, uint64_t block_bytes, uint32_t b, uint32_t ch) {
    w.p = buf + (size_t)b * block_bytes + (size_t)ch * planar_run<ONE_ROW>(buf, nch, ns, block_bytes).hns * 4u;
    w.run = planar_run<ONE_ROW>(w.p, nch, ns, block_bytes);
}
template <bool ONE_ROW>
__device__ __forceinline__ void casc_planar_start(CascWave&, uint8_t*, uint32_t, uint32_t, uint64_t, uint32_t, uint32_t) {}

// Each role is a tick loop of its own with the same number of barriers, so that no role's registers live through another's.

// section k's recurrence: sums -> outputs, its y ring in registers (filter(): both rings); the history initialisation in front
template <bool CARRY>
__device__ __forceinline__ void casc_wave_rec(const CascWave& w, const IirCoef& c) {
    double x[5], y[5];
    casc_start(c, w.x0, w.started, w.cs, x, y);
    for (uint32_t t = 0; t < w.nticks; ++t) {
        const uint32_t j = t - w.off;  // (wraps in front of the wave's first chunk)
        if (j < w.nchunks) {
            by_nc(c.nc, [&](auto ncv) {
                constexpr int NC = decltype(ncv)::value;
                IirState<NC> f;
                f.load(x, y);
                if (w.filt) casc_rec_chunk<NC, true>(w.tiles[j % kCascSlots], w.lane, w.count(j), c, f);
                else casc_rec_chunk<NC, false>(w.tiles[j % kCascSlots], w.lane, w.count(j), c, f);
                f.store(x, y);
            });
        }
        __syncthreads();
    }
    if (CARRY && w.valid) {  // the object as it stands behind the run's last sample
        for (uint32_t i = 0; i < c.nc; ++i) {
            w.cs->y[i] = y[i];
            if (w.filt) w.cs->x[i] = x[i];
        }
        w.cs->started = 1;
    }
}

// section k >= 1's feed-forward sums: outputs of section k - 1 -> sums, the inputs in front of the chunk in registers
// (filter(): the tile passes as it is, and the recurrence wave holds the x ring)
template <bool CARRY>
__device__ __forceinline__ void casc_wave_ff(const CascWave& w, const IirCoef& c) {
    double x[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) x[i] = w.filt ? 0.0 : w.started ? w.cs->x[i] : iir_front(c, w.x0, i);
    for (uint32_t t = 0; t < w.nticks; ++t) {
        const uint32_t j = t - w.off;
        if (j < w.nchunks && !w.filt) by_nc(c.nc, [&](auto ncv) { casc_ff_chunk<decltype(ncv)::value>(w.tiles[j % kCascSlots], w.lane, w.count(j), c, x); });
        __syncthreads();
    }
    if (CARRY && w.valid && !w.filt) {
        for (uint32_t i = 0; i < c.nc; ++i) w.cs->x[i] = x[i];
    }
}

// a producer: loads its half of every chunk two chunks ahead, converts, writes section 0's feed-forward sums (filter(): the samples)
template <int BPS, bool ALIGNED, bool CARRY, class W>
__device__ __forceinline__ void casc_wave_prod(const W& w, const IirCoef& c, uint32_t part) {
    constexpr bool PLANAR = std::is_same<W, CascWavePlanar>::value;
    constexpr int H = 4;
    constexpr uint32_t SET = kCascPart + H;  // its 16 samples and the H in front: element e of chunk j is sample j * 32 + part * 16 - H + e
    double x[5];  // the inputs in front of the run, newest first; behind the run's last chunk: the run's last inputs
#pragma unroll
    for (int i = 0; i < 5; ++i) x[i] = (w.filt || part != 0u) ? 0.0 : w.started ? w.cs->x[i] : iir_front(c, w.x0, i);
    bool have_last = false;
    int32_t cur[SET], nxt[SET], nx2[SET];
    auto load_set = [&](int32_t (&v)[SET], uint32_t j) {
        const int32_t s0 = (int32_t)(j * kCascChunk + part * kCascPart) - H;
        if constexpr (PLANAR) {
            planar_load_set<(uint32_t)H, !CARRY>(w.run, w.ns, s0, v);
        } else if (s0 >= 0 && s0 + (int32_t)SET <= (int32_t)w.ns) {  // (wave-uniform; all but a run's first and last sets)
            const uint8_t* q = w.p + (size_t)s0 * w.stride;
#pragma unroll
            for (uint32_t e = 0; e < SET; ++e) v[e] = sample_load<BPS>(q + (size_t)e * w.stride, ALIGNED);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < SET; ++e) {
                int32_t si = s0 + (int32_t)e;
                si = si < 0 ? 0 : si >= (int32_t)w.ns ? (int32_t)w.ns - 1 : si;  // (clamped: what lies outside is never used as such)
                v[e] = sample_load<BPS>(w.p + (size_t)si * w.stride, ALIGNED);
            }
        }
    };
    load_set(cur, 0);
    if (w.nchunks > 1) load_set(nxt, 1);
    for (uint32_t t = 0; t < w.nticks; ++t) {
        const uint32_t j = t;
        if (j < w.nchunks) {
            if (j + 2 < w.nchunks) load_set(nx2, j + 2);  // (the loads have two ticks to arrive)
            double(*T)[64] = w.tiles[j % kCascSlots];
            const int32_t s0 = (int32_t)(j * kCascChunk + part * kCascPart) - H;
            double xs[SET];
#pragma unroll
            for (uint32_t e = 0; e < SET; ++e) xs[e] = (double)cur[e];
            if (w.filt) {
#pragma unroll
                for (uint32_t e = 0; e < kCascPart; ++e) T[part * kCascPart + e][w.lane] = xs[H + e];
            } else {
                if (s0 < 0) {  // (wave-uniform: the first producer's first set; element e < H is the input H - e in front of the run)
#pragma unroll
                    for (int e = 0; e < H; ++e) xs[e] = x[H - 1 - e];
                }
                by_nc(c.nc, [&](auto ncv) {
#pragma unroll
                    for (uint32_t e = 0; e < kCascPart; ++e) T[part * kCascPart + e][w.lane] = iir_ff<decltype(ncv)::value>(c.d, &xs[H + e]);
                });
                const int32_t last = (int32_t)w.ns - 1 - (s0 + H);  // index of sample ns - 1 in this wave's part
                if constexpr (PLANAR) {
                    // (the run's last inputs go to the state below, straight from the matrix: picked out of the set by index, as
                    // in the native form, they cost this kernel 16 spilled VGPRs)
                } else if (CARRY && j + 1 == w.nchunks && last >= 0 && last < (int32_t)kCascPart) {  // whoever holds the run's last sample
                    have_last = true;
#pragma unroll
                    for (int i = 0; i < 5; ++i) {
                        double v = 0.0;
#pragma unroll
                        for (uint32_t e = 0; e < SET; ++e)
                            if ((int32_t)e == last + H - i) v = xs[e];
                        x[i] = v;
                    }
                }
            }
#pragma unroll
            for (uint32_t e = 0; e < SET; ++e) {
                cur[e] = nxt[e];
                nxt[e] = nx2[e];
            }
        }
        if constexpr (PLANAR) {
            // The x ring behind the run: its last nc samples.  At tick 1 nothing of the matrix is filtered yet -- the store wave's
            // first tick is 2 S >= 2 (k_iir_cascade_pipe_body.hpp: w.off) -- and a pipelined run has kCascChunk rows and more, so
            // the nc <= 5 samples exist and are the inputs.  The second producer writes them behind the first barrier: the first
            // one has read the carried ring in front of it, and nobody else reads these places.
            static_assert(kCascChunk >= 5 && kCascProd >= 2, "a pipelined run holds a ring's five inputs; a second producer writes them");
            if (CARRY && t == 1u && part == 1u && !w.filt && w.valid) {
                for (uint32_t i = 0; i < c.nc; ++i) w.cs->x[i] = (double)*w.run.at(w.ns - 1u - i);
            }
        }
        __syncthreads();
    }
    // (behind the last barrier: the other producer has long read the ring, also in a run of one chunk)
    if (CARRY && have_last && w.valid) {
        for (uint32_t i = 0; i < c.nc; ++i) w.cs->x[i] = x[i];
    }
}

// the store wave: the last section's outputs, truncated as C truncates them, once
template <int BPS, bool ALIGNED, bool CARRY, class W>
__device__ __forceinline__ void casc_wave_store(const W& w) {
    constexpr bool PLANAR = std::is_same<W, CascWavePlanar>::value;
    for (uint32_t t = 0; t < w.nticks; ++t) {
        const uint32_t j = t - w.off;
        if (j < w.nchunks) {
            double(*T)[64] = w.tiles[j % kCascSlots];
            const uint32_t cnt = w.count(j);
            uint8_t* q = w.p + (size_t)j * kCascChunk * w.stride;
            if constexpr (PLANAR) {
#pragma unroll 1
                for (uint32_t e0 = 0; e0 < cnt; e0 += kCascGroup) {
                    int32_t o[kCascGroup];
#pragma unroll
                    for (uint32_t e = 0; e < kCascGroup; ++e) o[e] = trunc_i32_c(T[e0 + e][w.lane]);
                    planar_store_part<!CARRY>(w.run, j * kCascChunk + e0, min(kCascGroup, cnt - e0), o, w.valid);
                }
            } else if (cnt == kCascChunk) {
#pragma unroll 1
                for (uint32_t e0 = 0; e0 < kCascChunk; e0 += kCascGroup) {
                    double v[kCascGroup];
#pragma unroll
                    for (uint32_t e = 0; e < kCascGroup; ++e) v[e] = T[e0 + e][w.lane];
                    if (w.valid) {
#pragma unroll
                        for (uint32_t e = 0; e < kCascGroup; ++e) sample_store<BPS>(q + (size_t)(e0 + e) * w.stride, trunc_i32_c(v[e]), ALIGNED);
                    }
                }
            } else {
                for (uint32_t e = 0; e < cnt; ++e) {
                    const double v = T[e][w.lane];
                    if (w.valid) sample_store<BPS>(q + (size_t)e * w.stride, trunc_i32_c(v), ALIGNED);
                }
            }
        }
        __syncthreads();
    }
}

template <int BPS, bool ALIGNED, bool CARRY>
__global__ __launch_bounds__(kCascMaxThreads) void k_iir_cascade_pipe(uint8_t* __restrict__ buf, uint32_t nch, uint32_t ns, uint64_t block_bytes, CascadeArgs a,
                                                                      uint32_t nblocks, IirCarry* __restrict__ state) {
    constexpr bool PLANAR = false;
#include "k_iir_cascade_pipe_body.hpp"
}

template <bool CARRY>
__global__ __launch_bounds__(kCascMaxThreads) void k_iir_cascade_pipe_planar(uint8_t* __restrict__ buf, uint32_t nch, uint32_t ns, uint64_t block_bytes,
                                                                             CascadeArgs a, uint32_t nblocks, IirCarry* __restrict__ state) {
    constexpr int BPS = 4;
    constexpr bool ALIGNED = true, PLANAR = true;
#include "k_iir_cascade_pipe_body.hpp"
}

}  // namespace rspt

#pragma clang fp contract(fast)
