// iir_zero_phase.hip -- the zero-phase (forward-backward) IIR stage: one reference filter object per (block, channel) run forward
// over the block and then backward over its own untruncated outputs, truncated once (rspt_hip_iir_zero_phase_batch_dev, and
// rspt_hip_iir_zero_phase_planar_batch_dev on the converters' int32 matrix; semantics: rspt_hip.h).
//
// The reference's offline user runs a filter forward and then backward over the SAME object (peak_detector.h:309-328), so the
// rings run on through the turn:
//     f = i_filter::new_iir(n, d, nc);  f->init_history_values((double)x[0], init)
//     for t = 0 .. ns-1:   w[t] = f->filter_opt((double)x[t])
//     f->init_history_values(w[ns-1], backward_init)               -- 4 * backward_init calls of filter(); it does not reset the rings
//     for t = ns-1 .. 0:   w[t] = f->filter_opt(w[t])
//     y[t] = (int32_t)w[t]
// What the object holds at the turn: the y ring the forward pass's last outputs, the x ring the forward pass's last INPUTS -- the
// raw samples x[ns-1], x[ns-2], ... as doubles (and behind a block shorter than the ring what init_history_values left there).
// The backward pass's first feed-forward sums see them as the inputs "in front".  w stays double between the passes, in a
// caller-owned workspace laid out as k_peak_offline's: a slab double [ns][64] per wave of 64 lanes, element t of lane l at
// [t * 64 + l], so a wave touches 512 contiguous bytes per t whatever nch is.  The filter object (IirState) and the reason for
// `#pragma clang fp contract(off)` are stated in iir.hpp.
#include "iir.hpp"

// NO contraction in this file: iir.hpp says why.
#pragma clang fp contract(off)

namespace rspt {

// ---------------------------------------------------------------------------------------------------------------------------
// The plain kernel: one thread per (block, channel) runs both passes as written above.  It serves blocks of fewer rows than a
// chunk of the pipelined kernel and histories shorter than the ring.
template <int BPS, int NC>
__global__ __launch_bounds__(64) void k_iir_zp(uint8_t* __restrict__ buf, uint32_t nch, uint32_t ns, uint64_t block_bytes, IirCoef c, int32_t back_steps,
                                               uint32_t nblocks, double* work) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    const uint32_t b = t / nch, ch = t - b * nch;
    if (b >= nblocks) return;
    const size_t stride = (size_t)nch * BPS;
    const bool aligned = (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(buf) % BPS) == 0 && (block_bytes % BPS) == 0;
    uint8_t* p = buf + (size_t)b * block_bytes + (size_t)ch * BPS;
    double* W = work + (size_t)blockIdx.x * ns * 64u + threadIdx.x;  // this lane's column of its wave's slab
    IirState<NC> f;
    f.clear();
    f.init_history(c, (double)sample_load<BPS>(p, aligned));
    for (uint32_t s = 0; s < ns; ++s) W[(size_t)s * 64u] = f.step_opt(c.n, c.d, (double)sample_load<BPS>(p + (size_t)s * stride, aligned));
    // the turn: the same object, its rings as they stand, 4 * backward_init calls of filter() on the last forward output
    IirCoef cb = c;
    cb.init_steps = back_steps;
    f.init_history(cb, f.y[0]);
    for (uint32_t s = ns; s-- > 0;)
        sample_store<BPS>(p + (size_t)s * stride, trunc_i32_c(f.step_opt(c.n, c.d, W[(size_t)s * 64u])), aligned);  // C truncation, once
}

// k_iir_zp on the planar matrix (rspt_hip_iir_zero_phase_planar_batch_dev): row r = b * nch + ch of the converters' matrix
// [nblocks][nch][ns], sample s at r * ns + s, the whole int32 the sample and the result stored whole.  The forward pass only reads
// src and the backward pass only writes dst, so dst may be src itself (in place) or a matrix of its own.
template <int NC>
__global__ __launch_bounds__(64) void k_iir_zp_planar(const int32_t* src, int32_t* dst, uint32_t ns, IirCoef c, int32_t back_steps, uint32_t rows, double* work) {
    const uint32_t r = blockIdx.x * 64u + threadIdx.x;
    if (r >= rows) return;
    const int32_t* x = src + (size_t)r * ns;
    int32_t* y = dst + (size_t)r * ns;
    double* W = work + (size_t)blockIdx.x * ns * 64u + threadIdx.x;  // this lane's column of its wave's slab
    IirState<NC> f;
    f.clear();
    f.init_history(c, (double)x[0]);
    for (uint32_t s = 0; s < ns; ++s) W[(size_t)s * 64u] = f.step_opt(c.n, c.d, (double)x[s]);
    IirCoef cb = c;  // the turn, as in k_iir_zp
    cb.init_steps = back_steps;
    f.init_history(cb, f.y[0]);
    for (uint32_t s = ns; s-- > 0;) y[s] = trunc_i32_c(f.step_opt(c.n, c.d, W[(size_t)s * 64u]));  // C truncation, once
}

// ---------------------------------------------------------------------------------------------------------------------------
// The pipelined kernel, in the manner of k_iir_pipe (filter.hip): a workgroup of six waves, lane <-> (block, channel) in all of
// them, and the wave that holds the filter state issues only what depends on it.
//   wave 0      the recurrence through BOTH passes: per sample one LDS read of the feed-forward sum, NC - 1 products, NC - 1
//               subtractions and one LDS write of the untruncated double; the history initialisation in front of each pass
//   waves 1-4   the producers: a quarter chunk each.  Forward: load the samples (two chunks ahead), convert them, form the
//               feed-forward sums.  Backward: load the forward outputs from the workspace at descending t (two chunks ahead) and
//               form the feed-forward sums with the H = NC - 1 later-in-time values in front
//   wave 5      the writer.  Forward: stores the untruncated doubles to the workspace.  Backward: truncates (trunc_i32_c) and
//               stores native samples
// One workgroup barrier per chunk of 64 samples; a pass takes nchunks + 2 ticks (produce, recur, write) and the backward pass
// starts behind the forward pass's last tick, so the pipeline drains and refills once per channel: the barrier that ends the
// forward pass orders the writer's workspace stores in front of the producers' workspace loads (one workgroup, one CU).
// Backward chunk k holds the positions r = 64 k .. 64 k + 63 of the backward pass, r = ns - 1 - t: the partial chunk, if any, is
// the last one of each pass.
//
// The turn.  The recurrence wave keeps its y ring.  The producer that holds the forward pass's last sample hands the last NC
// inputs on through L.xlast (newest first: the x ring of the object at the turn).  With them the recurrence wave runs the
// backward history initialisation -- back_steps = 4 * backward_init calls of filter() on wl = w[ns-1], its own y[0] --, and the
// first producer's first backward set takes its H inputs "in front" from the x ring as it stands BEHIND that initialisation:
//     place i of the x ring = wl                       for i < min(back_steps, NC)
//                           = L.xlast[i - back_steps]   behind them: the forward pass's older inputs, pushed back by back_steps places
// (back_steps = 0: the forward pass's last H inputs, newest first -- neither zeros nor clamped reads).
//
// Needs ns >= 64 and a forward history that fills the ring's tail (the host checks; else k_iir_zp): in front of the channel's
// first sample the x ring then holds x0.  Lanes past the batch read block 0, channel 0 along with the others, keep a column of
// their own in the last slab (the workspace bound counts whole slabs) and store no sample.
//
// PLANAR (k_iir_zp_pipe_planar: the same ticks, roles and workspace; BPS = 4, aligned).  Lane <-> row r = b * nch + ch of the
// matrix [nblocks][nch][ns], sample s of the row 4 bytes behind sample s - 1, the next row -- another lane's, or another
// workgroup's -- directly behind the last sample.  Only two places see where a sample lives:
//   the forward producers   a set inside the row takes its H samples in front as dwords and its 16-sample part, 64 contiguous
//                           bytes, as four 16-byte loads that need the int32's alignment only (planar_load_set, filter.hip); a
//                           set at an end of the row goes dword by dword, its sample INDEX clamped into the row, never an address
//   the backward writer     the 16 outputs of a part lie at descending t: 64 contiguous bytes at ascending addresses, stored as
//                           four 16-byte stores in reversed register order.  Only whole chunks go that way (all 64 positions are
//                           samples of the row then); the partial last chunk is stored dword by dword, so no store passes
//                           either end of the row
// The producers read `buf` (the source) and the writer stores to `dst`, which is buf itself in place: x0 and every forward load
// are issued in front of the barrier that ends the forward pass and the first sample is stored behind it, as in the native
// kernel, so in place needs no staging and out of place costs nothing.  The backward producers, the forward writer, the
// recurrence wave, the turn and L.xlast never see a sample's address.
constexpr uint32_t kZpChunk = 64, kZpProd = 4, kZpPart = kZpChunk / kZpProd, kZpGroup = 16;
constexpr uint32_t kZpThreads = 64 * (2 + kZpProd);
constexpr uint32_t kZpWriter = 1 + kZpProd;
static_assert(kZpPart == kZpGroup && kZpChunk % kZpGroup == 0, "a producer takes one group of a chunk");
struct ZpLds {
    double ff[2][kZpChunk][64];   // feed-forward sums: producers -> recurrence
    double out[2][kZpChunk][64];  // untruncated outputs: recurrence -> writer
    double xlast[5][64];          // the forward pass's last inputs, newest first
};
// 130.5 KiB of static LDS: one workgroup per CU, on a part with 160 KiB per workgroup (gfx950)
static_assert(sizeof(ZpLds) <= 160 * 1024, "k_iir_zp_pipe: the tiles must fit one CU's LDS");

// What every wave knows about its lane's run.
struct ZpWave {
    uint8_t* p;     // the lane's first sample
    double* W;      // the lane's column of its wave's slab: w[t] at W[t * 64]
    size_t stride;  // bytes from one sample of the channel to the next
    uint32_t ns, nchunks, lane;
    bool valid;
    double x0;
    __device__ __forceinline__ uint32_t count(uint32_t k) const { return min(kZpChunk, ns - k * kZpChunk); }
};

// Each role is two tick loops of nchunks + 2 barriers, so that no role's registers live through another's.

// wave 0: the recurrence.  One chunk: sums -> outputs, sixteen at a time (read together, one wait; written together).
template <int NC>
__device__ __forceinline__ void zp_rec_chunk(ZpLds& L, uint32_t bi, uint32_t lane, uint32_t cnt, const IirCoef& c, IirState<NC>& f) {
    if (cnt == kZpChunk) {
#pragma unroll 1
        for (uint32_t e0 = 0; e0 < kZpChunk; e0 += kZpGroup) {
            double a[kZpGroup];
#pragma unroll
            for (uint32_t e = 0; e < kZpGroup; ++e) a[e] = L.ff[bi][e0 + e][lane];
#pragma unroll
            for (uint32_t e = 0; e < kZpGroup; ++e) a[e] = f.feedback(c.n, a[e]);
#pragma unroll
            for (uint32_t e = 0; e < kZpGroup; ++e) L.out[bi][e0 + e][lane] = a[e];
        }
    } else {
        for (uint32_t e = 0; e < cnt; ++e) L.out[bi][e][lane] = f.feedback(c.n, L.ff[bi][e][lane]);
    }
    // The chunk's LDS stores are complete before this wave reaches the tick's barrier.  __syncthreads() alone did not give that
    // here: in all 24 instantiations hipcc left the wait out on the paths from both loops above to the barrier
    // (tools/check_barrier_waits.py reported one unpublished barrier per instantiation; tests/test_stream_asm.py gates it).
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

template <int NC>
__device__ __forceinline__ void zp_wave_rec(ZpLds& L, const ZpWave& w, const IirCoef& c, int32_t back_steps) {
    IirState<NC> f;
    f.clear();
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t t = 0; t < w.nchunks + 2; ++t) {
            if (t == 0) {
                if (pass == 0) {
                    f.init_history(c, w.x0);
                } else {
                    // the same object at the turn: the y ring is this wave's, the x ring the forward pass's last inputs
#pragma unroll
                    for (int i = 0; i < NC; ++i) f.x[i] = L.xlast[i][w.lane];
                    IirCoef cb = c;
                    cb.init_steps = back_steps;
                    f.init_history(cb, f.y[0]);
                }
            } else if (t <= w.nchunks) {
                zp_rec_chunk<NC>(L, (t - 1) & 1u, w.lane, w.count(t - 1), c, f);
            }
            __syncthreads();
        }
    }
}

// waves 1-4: element j of a producer's set in chunk k is position k * 64 + part * 16 - H + j of the pass (forward: sample t = the
// position; backward: t = ns - 1 - the position); the set is its 16 positions and the H in front of them.
template <int BPS, int NC, bool ALIGNED, bool PLANAR = false>
__device__ __forceinline__ void zp_wave_prod(ZpLds& L, const ZpWave& w, const IirCoef& c, int32_t back_steps, uint32_t part) {
    constexpr int H = NC - 1;
    constexpr uint32_t SET = kZpPart + H;
    const int32_t ns = (int32_t)w.ns;
    auto first = [&](uint32_t k) { return (int32_t)(k * kZpChunk + part * kZpPart) - H; };
    // (clamped where a set reaches past the pass: what lies outside is never used as such)
    auto whole = [&](int32_t s0) { return s0 >= 0 && s0 + (int32_t)SET <= ns; };  // (wave-uniform; all but a pass's first and last sets)
    auto clamp = [&](int32_t s) { return s < 0 ? 0 : s >= ns ? ns - 1 : s; };
    // the feed-forward sums of the set's 16 positions into the chunk's tile
    auto sums = [&](uint32_t k, const double (&xs)[SET]) {
#pragma unroll
        for (uint32_t e = 0; e < kZpPart; ++e) L.ff[k & 1u][part * kZpPart + e][w.lane] = iir_ff<NC>(c.d, &xs[H + e]);
    };
    // ---- forward: native samples ----
    {
        int32_t cur[SET], nxt[SET], nx2[SET];
        auto load_set = [&](int32_t (&v)[SET], uint32_t k) {
            const int32_t s0 = first(k);
            if constexpr (PLANAR) {  // (w.p: the lane's row of the source matrix)
                planar_load_set<(uint32_t)H, true>(PlanarRun{reinterpret_cast<int32_t*>(w.p), w.ns, 0}, w.ns, s0, v);
                return;
            }
            if (whole(s0)) {
                const uint8_t* q = w.p + (size_t)s0 * w.stride;
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) v[j] = sample_load<BPS>(q + (size_t)j * w.stride, ALIGNED);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) v[j] = sample_load<BPS>(w.p + (size_t)clamp(s0 + (int32_t)j) * w.stride, ALIGNED);
            }
        };
        load_set(cur, 0);
        if (w.nchunks > 1) load_set(nxt, 1);
        for (uint32_t t = 0; t < w.nchunks + 2; ++t) {
            if (t < w.nchunks) {
                if (t + 2 < w.nchunks) load_set(nx2, t + 2);  // (two chunks ahead: the loads have two ticks to arrive)
                const int32_t s0 = first(t);
                double xs[SET];
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) xs[j] = (double)cur[j];
                if (s0 < 0) {  // (the first producer's first set: in front of the channel the x ring holds x0 -- the host checks the history)
#pragma unroll
                    for (uint32_t j = 0; j < SET; ++j) xs[j] = (s0 + (int32_t)j < 0) ? w.x0 : xs[j];
                }
                sums(t, xs);
                const int32_t last = ns - 1 - (s0 + H);  // index of sample ns - 1 in this wave's part
                if (t + 1 == w.nchunks && last >= 0 && last < (int32_t)kZpPart) {  // whoever holds the last sample hands the x ring on
#pragma unroll
                    for (int i = 0; i < NC; ++i) {
                        double v = 0.0;
#pragma unroll
                        for (uint32_t j = 0; j < SET; ++j)
                            if ((int32_t)j == last + H - i) v = xs[j];
                        L.xlast[i][w.lane] = v;
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) {
                    cur[j] = nxt[j];
                    nxt[j] = nx2[j];
                }
            }
            __syncthreads();
        }
    }
    // ---- backward: the forward outputs from the workspace, at descending t (behind the barrier that ended the forward pass) ----
    {
        double cur[SET], nxt[SET], nx2[SET];
        auto load_set = [&](double (&v)[SET], uint32_t k) {
            const int32_t r0 = first(k);
            if (whole(r0)) {
                const double* q = w.W + (size_t)(ns - 1 - r0) * 64u;
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) v[j] = *(q - (size_t)j * 64u);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) v[j] = w.W[(size_t)(ns - 1 - clamp(r0 + (int32_t)j)) * 64u];
            }
        };
        load_set(cur, 0);
        if (w.nchunks > 1) load_set(nxt, 1);
        for (uint32_t t = 0; t < w.nchunks + 2; ++t) {
            if (t < w.nchunks) {
                if (t + 2 < w.nchunks) load_set(nx2, t + 2);
                const int32_t r0 = first(t);
                double xs[SET];
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) xs[j] = cur[j];
                if (r0 < 0) {
                    // (the first producer's first set, r0 = -H: element j < H is the input H - j calls in front of the backward pass,
                    // place i = H - 1 - j of the x ring behind the backward history initialisation.  That ring holds wl = w[ns-1] in
                    // its first min(back_steps, NC) places and the forward pass's last INPUTS, newest first, behind them.)
                    const double wl = xs[H];
#pragma unroll
                    for (int j = 0; j < H; ++j) {
                        const int i = H - 1 - j;
                        xs[j] = i < back_steps ? wl : L.xlast[i - back_steps][w.lane];
                    }
                }
                sums(t, xs);
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) {
                    cur[j] = nxt[j];
                    nxt[j] = nx2[j];
                }
            }
            __syncthreads();
        }
    }
}

// wave 5: the writer
template <int BPS, bool ALIGNED, bool PLANAR = false>
__device__ __forceinline__ void zp_wave_write(ZpLds& L, const ZpWave& w) {
    // forward: the untruncated doubles to the workspace
    for (uint32_t t = 0; t < w.nchunks + 2; ++t) {
        if (t >= 2) {
            const uint32_t k = t - 2, bi = k & 1u, cnt = w.count(k);
            double* q = w.W + (size_t)k * kZpChunk * 64u;
            if (cnt == kZpChunk) {
#pragma unroll 1
                for (uint32_t e0 = 0; e0 < kZpChunk; e0 += kZpGroup) {
                    double v[kZpGroup];
#pragma unroll
                    for (uint32_t e = 0; e < kZpGroup; ++e) v[e] = L.out[bi][e0 + e][w.lane];
#pragma unroll
                    for (uint32_t e = 0; e < kZpGroup; ++e) q[(size_t)(e0 + e) * 64u] = v[e];
                }
            } else {
                for (uint32_t e = 0; e < cnt; ++e) q[(size_t)e * 64u] = L.out[bi][e][w.lane];
            }
        }
        __syncthreads();
    }
    // backward: position r of the pass is sample ns - 1 - r; C truncation, once
    for (uint32_t t = 0; t < w.nchunks + 2; ++t) {
        if (t >= 2) {
            const uint32_t k = t - 2, bi = k & 1u, cnt = w.count(k);
            uint8_t* q = w.p + (size_t)(w.ns - 1u - k * kZpChunk) * w.stride;  // position k * 64; the chunk goes downwards from it
            if (cnt == kZpChunk) {
#pragma unroll 1
                for (uint32_t e0 = 0; e0 < kZpChunk; e0 += kZpGroup) {
                    double v[kZpGroup];
#pragma unroll
                    for (uint32_t e = 0; e < kZpGroup; ++e) v[e] = L.out[bi][e0 + e][w.lane];
                    if constexpr (PLANAR) {
                        // (a whole chunk: its 64 positions are samples of the row, so the group's 16 are the 64 bytes that end
                        // with sample ns - 1 - (k * 64 + e0), in reversed order)
                        int32_t r[kZpGroup];
#pragma unroll
                        for (uint32_t e = 0; e < kZpGroup; ++e) r[kZpGroup - 1u - e] = trunc_i32_c(v[e]);
                        if (w.valid) __builtin_memcpy(q - (size_t)(e0 + kZpGroup - 1u) * 4u, &r[0], 64);
                        continue;
                    }
                    if (w.valid) {
#pragma unroll
                        for (uint32_t e = 0; e < kZpGroup; ++e) sample_store<BPS>(q - (size_t)(e0 + e) * w.stride, trunc_i32_c(v[e]), ALIGNED);
                    }
                }
            } else {
                for (uint32_t e = 0; e < cnt; ++e) {
                    const double v = L.out[bi][e][w.lane];
                    if (w.valid) sample_store<BPS>(q - (size_t)e * w.stride, trunc_i32_c(v), ALIGNED);
                }
            }
        }
        __syncthreads();
    }
}

// The body is a file of its own (k_iir_zp_pipe_body.hpp), included once into the native kernel and once into its planar form
// with every planar statement under `if constexpr (PLANAR)`, as filter.hip's are and for its reason: the native instantiations
// keep their names and are compiled from the statements they had (tools/isa_diff.py).
template <int BPS, int NC, bool ALIGNED>
__global__ __launch_bounds__(kZpThreads) void k_iir_zp_pipe(uint8_t* __restrict__ buf, uint32_t nch, uint32_t ns, uint64_t block_bytes, IirCoef c,
                                                          int32_t back_steps, uint32_t nblocks, double* work) {
    constexpr bool PLANAR = false;
    uint8_t* const dst = buf;
#include "k_iir_zp_pipe_body.hpp"
}

// buf: the source matrix, only read; dst: where the result goes, buf itself in place (so neither is __restrict__); block_bytes:
// one [nch][ns] block of the matrix.
template <int NC>
__global__ __launch_bounds__(kZpThreads) void k_iir_zp_pipe_planar(uint8_t* buf, uint8_t* dst, uint32_t nch, uint32_t ns, uint64_t block_bytes, IirCoef c,
                                                                 int32_t back_steps, uint32_t nblocks, double* work) {
    constexpr int BPS = 4;
    constexpr bool ALIGNED = true, PLANAR = true;
#include "k_iir_zp_pipe_body.hpp"
}

}  // namespace rspt

#pragma clang fp contract(fast)
