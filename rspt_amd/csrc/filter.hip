// filter.hip -- the IIR pre-filter stage in front of the packers.
//
// Restates i_filter::new_iir / init_history_values / filter / filter_opt of lib_rspt/lib_filter/iir_filter.cpp:46-116 as the
// reference's test harness drives them (lib_rspt_test/rspt_test.cpp:116-136): per channel, 4 * nr_samples copies of the
// channel's first sample through filter(), then filter_opt() on every sample, the double result truncated to int32 and
// written back in the native sample width.  Double arithmetic in the reference's order of operations, every product and sum
// rounded on its own, so the filtered block is bit-identical with the reference's.  The filter object itself (IirState: filter,
// filter_opt, init_history_values) and the reason for `#pragma clang fp contract(off)` are stated in iir.hpp.
//
// Two modes, because the harness shares ONE filter object between the channels and its state runs on from channel to channel
// (the history initialisation damps the old state by ~e^-10, it does not erase it: on the 24-bit test recording the carried
// state moves a third of the samples, by up to 2569 counts):
//   shared       bit-exact with the harness; the channels of a block are a serial chain, so one thread takes one block
//   per channel  a fresh filter per channel (what a caller with one i_filter per channel gets): one thread per channel,
//                lane <-> channel so that every wave access is a contiguous row segment of the interleaved block
#include "iir.hpp"

// NO contraction in this file: iir.hpp says why.
#pragma clang fp contract(off)

namespace rspt {

// One channel: history initialisation with its first sample, then every sample in place through filter_opt, whose
// feed-forward sum has no output in it (IirState::step_opt).  Samples are handled in chunks of CH: the next
// chunk's loads are in flight while this one is filtered, the feed-forward sums of the chunk are independent work the
// scheduler places into the latency of the dependent chain, and the results leave as one store per sample.
// INIT = false: the history is the caller's (a carried state), the samples follow whatever f holds.
template <int BPS, int NC, bool INIT = true>
__device__ __forceinline__ void iir_channel(uint8_t* p, size_t stride, uint32_t ns, const IirCoef& c, IirState<NC>& f, bool aligned) {
    if (INIT) f.init_history(c, (double)sample_load<BPS>(p, aligned));
    constexpr uint32_t CH = 16;
    int32_t cur[CH], nxt[CH];
    const uint32_t nfull = ns / CH;
    if (nfull) {
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) cur[e] = sample_load<BPS>(p + (size_t)e * stride, aligned);
    }
    for (uint32_t k = 0; k < nfull; ++k) {
        uint8_t* q = p + (size_t)k * CH * stride;
        if (k + 1 < nfull) {
#pragma unroll
            for (uint32_t e = 0; e < CH; ++e) nxt[e] = sample_load<BPS>(q + (size_t)(CH + e) * stride, aligned);
        }
        // feed-forward sums of the chunk (xs[e + NC - 1] = sample e of the chunk, the NC - 1 values in front come from the state)
        double xs[CH + NC - 1], ff[CH];
#pragma unroll
        for (int i = 0; i < NC - 1; ++i) xs[i] = f.x[NC - 2 - i];
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) xs[NC - 1 + e] = (double)cur[e];
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) ff[e] = iir_ff<NC>(c.d, &xs[NC - 1 + e]);
        // the recurrence, then one store per sample
        int32_t out[CH];
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) out[e] = trunc_i32_c(f.feedback(c.n, ff[e]));  // C truncation (rspt_test.cpp:130)
#pragma unroll
        for (int i = 0; i < NC; ++i) f.x[i] = xs[CH + NC - 2 - i];  // the last NC inputs, newest first
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) sample_store<BPS>(q + (size_t)e * stride, out[e], aligned);
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) cur[e] = nxt[e];
    }
    for (uint32_t s = nfull * CH; s < ns; ++s) {  // the tail, sample by sample
        uint8_t* q = p + (size_t)s * stride;
        sample_store<BPS>(q, trunc_i32_c(f.step_opt(c.n, c.d, (double)sample_load<BPS>(q, aligned))), aligned);
    }
}

template <int BPS, int NC, bool SHARED>
__global__ __launch_bounds__(64) void k_iir(uint8_t* __restrict__ buf, uint32_t nch, uint32_t ns, uint64_t block_bytes, IirCoef c, uint32_t nblocks) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    IirState<NC> f;
    f.clear();
    const size_t stride = (size_t)nch * BPS;
    // (wave-uniform: every block base and every row start is aligned when the first one is and the sizes are multiples)
    const bool aligned = (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(buf) % BPS) == 0 && (block_bytes % BPS) == 0;
    if (SHARED) {  // one filter object for all channels of the block, as in the harness
        if (t >= nblocks) return;
        for (uint32_t ch = 0; ch < nch; ++ch) iir_channel<BPS, NC>(buf + (size_t)t * block_bytes + (size_t)ch * BPS, stride, ns, c, f, aligned);
    } else {
        const uint32_t b = t / nch, ch = t - b * nch;
        if (b >= nblocks) return;
        iir_channel<BPS, NC>(buf + (size_t)b * block_bytes + (size_t)ch * BPS, stride, ns, c, f, aligned);
    }
}

// The carried form of k_iir (calls of fewer than 64 rows): one thread per channel of ONE run of ns rows (the blocks of a call lie
// back to back, so they are one interleaved block of nblocks * ns rows).  A channel that has started continues from its rings;
// one that has not runs init_history_values on the call's first sample.  The rings are saved when the call ends.
template <int BPS, int NC>
__global__ __launch_bounds__(64) void k_iir_carry(uint8_t* __restrict__ buf, uint32_t nch, uint32_t ns, IirCoef c, IirCarry* __restrict__ state) {
    const uint32_t ch = blockIdx.x * 64u + threadIdx.x;
    if (ch >= nch) return;
    const size_t stride = (size_t)nch * BPS;
    const bool aligned = (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(buf) % BPS) == 0;
    uint8_t* p = buf + (size_t)ch * BPS;
    IirCarry& s = state[ch];
    IirState<NC> f;
    if (s.started) {
        f.load(s.x, s.y);
        iir_channel<BPS, NC, false>(p, stride, ns, c, f, aligned);
    } else {
        f.clear();
        iir_channel<BPS, NC, true>(p, stride, ns, c, f, aligned);
    }
    f.store(s.x, s.y);
    s.started = 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The pipelined form.  A lone wave issues one instruction every ~2 ns whatever it is (tools/issue_rate.hip), so the time of a
// channel is its sample count times the instructions the wave that HOLDS THE FILTER STATE has to issue per sample.  k_iir above
// issues everything from that wave (load, conversion, 2 NC - 1 feed-forward operations, 2 (NC - 1) feedback operations,
// conversion, store: ~22 instructions, 6.6 ms for the 64-block batch).  Here a workgroup of six waves splits the work, lane <->
// channel (or lane <-> block in shared mode) in all of them:
//   wave 0      the recurrence alone: per sample one LDS read of the feed-forward sum, NC - 1 products, NC - 1 subtractions, the
//               truncation and one LDS write -- and the history initialisation at the start of every channel
//   waves 1-4   load the samples (two chunks ahead), convert them and form the feed-forward sums of a quarter chunk each
//               (every product and sum rounded on its own, in the reference's left-to-right order) into LDS
//   wave 5      stores the filtered samples of the chunk before
// One workgroup barrier per chunk of 64 samples; the chunk being produced, the one in the recurrence and the one being stored
// live in double-buffered LDS tiles [sample][lane] (conflict-free).  Needs ns >= 64 and init_steps >= NC - 1 (else k_iir).
//
// CARRY (rspt_hip_iir_prefilter_stream_dev): per-channel driving of ONE run of ns rows (nblocks = 1: the blocks of the call back to
// back), the filter of channel ch living in state[ch].  A channel that has started loads its y ring instead of the history
// initialisation, and the first producer's first set takes the NC - 1 inputs in front of the call from the state's x ring (in
// place those rows are long overwritten); a channel that has not started runs init_history_values, and what its x ring then
// holds -- x0 in the first min(init_steps, NC) places, 0.0 behind them -- stands in front of the call, so any init_steps will
// do.  Whoever holds the run's last sample hands the last NC inputs on through L.xlast, as shared mode does for the next
// channel, and the recurrence wave writes both rings back behind the last chunk.  The state is read before the first barrier
// and written behind the last chunk's, by the workgroup that owns the channel.
//
// The recurrence (IirState::feedback) and the steps of the history initialisation come from iir.hpp.  The initialisation's
// loop, the producers' clamped set load and feed-forward sums (iir_ff: it moved the four unaligned int24 per-channel
// instantiations) and the selection of the run's last inputs are written out here, as in k_iir_cascade_pipe: moved into
// functions of their own, each of them compiled to other instructions (up to +-34 per instantiation, other register counts),
// and this kernel is kept instruction for instruction what was timed.
constexpr uint32_t kIirChunk = 64, kIirProd = 4, kIirPart = kIirChunk / kIirProd;  // four producer waves, 16 samples of a chunk each
constexpr uint32_t kIirThreads = 64 * (2 + kIirProd);
struct IirPipeLds {
    double ff[2][kIirChunk][64];
    int32_t out[2][kIirChunk][64];
    double xlast[5][64];  // the channel's last inputs, newest first (shared mode: the x ring the next channel's initialisation starts from)
};
// ~98.5 KiB of static LDS: one workgroup per CU, and only on a part with more than 64 KiB per workgroup (gfx950: 160 KiB)
static_assert(sizeof(IirPipeLds) <= 160 * 1024, "k_iir_pipe: the tiles must fit one CU's LDS");

template <int BPS, int NC, bool SHARED, bool ALIGNED, bool CARRY = false>
__global__ __launch_bounds__(kIirThreads) void k_iir_pipe(uint8_t* __restrict__ buf, uint32_t nch, uint32_t ns, uint64_t block_bytes, IirCoef c, uint32_t nblocks,
                                                 uint32_t lanes_per_wg, IirCarry* __restrict__ state) {
    static_assert(NC >= 2 && NC <= 5, "IirPipeLds::xlast holds five inputs per channel");
    static_assert(!(SHARED && CARRY), "a carried state is one filter per channel");
    __shared__ IirPipeLds L;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t role = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // lanes_per_wg < 64 spreads the lanes over more workgroups: in shared mode a lane is a BLOCK, its accesses are 16 MiB apart
    // from its neighbours', and 64 of them per CU would ask one CU's memory path for more than it can give
    const uint32_t unit = blockIdx.x * lanes_per_wg + lane;
    uint32_t b, ch0, nser;
    if (SHARED) {
        b = unit;
        ch0 = 0;
        nser = nch;
    } else {
        b = unit / nch;
        ch0 = unit - b * nch;
        nser = 1;
    }
    // six waves on four SIMDs: the wave with the recurrence shares its SIMD with a producer -- it goes first whenever it can issue
    if (role == 0u) __builtin_amdgcn_s_setprio(3);
    const bool valid = lane < lanes_per_wg && b < nblocks;  // (lanes past the batch read block 0 along with the others and store nothing)
    const size_t stride = (size_t)nch * BPS;
    constexpr bool aligned = ALIGNED;  // (the host has looked at the base address: one load / store instruction per sample)
    uint8_t* base = buf + (size_t)(valid ? b : 0u) * block_bytes + (size_t)(valid ? ch0 : 0u) * BPS;
    const uint32_t nchunks = (ns + kIirChunk - 1) / kIirChunk;
    IirState<NC> f;
    f.clear();
    constexpr int H = NC - 1;            // inputs in front of a sample that its feed-forward sum needs
    constexpr uint32_t SET = kIirPart + H;  // a producer's samples per chunk: its part and the H in front of it
    constexpr uint32_t kWriter = 1 + kIirProd;
    // (lanes past the shape look at channel 0's state along with it and write nothing)
    IirCarry* const cs = CARRY ? state + (valid ? ch0 : 0u) : nullptr;
    const bool started = CARRY && cs->started != 0;
    for (uint32_t sc = 0; sc < nser; ++sc) {
        uint8_t* p = base + (size_t)sc * BPS;
        const double x0 = (double)sample_load<BPS>(p, aligned);
        int32_t cur[SET], nxt[SET], nx2[SET];
        // element j of a producer's set in chunk t is sample t * 64 + (role - 1) * 16 - H + j; in front of the channel: the history (x0, see below)
        auto load_set = [&](int32_t (&v)[SET], uint32_t t) {
            const int32_t s0 = (int32_t)(t * kIirChunk + (role - 1u) * kIirPart) - H;
            if (s0 >= 0 && s0 + (int32_t)SET <= (int32_t)ns) {  // (wave-uniform; all but a channel's first and last sets)
                const uint8_t* q = p + (size_t)s0 * stride;
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) v[j] = sample_load<BPS>(q + (size_t)j * stride, aligned);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) {
                    int32_t si = s0 + (int32_t)j;
                    si = si < 0 ? 0 : si >= (int32_t)ns ? (int32_t)ns - 1 : si;  // (clamped: what lies outside is never used as such)
                    v[j] = sample_load<BPS>(p + (size_t)si * stride, aligned);
                }
            }
        };
        const bool producer = role >= 1u && role <= kIirProd;
        if (producer) {
            load_set(cur, 0);
            if (nchunks > 1) load_set(nxt, 1);
        }
        for (uint32_t t = 0; t < nchunks + 2; ++t) {
            if (role == 0u) {
                if (CARRY && t == 0 && started) {  // (the y ring alone: this wave never reads x, the first producer takes it from the state)
#pragma unroll
                    for (int i = 0; i < NC; ++i) f.y[i] = cs->y[i];
                } else if (t == 0) {
                    // IirState::init_history, written out: as a call it compiles to other code here (see above the kernel)
                    int32_t i = 0;
                    for (; i < c.init_steps && i < NC; ++i) f.step(c.n, c.d, x0);  // (until the x ring holds nothing but x0)
                    if (i < c.init_steps) {
                        double P[NC];
#pragma unroll
                        for (int k = 0; k < NC; ++k) P[k] = c.d[k] * x0;
                        // (unrolled by the ring's length: the shifts of y become register names instead of moves)
#pragma unroll 4
                        for (; i < c.init_steps; ++i) f.step_const(c.n, P);
                    }
                } else if (t <= nchunks) {
                    const uint32_t k = t - 1, bi = k & 1u;
                    const uint32_t cnt = min(kIirChunk, ns - k * kIirChunk);
                    auto rec = [&](double ff) { return f.feedback(c.n, ff); };
                    if (cnt == kIirChunk) {
                        // sixteen samples at a time: their feed-forward sums are read from LDS together (one wait), the results
                        // written together -- per sample the wave issues the recurrence and little else.  The truncation is the
                        // GPU's own (saturating) conversion here; C's as the reference's build does it (trunc_i32_c, common.hpp) differs
                        // from it only where this conversion returns INT_MAX (the double is >= 2^31 or +inf) and where the double
                        // is NaN (this conversion: 0).  The largest result of the chunk is tracked (half an instruction per sample
                        // instead of two); a NaN needs no tracking, because it is absorbing: the step after it multiplies it by
                        // n[1], so every later output is NaN and the chunk's last one says whether any was (its high word: an
                        // all-ones exponent, NaN or +-inf).  A chunk that reaches INT_MAX -- full-scale input through a filter that
                        // overshoots -- or ends non-finite -- an unstable filter, non-finite coefficients -- is done once more, exactly.
                        double ysave[NC];
#pragma unroll
                        for (int i = 0; i < NC; ++i) ysave[i] = f.y[i];
                        int32_t mx = (int32_t)0x80000000u;
#pragma unroll 1
                        for (uint32_t e0 = 0; e0 < kIirChunk; e0 += 16) {
                            double a[16];
                            int32_t o[16];
#pragma unroll
                            for (uint32_t e = 0; e < 16; ++e) a[e] = L.ff[bi][e0 + e][lane];
#pragma unroll
                            for (uint32_t e = 0; e < 16; ++e) o[e] = (int32_t)rec(a[e]);
#pragma unroll
                            for (uint32_t e = 0; e < 16; e += 2) mx = max(mx, max(o[e], o[e + 1]));  // (v_max3_i32)
#pragma unroll
                            for (uint32_t e = 0; e < 16; ++e) L.out[bi][e0 + e][lane] = o[e];
                        }
                        if (__builtin_expect(__builtin_amdgcn_ballot_w64(mx == 0x7FFFFFFF || (__double2hiint(f.y[0]) & 0x7FF00000) == 0x7FF00000) != 0ull, 0)) {
#pragma unroll
                            for (int i = 0; i < NC; ++i) f.y[i] = ysave[i];
#pragma unroll 1
                            for (uint32_t e = 0; e < kIirChunk; ++e) L.out[bi][e][lane] = trunc_i32_c(rec(L.ff[bi][e][lane]));
                        }
                    } else {
                        for (uint32_t e = 0; e < cnt; ++e) L.out[bi][e][lane] = trunc_i32_c(rec(L.ff[bi][e][lane]));  // C truncation (rspt_test.cpp:130)
                    }
                    if (SHARED && t == nchunks) {  // the x ring the next channel's initialisation starts from (its first NC - 1 calls see it)
#pragma unroll
                        for (int i = 0; i < NC; ++i) f.x[i] = L.xlast[i][lane];
                    }
                    if (CARRY && t == nchunks && valid) {  // the object as it stands behind the call's last sample
#pragma unroll
                        for (int i = 0; i < NC; ++i) {
                            cs->x[i] = L.xlast[i][lane];
                            cs->y[i] = f.y[i];
                        }
                        cs->started = 1;
                    }
                }
            } else if (role == kWriter) {
                if (t >= 2) {
                    const uint32_t k = t - 2, bi = k & 1u;
                    const uint32_t cnt = min(kIirChunk, ns - k * kIirChunk);
                    uint8_t* q = p + (size_t)k * kIirChunk * stride;
                    if (cnt == kIirChunk) {
#pragma unroll 1
                        for (uint32_t e0 = 0; e0 < kIirChunk; e0 += 16) {
                            int32_t v[16];
#pragma unroll
                            for (uint32_t e = 0; e < 16; ++e) v[e] = L.out[bi][e0 + e][lane];
                            if (valid) {
#pragma unroll
                                for (uint32_t e = 0; e < 16; ++e) sample_store<BPS>(q + (size_t)(e0 + e) * stride, v[e], aligned);
                            }
                        }
                    } else {
                        for (uint32_t e = 0; e < cnt; ++e) {
                            const int32_t v = L.out[bi][e][lane];
                            if (valid) sample_store<BPS>(q + (size_t)e * stride, v, aligned);
                        }
                    }
                }
            } else if (t < nchunks) {
                if (t + 2 < nchunks) load_set(nx2, t + 2);  // (two chunks ahead: the loads have two ticks to arrive)
                // the inputs as doubles; in front of the channel's first sample the x ring holds x0 (init_steps >= NC - 1: the host checks)
                const int32_t s0 = (int32_t)(t * kIirChunk + (role - 1u) * kIirPart) - H;
                double xs[SET];
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) xs[j] = (double)cur[j];
                if (s0 < 0) {  // (wave-uniform: the first producer's first set only)
#pragma unroll
                    for (uint32_t j = 0; j < SET; ++j) xs[j] = (s0 + (int32_t)j < 0) ? x0 : xs[j];
                    if (CARRY) {  // (s0 = -H: element j < H is the input H - j samples in front of the call, place H - 1 - j of the x ring)
#pragma unroll
                        for (int j = 0; j < H; ++j) xs[j] = started ? cs->x[H - 1 - j] : (H - 1 - j < c.init_steps ? x0 : 0.0)  /* iir_front: the place is below NC */;
                    }
                }
#pragma unroll
                for (uint32_t e = 0; e < kIirPart; ++e) {  // (iir_ff, written out)
                    double a = c.d[0] * xs[H + e];
#pragma unroll
                    for (int i = 1; i < NC; ++i) a = a + c.d[i] * xs[H + e - i];
                    L.ff[t & 1u][(role - 1u) * kIirPart + e][lane] = a;
                }
                if ((SHARED || CARRY) && t + 1 == nchunks) {  // whoever holds the channel's last sample hands its last inputs on
                    const int32_t last = (int32_t)ns - 1 - (s0 + H);  // index of sample ns-1 in this wave's part
                    if (last >= 0 && last < (int32_t)kIirPart) {
#pragma unroll
                        for (int i = 0; i < NC; ++i) {
                            double v = 0.0;
#pragma unroll
                            for (uint32_t j = 0; j < SET; ++j)
                                if ((int32_t)j == last + H - i) v = xs[j];
                            L.xlast[i][lane] = v;
                        }
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
}

}  // namespace rspt

#pragma clang fp contract(fast)
