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

// ---------------------------------------------------------------------------------------------------------------------------
// The planar form (rspt_hip_iir_*_planar_*_dev): the samples are the whole int32 values of the converters' matrix
// [nblocks][nch][ns], filtered in place and stored whole.  Only where a sample of a run lives is new: the kernels below and
// those of iir_cascade.hip take it as a flag PLANAR (BPS = 4, aligned), and the filter, the ticks and the routes are the native
// ones.  The bodies of the three larger kernels are files of their own (k_iir_pipe_body.hpp, k_iir_cascade_body.hpp,
// k_iir_cascade_pipe_body.hpp), included once into the native kernel and once into its planar form, with every planar statement
// under `if constexpr (PLANAR)`: the native instantiations keep their names and are compiled from the statements they had.
// A run is channel ch's row of one block (stateless), or its rows in the call's consecutive blocks (carried).
// A neighbouring channel's row is adjacent in memory and another lane or workgroup is filtering it, so nothing here stores
// past the end of a row, and a clamped load clamps the sample's INDEX in the run, never an address.
struct PlanarRun {
    int32_t* row;   // the run's first sample: the channel's row in the run's first block
    uint32_t hns;   // samples of a row
    size_t bstep;   // elements from a row to the same channel's row in the next block: nch * hns
    // sample s of the run sits at (s / hns) * nch * hns + ch * hns + s % hns of the matrix
    __device__ __forceinline__ int32_t* at(uint32_t s) const {
        const uint32_t b = s / hns;
        return row + (size_t)b * bstep + (s - b * hns);
    }
    // samples s .. s + n - 1 where they lie in one row, else nullptr (wave-uniform: s, n and hns are)
    __device__ __forceinline__ int32_t* span(uint32_t s, uint32_t n) const {
        const uint32_t b = s / hns, r = s - b * hns;
        return r + n <= hns ? row + (size_t)b * bstep + r : nullptr;
    }
};
// The run whose first sample is p.  block_bytes is one [nch][hns] block of the matrix; stateless (ONE_ROW) the run is one row of
// ns samples, carried it is ns rows through ns / hns consecutive blocks.  (nch * hns < 2^31, rspt_hip_packer_create: a 32-bit
// division, whose expansion holds no fused multiply-add as a 64-bit one's does.)
template <bool ONE_ROW>
__device__ __forceinline__ PlanarRun planar_run(uint8_t* p, uint32_t nch, uint32_t ns, uint64_t block_bytes) {
    const uint32_t hns = ONE_ROW ? ns : (uint32_t)(block_bytes >> 2) / nch;
    return PlanarRun{reinterpret_cast<int32_t*>(p), hns, (size_t)nch * hns};
}

// A producer's set of a run of ns samples: the H samples in front of its part and its 16-sample part, from sample s0 on.  A
// set inside the run and inside one row takes the H in front as dwords and the part -- 64 contiguous bytes -- as four 16-byte
// loads, which need the 4-byte alignment of an int32 only (as k_planar_stream's do).  A set at an end of the run (its indices
// clamped into the run: what lies outside is never used as such) or across a block boundary goes dword by dword.
// ONE_ROW: the run is one row (the stateless forms), no set straddles.
template <uint32_t H, bool ONE_ROW>
__device__ __forceinline__ void planar_load_set(const PlanarRun& run, uint32_t ns, int32_t s0, int32_t (&v)[16 + H]) {
    const int32_t* q = nullptr;
    if (s0 >= 0 && s0 + (int32_t)(16 + H) <= (int32_t)ns) q = ONE_ROW ? run.row + s0 : run.span((uint32_t)s0, 16 + H);
    if (q) {  // (wave-uniform)
#pragma unroll
        for (uint32_t j = 0; j < H; ++j) v[j] = q[j];
        __builtin_memcpy(&v[H], q + H, 64);
    } else if constexpr (ONE_ROW) {
#pragma unroll
        for (uint32_t j = 0; j < 16 + H; ++j) {
            const int32_t si = s0 + (int32_t)j;
            v[j] = run.row[si < 0 ? 0 : si >= (int32_t)ns ? (int32_t)ns - 1 : si];
        }
    } else {
        // (one division for the set: the place of its first sample, and from there on step by step)
        const int32_t first = s0 < 0 ? 0 : s0 >= (int32_t)ns ? (int32_t)ns - 1 : s0;
        uint32_t b = (uint32_t)first / run.hns, r = (uint32_t)first - b * run.hns;
#pragma unroll
        for (uint32_t j = 0; j < 16 + H; ++j) {
            v[j] = run.row[(size_t)b * run.bstep + r];
            const int32_t si = s0 + (int32_t)j;
            if (si >= 0 && si + 1 < (int32_t)ns && ++r == run.hns) {  // (the next element is the next sample; its row may be the next block's)
                r = 0;
                ++b;
            }
        }
    }
}

// The first n <= 16 of a writer's 16 results, from sample s of the run on: a whole part inside one row as four 16-byte stores,
// else dword by dword -- never a byte past sample s + n - 1, which may be the row's last.
template <bool ONE_ROW>
__device__ __forceinline__ void planar_store_part(const PlanarRun& run, uint32_t s, uint32_t n, const int32_t (&v)[16], bool valid) {
    int32_t* q = nullptr;
    if (n == 16u) q = ONE_ROW ? run.row + s : run.span(s, 16u);
    if (!valid) return;
    if (q) {  // (wave-uniform)
        __builtin_memcpy(q, &v[0], 64);
    } else if constexpr (ONE_ROW) {
#pragma unroll
        for (uint32_t e = 0; e < 16; ++e)
            if (e < n) run.row[s + e] = v[e];
    } else {
        uint32_t b = s / run.hns, r = s - b * run.hns;
#pragma unroll
        for (uint32_t e = 0; e < 16; ++e) {
            if (e < n) run.row[(size_t)b * run.bstep + r] = v[e];
            if (++r == run.hns) {
                r = 0;
                ++b;
            }
        }
    }
}

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

// k_iir on the planar matrix: the two steps change places -- a channel's samples lie side by side, the channels' rows ns samples
// apart, the blocks nch * ns.
template <int NC, bool SHARED>
__global__ __launch_bounds__(64) void k_iir_planar(int32_t* __restrict__ buf, uint32_t nch, uint32_t ns, IirCoef c, uint32_t nblocks) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    IirState<NC> f;
    f.clear();
    if (SHARED) {  // one filter object for all channels of the block, as in the harness
        if (t >= nblocks) return;
        for (uint32_t ch = 0; ch < nch; ++ch) iir_channel<4, NC>(reinterpret_cast<uint8_t*>(buf + ((size_t)t * nch + ch) * ns), 4, ns, c, f, true);
    } else {
        if (t / nch >= nblocks) return;
        iir_channel<4, NC>(reinterpret_cast<uint8_t*>(buf + (size_t)t * ns), 4, ns, c, f, true);
    }
}

// k_iir_carry on the planar matrix: the run is the channel's row in each of the call's nblocks blocks in turn, ns samples each.
// (It takes the block count, which k_iir_carry's arguments have no place for.)
template <int NC>
__global__ __launch_bounds__(64) void k_iir_planar_carry(int32_t* __restrict__ buf, uint32_t nch, uint32_t ns, uint32_t nblocks, IirCoef c,
                                                         IirCarry* __restrict__ state) {
    const uint32_t ch = blockIdx.x * 64u + threadIdx.x;
    if (ch >= nch) return;
    IirCarry& s = state[ch];
    IirState<NC> f;
    const bool started = s.started != 0;
    if (started) f.load(s.x, s.y);
    else f.clear();
    for (uint32_t b = 0; b < nblocks; ++b) {
        uint8_t* p = reinterpret_cast<uint8_t*>(buf + ((size_t)b * nch + ch) * ns);
        if (b == 0 && !started) iir_channel<4, NC, true>(p, 4, ns, c, f, true);
        else iir_channel<4, NC, false>(p, 4, ns, c, f, true);
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
//
// PLANAR (k_iir_pipe_planar, the same body): lane <-> channel (or block) as before, so a wave's access touches 64 rows; a
// producer's part and a writer's part are 64 contiguous bytes of one row (planar_load_set, planar_store_part).  block_bytes is
// one [nch][hns] block of the matrix; with CARRY the run of ns rows passes through ns / hns such blocks, and a set or part across
// a block boundary goes dword by dword.
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
    constexpr bool PLANAR = false;
#include "k_iir_pipe_body.hpp"
}

template <int NC, bool SHARED, bool CARRY>
__global__ __launch_bounds__(kIirThreads) void k_iir_pipe_planar(uint8_t* __restrict__ buf, uint32_t nch, uint32_t ns, uint64_t block_bytes, IirCoef c,
                                                                 uint32_t nblocks, uint32_t lanes_per_wg, IirCarry* __restrict__ state) {
    constexpr int BPS = 4;
    constexpr bool ALIGNED = true, PLANAR = true;
#include "k_iir_pipe_body.hpp"
}

}  // namespace rspt

#pragma clang fp contract(fast)
