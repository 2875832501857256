// fir.hip -- the FIR pre-filter stage in front of the packers.
//
// Restates i_filter::new_fir / init_history_values / filter_opt (lib_rspt/lib_filter/fir_filter.cpp) as the reference's test
// harness drives a filter (lib_rspt_test/rspt_test.cpp:116-136): init_history_values(first sample of the channel), then
// filter_opt on every sample, the double result truncated to int32 and written back in the native sample width.  For a
// kernel k[0..K-1] that is
//     y[c][t] = ((((0.0 + x[c][t-K+1]*k[0]) + x[c][t-K+2]*k[1]) + ...) + x[c][t]*k[K-1]),   x[c][s < 0] = x[c][0]
// with every product and every sum rounded on its own, in ascending tap order.  Unlike the IIR stage there is no state that
// runs from channel to channel: init_history_values replaces the whole window (filter() pushes into a ring that is not yet
// full, or calls filter_opt, K times), so one filter shared by all channels and one filter per channel give the same block.
//
// Every output depends on inputs only, so all of them are computed in parallel:
//   lane <-> (channel, run of kFirR consecutive outputs): channel fastest, so that a wave's load of one row offset is a
//             contiguous row segment of the interleaved block where the block is wide, and the lanes of a narrow block
//             (1-3 channels) spread over the time axis;
//   kFirR independent accumulators per lane: one loaded sample serves kFirR taps, and the kFirR dependent chains overlap;
//   coefficients: wave-uniform addresses, scalar loads (s_load), fed to v_mul_f64 as an SGPR operand;
//   the tap loop runs in groups of kFirR taps over a register window of 2 kFirR samples, the next group's samples in flight
//             while this one is multiplied: any K, ascending order kept across the groups.
// Per tap and output the work is one v_mul_f64 and one v_add_f64 -- what bounds the stage at all but the smallest K.
//
// In place (d_dst == d_src) is safe by construction, not by launch order: a workgroup owns a span of rows [lo, hi) of a
// channel group and walks it in chunks from the LAST to the first -- a chunk reads rows below its own first one, which no
// earlier-processed chunk has written, and writes its own rows behind a barrier that follows all of its reads.  The only
// rows a workgroup reads but does not own are the K - 1 in front of its span; k_fir_halo copies them into a side buffer
// owned by the handle BEFORE the filter kernel starts (stream order), and the filter reads them there.
//
// Carried state (rspt_hip_fir_prefilter_stream_dev): the blocks of a call lie back to back, so the call is ONE block of
// nblocks * ns rows, and the reference's object between two calls is its ring: the last K - 1 inputs of every channel.  The
// K - 1 rows in front of the call's row 0 are one more piece (`head`), staged from the state -- or, on a fresh state, the
// call's first row K - 1 times, which is what init_history_values leaves -- by k_fir_carry BEFORE anything is overwritten; a
// second k_fir_carry launch then writes the new state, the last K - 1 rows of (head ++ call), from the staged head and d_src.
// Stream order puts both in front of k_fir, so neither an in-place call nor K - 1 > nblocks * ns needs anything else.
#include "common.hpp"

// NO contraction in this file: every product and sum rounded on its own, as in the reference's x86-64 build (filter.hip says
// why __dmul_rn / __dadd_rn do not do that in HIP).  No f64 MFMA either: its internal rounding is not the reference's.
#pragma clang fp contract(off)

namespace rspt {

constexpr uint32_t kFirR = 16;          // consecutive outputs per lane (independent accumulators)
constexpr uint32_t kFirThreads = 256;
constexpr uint32_t kFirMaxTaps = 65536;

// The K taps of R consecutive outputs of one lane, ld(m) = window element m (the sample of row sb + m, see k_fir).  Tap i of
// output r reads element r + i + skip, where skip = G R - K virtual taps in front of the first group make every group R wide.
// Group g multiplies the window elements [g R, g R + 2 R) -- held in two halves lo, hi -- while the loads of the half after
// them are in flight; the halves then trade places (no register moves).  Elements up to (G + 2) R - 1 are loaded.
template <uint32_t R, class Ld>
__device__ __forceinline__ void fir_taps(double (&acc)[R], const double* __restrict__ coef, uint32_t K, Ld&& ld) {
    const uint32_t G = (K + R - 1) / R;
    const uint32_t skip = G * R - K;
    double A[R], B[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) acc[r] = 0.0;  // the reference's y = 0 (its first sum is 0.0 + product)
#pragma unroll
    for (uint32_t m = 0; m < R; ++m) A[m] = m >= skip ? (double)ld(m) : 0.0;  // (rows of virtual taps only are not read)
#pragma unroll
    for (uint32_t m = 0; m < R; ++m) B[m] = (double)ld(R + m);
    auto group = [&](double(&lo)[R], double(&hi)[R], uint32_t gi, auto first) {
        int32_t nx[R];  // (loaded after the last group too, unused: one branch less per group)
#pragma unroll
        for (uint32_t m = 0; m < R; ++m) nx[m] = ld((gi + 2) * R + m);
        const double* kg = coef + (int32_t)(gi * R) - (int32_t)skip;  // kg[d] = k of virtual tap gi R + d
#pragma unroll
        for (uint32_t d = 0; d < R; ++d) {
            if (decltype(first)::value && d < skip) continue;
            const double kk = kg[d];
#pragma unroll
            for (uint32_t r = 0; r < R; ++r) acc[r] = acc[r] + (r + d < R ? lo[r + d] : hi[r + d - R]) * kk;
        }
#pragma unroll
        for (uint32_t m = 0; m < R; ++m) lo[m] = (double)nx[m];  // the upper half of group gi + 1
    };
    group(A, B, 0, std::true_type());
    uint32_t gi = 1;
    for (; gi + 1 < G; gi += 2) {
        group(B, A, gi, std::false_type());
        group(A, B, gi + 1, std::false_type());
    }
    if (gi < G) group(B, A, gi, std::false_type());
}

// One span of one channel group of one block per unit.  `halo` is null out of place; in place it holds, for span w >= 1 of
// block b, the K - 1 rows in front of the span at halo + ((b * (nsplit - 1) + w - 1) * (K - 1)) * stride, each a copy of the
// block's row with the same layout.  `head` is null without a carried state; else it holds the K - 1 rows in front of row 0
// of block b at head + b * (K - 1) * stride (rows -(K - 1) .. -1 of the recording), and span 0 reads them in place of x[0].
template <int BPS, bool ALIGNED>
__global__ __launch_bounds__(kFirThreads) void k_fir(const uint8_t* src, uint8_t* dst, const uint8_t* halo, const double* __restrict__ coef,
                                                    WinGeom g, const uint8_t* head) {
    constexpr uint32_t R = kFirR;
    const uint32_t tid = threadIdx.x;
    const uint32_t cl = tid % g.cw, sub = tid / g.cw;
    const uint32_t K = g.K;
    const uint32_t G = (K + R - 1) / R;  // tap groups (fir_taps)
    const uint32_t C = g.subs * R;       // rows of a chunk
    const int32_t ns1 = (int32_t)g.ns - 1;
    const uint32_t stride = g.stride;
    for (uint64_t u = blockIdx.x; u < g.units; u += gridDim.x) {
        const uint32_t w = (uint32_t)(u % g.nsplit);
        const uint64_t rest = u / g.nsplit;
        const uint32_t cg = (uint32_t)(rest % g.ncg);
        const uint64_t b = rest / g.ncg;
        const uint32_t ch = cg * g.cw + cl;
        const bool live = sub < g.subs && ch < g.nch;
        // lanes past the shape read what lane 0 of their wave's channel group reads and store nothing
        const uint32_t chc = ch < g.nch ? ch : cg * g.cw, subc = sub < g.subs ? sub : 0u;
        const uint32_t lane_off = subc * R * stride + chc * BPS;  // (below 2^31: the host checks)
        const uint64_t blk = b * g.block_bytes;
        const int32_t lo = (int32_t)(w * g.span);
        const int32_t hi = (int32_t)min((uint64_t)g.ns, (uint64_t)lo + g.span);
        // rows below `lim` come from a staged copy: the halo (in place, every span but the first) or the head (carried state,
        // span 0: rows below 0, down to `smin`)
        const uint8_t* piece = w ? (halo ? halo + ((b * (g.nsplit - 1) + w - 1) * (uint64_t)(K - 1)) * stride : nullptr)
                                 : (head ? head + (b * (uint64_t)(K - 1)) * stride : nullptr);
        const int32_t lim = piece ? lo : 0;
        const int32_t smin = (head && !w) ? -(int32_t)(K - 1) : 0;
        // address of row 0 of the lane's channel in the block, and where row 0 would be in the staged copy (only rows >= lo - K + 1
        // are ever read there)
        const uintptr_t srow0 = reinterpret_cast<uintptr_t>(src + blk) + chc * BPS;
        const uintptr_t hrow0 = piece ? reinterpret_cast<uintptr_t>(piece) + chc * BPS - (uint64_t)(int64_t)(lo - (int32_t)(K - 1)) * stride : srow0;
        const uint32_t nq = ((uint32_t)(hi - lo) + C - 1) / C;
        for (uint32_t q = nq; q-- > 0;) {
            const int32_t a = lo + (int32_t)(q * C);
            // window element m of this lane is row sb + m (fir_taps)
            const int32_t first = a - (int32_t)(G * R - 1);  // row of element 0 of the chunk's first lane
            const int32_t sb = first + (int32_t)(subc * R);
            // wave-uniform: every row the chunk touches (up to a + C + R) lies in [lim, ns) -- one address add per load, no clamps
            const bool fast = first >= lim && a <= ns1 - (int32_t)(C + R);
            double acc[R];
            if (fast) {
                const uint8_t* rowbase = src + blk + (uint64_t)(uint32_t)first * stride;
                fir_taps<R>(acc, coef, K, [&](uint32_t m) { return sample_load<BPS>(rowbase + (uint64_t)m * stride + lane_off, ALIGNED); });
            } else {
                fir_taps<R>(acc, coef, K, [&](uint32_t m) {
                    const int32_t s = min(max(sb + (int32_t)m, smin), ns1);  // x[s < 0] = x[0] without a head; rows past the block are never used
                    const uintptr_t base = s < lim ? hrow0 : srow0;
                    return sample_load<BPS>(reinterpret_cast<const uint8_t*>(base + (uint64_t)(int64_t)s * stride), ALIGNED);
                });
            }
            __syncthreads();  // every lane of the workgroup has read the chunk's rows before any of them is overwritten
            if (live) {
                uint8_t* out = dst + blk + (uint64_t)(uint32_t)a * stride + lane_off;
                const int32_t t0 = a + (int32_t)(subc * R);
#pragma unroll
                for (uint32_t r = 0; r < R; ++r)
                    if (t0 + (int32_t)r < hi) sample_store<BPS>(out + r * stride, trunc_i32_c(acc[r]), ALIGNED);  // (x86-64's (int32_t): common.hpp)
            }
        }
    }
}

// In place: copy the K - 1 rows in front of every span but the first (rows [w * span - K + 1, w * span), all inside the block
// because span >= K - 1) into the handle's side buffer, one piece after the other.
template <bool WORDS>
__global__ __launch_bounds__(256) void k_fir_halo(const uint8_t* __restrict__ src, uint8_t* __restrict__ halo, WinGeom g, uint64_t pieces) {
    const uint64_t n = (uint64_t)(g.K - 1) * g.stride;  // bytes of a piece
    for (uint64_t pc = blockIdx.x; pc < pieces; pc += gridDim.x) {
        const uint64_t b = pc / (g.nsplit - 1);
        const uint32_t w = (uint32_t)(pc % (g.nsplit - 1)) + 1u;
        const uint8_t* s = src + b * g.block_bytes + ((uint64_t)w * g.span - (g.K - 1)) * g.stride;
        uint8_t* d = halo + pc * n;
        if (WORDS) {
            for (uint64_t i = threadIdx.x; i < n / 4; i += 256)
                reinterpret_cast<uint32_t*>(d)[i] = reinterpret_cast<const uint32_t*>(s)[i];
        } else {
            for (uint64_t i = threadIdx.x; i < n; i += 256) d[i] = s[i];
        }
    }
}

// The two byte movers of a carried-state call, n = (K - 1) * stride bytes each (rows of the block's layout), N = the call's rows:
//   SAVE = false   head <- the state's rows if it has started, else the call's row 0 in every row (init_history_values)
//   SAVE = true    state <- the last K - 1 rows of (head ++ call): the call's last K - 1 rows, or, where the call is shorter
//                  than that, the head's rows from N on and then the whole call; and the state has started
// `started` is the state's first word, `rows` follow it.  SAVE = true runs behind SAVE = false and in front of k_fir (stream
// order), so the state is never read while it is written and d_src is still the input.
template <bool SAVE>
__global__ __launch_bounds__(256) void k_fir_carry(const uint8_t* __restrict__ src, uint8_t* head, uint64_t* started, uint8_t* rows, uint64_t n,
                                                   uint32_t stride, uint32_t K, uint32_t N) {
    const uint64_t i0 = (uint64_t)blockIdx.x * 256u + threadIdx.x, step = (uint64_t)gridDim.x * 256u;
    if (!SAVE) {
        const bool st = *started != 0;
        for (uint64_t i = i0; i < n; i += step) head[i] = st ? rows[i] : src[i % stride];
    } else {
        const uint64_t call = (uint64_t)N * stride;
        for (uint64_t i = i0; i < n; i += step) rows[i] = call >= n ? src[call - n + i] : i + call < n ? head[i + call] : src[i + call - n];
        if (i0 == 0) *started = 1;
    }
}

}  // namespace rspt

#pragma clang fp contract(fast)
