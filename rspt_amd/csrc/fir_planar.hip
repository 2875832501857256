// fir_planar.hip -- the FIR pre-filter on the planar int32 matrix [nblocks][nch][ns] ("planar form").
//
// The arithmetic is fir.hip's: y[c][t] = ((((0.0 + x[c][t-K+1]*k[0]) + ...) + x[c][t]*k[K-1]), x[c][s < 0] = x[c][0], every
// product and sum rounded on its own, kFirR independent accumulators per lane, tap groups over a register window of two halves,
// wave-uniform coefficients.  What differs is where a window lies: K consecutive samples of a channel are K consecutive WORDS of
// one row of the matrix, so the lanes run along the row:
//   lane <-> (row, run of kFirR consecutive outputs), consecutive lanes on consecutive runs.  The kFirR window elements of a tap
//             group are 64 contiguous bytes of the lane; where the rows are 16-byte aligned they arrive as four
//             global_load_dwordx4, and the kFirR outputs leave as four global_store_dwordx4.  A wave's loads of one group are
//             4 KiB of one row.
//   a row shorter than a chunk of kFirThreads * kFirR outputs takes the smallest power of two of lanes that covers it, and the
//             workgroup takes kFirThreads / lanes rows side by side: 40-sample rows go 64 to a workgroup, no lane idles for
//             want of a row.
// A row = (block, channel) is b * nch + c; a workgroup owns one span of samples of each of its rows and walks it from its LAST
// chunk to its first, writing a chunk behind a barrier that follows every read of it (in place is safe by construction, as in
// k_fir).  What it reads but does not own is a `front`: the K - 1 samples in front of a span, staged by k_firp_front BEFORE the
// filter kernel (stream order).  Stateless, spans 1.. of an in-place call have one (out of place they read d_src itself, and
// span 0 reads x[0]).  A carried call adds the front of span 0 of EVERY row: the channel's samples in the blocks before this one
// and, behind the call's first block, the head -- the state's rows, or the run's first sample K - 1 times on a fresh state.
// The blocks of a carried call are NOT one contiguous row per channel (channel c's run is P[0][c][:], P[1][c][:], ...), which
// is why the front is gathered: a window near the start of block b reaches into block b - 1, several blocks back where
// K - 1 > ns, and into the head.
//
// Whether a tap group's loads need clamps is decided per WAVE (there is no barrier inside the taps): a wave whose whole reach
// lies inside [the first sample it may read from the row, the end of the matrix) takes the wide loads; reads past the END of a
// row or a span fetch values that no stored output uses (the rows behind it, or samples another workgroup is writing), so only
// the last few samples of the whole matrix ever force the clamped path from that side.
#include "common.hpp"

#pragma clang fp contract(off)  // (as fir.hip: no fused multiply-add, no f64 MFMA)

namespace rspt {

// Decomposition of a sliding-window stage on the planar matrix (the host's planar_win makes it, with win_geom's split rule);
// nothing in it is FIR's alone: the median's short path runs on it too.
struct PlanarWin {
    uint64_t rows;     // nblocks * nch rows of ns samples
    uint64_t total;    // rows * ns: samples of the matrix
    uint64_t units;    // row groups * nsplit: one workgroup's work each
    uint32_t nch, ns, K;
    uint32_t lanes;    // lanes along a row: a power of two <= the workgroup's threads; a chunk is lanes * run outputs
    uint32_t rpw;      // rows of a workgroup: threads / lanes
    uint32_t span;     // samples of a workgroup per row (a multiple of the chunk; >= 4 (K - 1) where nsplit > 1)
    uint32_t nsplit;   // spans per row
    uint32_t npiece;   // staged fronts per row: (in place: nsplit - 1) + (carried: 1)
    uint32_t in_place, carried;
};

// The front of span w of a row, if it has one: K - 1 samples at front + piece * (K - 1).
__device__ __forceinline__ bool planar_staged(const PlanarWin& g, uint32_t w) { return w ? g.in_place != 0 : g.carried != 0; }
__device__ __forceinline__ uint64_t planar_piece(const PlanarWin& g, uint64_t row, uint32_t w) { return row * g.npiece + (g.carried ? w : w - 1u); }

// fir_taps (fir.hip) with the window fetched a tap group at a time: fetch(j, v) sets v[m] = window element j R + m for the R
// elements of group j.  Tap i of output r reads element r + i + skip, skip = G R - K virtual taps in front of the first group;
// groups 0 .. G + 1 are fetched (the last one unused: one branch less per group).
template <uint32_t R, class Fetch>
__device__ __forceinline__ void fir_taps_grouped(double (&acc)[R], const double* __restrict__ coef, uint32_t K, Fetch&& fetch) {
    const uint32_t G = (K + R - 1) / R;
    const uint32_t skip = G * R - K;
    double A[R], B[R];
    int32_t nx[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) acc[r] = 0.0;  // the reference's y = 0 (its first sum is 0.0 + product)
    fetch(0u, nx);
#pragma unroll
    for (uint32_t m = 0; m < R; ++m) A[m] = (double)nx[m];  // (elements below skip are never multiplied)
    fetch(1u, nx);
#pragma unroll
    for (uint32_t m = 0; m < R; ++m) B[m] = (double)nx[m];
    auto group = [&](double(&lo)[R], double(&hi)[R], uint32_t gi, auto first) {
        fetch(gi + 2u, nx);
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

// WIDE: src, dst and every row of them are 16-byte aligned (ns % 4 == 0), so a lane's group is whole dwordx4s.
template <bool WIDE>
__global__ __launch_bounds__(kFirThreads) void k_fir_planar(const int32_t* src, int32_t* dst, const int32_t* front, const double* __restrict__ coef,
                                                           PlanarWin g) {
    constexpr uint32_t R = kFirR;
    static_assert(R == 16, "a tap group is four dwordx4");
    const uint32_t tid = threadIdx.x;
    const uint32_t sub = tid & (g.lanes - 1u), rl = tid / g.lanes;
    const uint32_t K = g.K;
    const uint32_t G = (K + R - 1) / R;
    const uint32_t C = g.lanes * R;  // outputs of a chunk
    const int32_t ns1 = (int32_t)g.ns - 1;
    // the first and the last run of this lane's wave along the row (a wave of a narrow shape holds whole rows)
    const uint32_t wsub_lo = g.lanes >= 64u ? (tid & ~63u) & (g.lanes - 1u) : 0u;
    const uint32_t wsub_hi = g.lanes >= 64u ? wsub_lo + 63u : g.lanes - 1u;
    for (uint64_t u = blockIdx.x; u < g.units; u += gridDim.x) {
        const uint32_t w = (uint32_t)(u % g.nsplit);
        const uint64_t row0 = u / g.nsplit * g.rpw;  // (a row group's first row always exists)
        const bool live = row0 + rl < g.rows;
        const uint64_t row = live ? row0 + rl : row0;  // lanes past the last row read what row0's lanes read and store nothing
        const uint64_t row_last = min(row0 + g.rpw, g.rows) - 1u;
        const int32_t lo = (int32_t)(w * g.span);
        const int32_t hi = (int32_t)min((uint64_t)g.ns, (uint64_t)lo + g.span);
        // samples below `lim` come from the staged front, which begins at sample `smin`; without one x[s < 0] = x[0]
        const bool staged = planar_staged(g, w);
        const int32_t lim = staged ? lo : 0;
        const int32_t smin = staged ? lo - (int32_t)(K - 1) : 0;
        const int32_t* rowp = src + row * g.ns;
        const int32_t* piece = staged ? front + planar_piece(g, row, w) * (uint64_t)(K - 1) - smin : rowp;  // (indexed by the sample, as rowp)
        const uint32_t nq = ((uint32_t)(hi - lo) + C - 1) / C;
        for (uint32_t q = nq; q-- > 0;) {
            const int32_t a = lo + (int32_t)(q * C);
            const int32_t first = a - (int32_t)(G * R - 1);  // sample of window element 0 of the chunk's first lane
            const int32_t sb = first + (int32_t)(sub * R);   // ... of this lane: element m is sample sb + m
            // wave-uniform: the wave reads samples [first + wsub_lo R - 1, a + (wsub_hi + 2) R + 4) of its rows at most
            const bool fast = __builtin_amdgcn_readfirstlane(
                (int)(first + (int32_t)(wsub_lo * R) - 1 >= lim && row_last * g.ns + (uint64_t)(uint32_t)a + (wsub_hi + 2u) * R + 4u <= g.total));
            double acc[R];
            if (fast) {
                if (WIDE) {
                    // the aligned quads around the window: element m is word m + 1 of them
                    const int4* qp = reinterpret_cast<const int4*>(rowp + (sb - 1));
                    int4 c0 = qp[0];
                    fir_taps_grouped<R>(acc, coef, K, [&](uint32_t j, int32_t(&v)[R]) {
                        const int4* p = qp + 4u * j;
                        const int4 n1 = p[1], n2 = p[2], n3 = p[3], n4 = p[4];
                        v[0] = c0.y, v[1] = c0.z, v[2] = c0.w;
                        v[3] = n1.x, v[4] = n1.y, v[5] = n1.z, v[6] = n1.w;
                        v[7] = n2.x, v[8] = n2.y, v[9] = n2.z, v[10] = n2.w;
                        v[11] = n3.x, v[12] = n3.y, v[13] = n3.z, v[14] = n3.w;
                        v[15] = n4.x;
                        c0 = n4;
                    });
                } else {
                    const int32_t* wp = rowp + sb;
                    fir_taps_grouped<R>(acc, coef, K, [&](uint32_t j, int32_t(&v)[R]) {
#pragma unroll
                        for (uint32_t m = 0; m < R; ++m) v[m] = wp[j * R + m];
                    });
                }
            } else {
                fir_taps_grouped<R>(acc, coef, K, [&](uint32_t j, int32_t(&v)[R]) {
#pragma unroll
                    for (uint32_t m = 0; m < R; ++m) {
                        const int32_t s = min(max(sb + (int32_t)(j * R + m), smin), ns1);  // (samples past the row are never used)
                        v[m] = (s < lim ? piece : rowp)[s];
                    }
                });
            }
            __syncthreads();  // every lane of the workgroup has read the chunk's samples before any of them is overwritten
            if (live) {
                const int32_t t0 = a + (int32_t)(sub * R);
                int32_t* out = dst + row * g.ns + t0;
                if (WIDE && t0 + (int32_t)R <= hi) {
#pragma unroll
                    for (uint32_t r = 0; r < R; r += 4)
                        reinterpret_cast<int4*>(out)[r / 4] =
                            make_int4(trunc_i32_c(acc[r]), trunc_i32_c(acc[r + 1]), trunc_i32_c(acc[r + 2]), trunc_i32_c(acc[r + 3]));
                } else {
#pragma unroll
                    for (uint32_t r = 0; r < R; ++r)
                        if (t0 + (int32_t)r < hi) out[r] = trunc_i32_c(acc[r]);  // (x86-64's (int32_t): common.hpp)
                }
            }
        }
    }
}

// The movers of the planar form gather between the time-major state ([K - 1] rows of nch int32, oldest first, as the native
// state at bps = 4) and the channel-major matrix.  Their order on the stream: k_firp_head, k_firp_save, k_firp_front, then
// k_fir_planar -- so the state is never read while it is written, and everything is staged before d_dst is stored to.
//
// head <- the state's rows if it has started, else the run's first sample of every channel in every row (init_history_values).
__global__ __launch_bounds__(256) void k_firp_head(const int32_t* __restrict__ src, int32_t* __restrict__ head, const uint64_t* started,
                                                   const int32_t* __restrict__ rows, uint64_t n, uint32_t nch, uint32_t ns) {
    const bool st = *started != 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u)
        head[i] = st ? rows[i] : src[(i % nch) * ns];
}

// The gather of both stages' save movers (k_firp_save, k_medp_save): rows <- the last k1 rows of (head's k1 rows ++ the call's
// run of N = nblocks * ns samples per channel), n = k1 * nch samples, time-major.
__device__ __forceinline__ void planar_save_rows(const int32_t* __restrict__ src, const int32_t* __restrict__ head, int32_t* __restrict__ rows, uint64_t n,
                                                 uint32_t nch, uint32_t ns, uint64_t k1, uint64_t N) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint64_t j = i / nch, c = i % nch;
        const int64_t pos = (int64_t)N - (int64_t)k1 + (int64_t)j;  // sample of the run
        rows[i] = pos >= 0 ? src[planar_run_at((uint64_t)pos, nch, c, ns)] : head[(j + N) * nch + c];
    }
}

// state <- the last K - 1 rows of (head ++ the call's run of N samples per channel); and the state has started.
__global__ __launch_bounds__(256) void k_firp_save(const int32_t* __restrict__ src, const int32_t* __restrict__ head, uint64_t* started,
                                                   int32_t* __restrict__ rows, uint64_t n, uint32_t nch, uint32_t ns, uint32_t K, uint64_t N) {
    planar_save_rows(src, head, rows, n, nch, ns, K - 1, N);
    if ((uint64_t)blockIdx.x * 256u + threadIdx.x == 0) *started = 1;
}

// front <- the K - 1 samples in front of every span that has a staged front (planar_staged): samples of the row itself, or, in
// front of a carried call's span 0, of the same channel in the blocks before and of the head.
__global__ __launch_bounds__(256) void k_firp_front(const int32_t* __restrict__ src, const int32_t* __restrict__ head, int32_t* __restrict__ front,
                                                    PlanarWin g) {
    const uint64_t k1 = g.K - 1, n = g.rows * g.npiece * k1;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        const uint64_t j = i % k1, pc = i / k1;
        const uint64_t row = pc / g.npiece;
        const uint32_t w = (uint32_t)(pc % g.npiece) + (g.carried ? 0u : 1u);
        const int64_t s = (int64_t)w * g.span - (int64_t)k1 + (int64_t)j;  // sample of the row
        int32_t v;
        if (s >= 0) {
            v = src[row * g.ns + (uint64_t)s];
        } else {  // (span 0 of a carried call)
            const uint64_t b = row / g.nch, c = row % g.nch;
            const int64_t pos = (int64_t)(b * g.ns) + s;  // sample of the channel's run in this call
            v = pos >= 0 ? src[planar_run_at((uint64_t)pos, g.nch, c, g.ns)] : head[(uint64_t)((int64_t)k1 + pos) * g.nch + c];
        }
        front[i] = v;
    }
}

}  // namespace rspt

#pragma clang fp contract(fast)
