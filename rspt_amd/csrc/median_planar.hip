// median_planar.hip -- the rolling-window median on the planar int32 matrix [nblocks][nch][ns] ("planar form").
//
// The arithmetic is median.hip's: med_step / med_replace on the four register buckets for 2 <= W <= kMedShortMax, ranks and the
// bitmap walk above it.  What differs is where a window lies: W consecutive samples of a channel are W consecutive WORDS of one
// row of the matrix, so the lanes of the short kernel run along the row (as in k_fir_planar):
//   lane <-> (row, run of kMedRun consecutive outputs), consecutive lanes on consecutive runs; a row shorter than a chunk of
//             kMedThreads * kMedRun outputs takes the smallest power of two of lanes that covers it (at least kMedpMinLanes) and
//             the workgroup takes kMedThreads / lanes rows side by side.
//   a chunk's samples -- its own and the W - 1 in front of it -- are brought into LDS by the row's lanes together (a wave's load
//             is contiguous; dwordx4 where src, dst and the rows are 16-byte aligned, dword otherwise), each lane sweeps its run
//             out of LDS (a run starts W - 1 samples early to fill its window, as in k_med_short; both the incoming sample and the
//             one W back are read there), stages its outputs in LDS, and the row's lanes store the chunk together.  Word i of
//             either buffer lies at i + i / 32: lanes 32 words apart hit 33 banks apart, so neither the sweep's reads and writes
//             nor the wide ones pile up on a bank.
// A row = (block, channel) is b * nch + c; a workgroup owns one span of samples of each of its rows and walks it from its LAST
// chunk to its first.  A chunk's stores follow a barrier that follows every global read of the chunk, they go to the chunk's own
// samples only, and what a workgroup reads outside its span is a `front`: the W - 1 samples in front of a span, staged by
// k_firp_front BEFORE this kernel (stream order).  So in place is safe by construction.  Stateless, spans 1.. of an in-place
// call have a front (out of place they read d_src itself) and span 0 has none: its window expands from m = 0.  A carried call
// adds the front of span 0 of EVERY row: the channel's samples in the blocks before this one and, behind the call's first
// block, the staged state.  A fresh state's rows are absent, not repeated: a run starts at max(-fill, t0 - (W - 1)) in the
// recording's coordinates, where fill is read from the staged state on the device, and never touches what lies in front of it.
//
// Generic path (W > kMedShortMax).  Stateless, a row of the matrix IS a block of one channel of 4-byte samples, so the native
// kernels k_med_tile_sort<4>, k_med_merge and k_med_walk<4> run on it as they are, on the geometry (nblocks * nch blocks, 1
// channel).  Carried, (head ++ call) of channel c is cut into the same segments (MedSeg, median_segment_rows), and
// k_medp_tile_sort / k_medp_walk -- the bodies of k_med_tile_sort / k_med_walk, included with BPS = kMedPlanar -- find row r of
// the call at sample r % ns of block r / ns (med_planar_at).  They are kernels of their own, not further instantiations, so
// that the native ones stay the set they were.  The in-place argument of DESIGN 4d holds per channel and per time index, so it
// carries over: only the sort reads samples, a walk writes only its segment's new rows, and the segments go from the LAST to the
// first, so no segment sorted later reads a row that a walk has written.
//
// Carry.  The state is the native one at bps = 4: [u64 fill][W - 1 rows of nch int32], valid rows last.  k_med_carry<false>
// stages it as it is; k_medp_save gathers the new rows from the tails of the blocks' row c (and the staged head where the call
// is shorter than W - 1) with k_firp_save's loop.  Both precede every store to d_dst.
#include "common.hpp"

namespace rspt {

constexpr uint32_t kMedpMinLanes = 8;  // lanes of the shortest rows: bounds the rows, and so the fronts, of a workgroup's LDS
constexpr uint32_t kMedpFront = 32;    // words kept in front of a chunk in LDS (>= kMedShortMax - 1, and a multiple of 32 and of 4)
// LDS words of the two buffers: kMedThreads / lanes rows of (front + lanes * kMedRun) samples in, kMedThreads * kMedRun out, each
// with one pad word per 32 and room for the reads of the last group of a run, which no step uses
constexpr uint32_t kMedpInWords = (kMedThreads / kMedpMinLanes) * kMedpFront + kMedThreads * kMedRun;
constexpr uint32_t kMedpIn = kMedpInWords + kMedpInWords / 32 + 16;
constexpr uint32_t kMedpOut = kMedThreads * kMedRun + kMedThreads * kMedRun / 32;

__device__ __forceinline__ uint32_t medp_pad(uint32_t i) { return i + (i >> 5); }

// WIDE: src, dst and every row of them are 16-byte aligned (ns % 4 == 0), so a chunk is whole dwordx4s.  `head`: the staged state
// of a carried call (g.carried), read for its fill only.
template <uint32_t N, bool WIDE>
__global__ __launch_bounds__(kMedThreads) void k_med_planar(const int32_t* src, int32_t* dst, const int32_t* front, PlanarWin g, const uint8_t* head) {
    constexpr uint32_t R = kMedRun, G = 8, F = kMedpFront;
    __shared__ int32_t xin[kMedpIn];
    __shared__ int32_t xout[kMedpOut];
    const uint32_t tid = threadIdx.x;
    const uint32_t sub = tid & (g.lanes - 1u), rl = tid / g.lanes;
    const uint32_t W = g.K;
    const uint32_t C = g.lanes * R;         // outputs of a chunk
    const uint32_t in0 = rl * (C + F) + F;  // the row's word of the chunk's first sample in xin; the front lies below it
    const uint32_t out0 = rl * C;
    const uint64_t fill = g.carried ? *reinterpret_cast<const uint64_t*>(head) : 0;
    for (uint64_t u = blockIdx.x; u < g.units; u += gridDim.x) {
        const uint32_t w = (uint32_t)(u % g.nsplit);
        const uint64_t row0 = u / g.nsplit * g.rpw;
        const bool live = row0 + rl < g.rows;
        const uint64_t row = live ? row0 + rl : row0;
        const int32_t lo = (int32_t)(w * g.span);
        const int32_t hi = (int32_t)min((uint64_t)g.ns, (uint64_t)lo + g.span);
        // samples below `lim` come from the staged front; `start` is the first sample a window of this span may hold
        const bool staged = planar_staged(g, w);
        const int32_t lim = staged ? lo : 0;
        const int32_t start = w ? lo - (int32_t)(W - 1) : g.carried ? -(int32_t)min(fill + row / g.nch * g.ns, (uint64_t)(W - 1)) : 0;
        const int32_t* rowp = src + row * g.ns;
        const int32_t* piece = staged ? front + planar_piece(g, row, w) * (uint64_t)(W - 1) - (lo - (int32_t)(W - 1)) : rowp;  // (indexed by the sample)
        const uint32_t nq = ((uint32_t)(hi - lo) + C - 1) / C;
        for (uint32_t q = nq; q-- > 0;) {
            const int32_t a = lo + (int32_t)(q * C);
            const uint32_t n = (uint32_t)(min(a + (int32_t)C, hi) - a);  // samples of the chunk
            if (live) {
                for (uint32_t i = sub; i < W - 1; i += g.lanes) {
                    const int32_t s = a - (int32_t)(W - 1) + (int32_t)i;
                    if (s >= start) xin[medp_pad(in0 - (W - 1) + i)] = (s < lim ? piece : rowp)[s];
                }
                if (WIDE) {
                    for (uint32_t k = 4 * sub; k < n; k += 4 * g.lanes) {  // (n % 4 == 0: ns % 4 == 0 and a span is whole chunks)
                        const int4 v = *reinterpret_cast<const int4*>(rowp + a + k);
                        int32_t* x = xin + medp_pad(in0 + k);  // (the four words share a group of 32: one pad)
                        x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
                    }
                } else {
                    for (uint32_t k = sub; k < n; k += g.lanes) xin[medp_pad(in0 + k)] = rowp[a + k];
                }
            }
            __syncthreads();
            const int32_t t0 = a + (int32_t)(sub * R);
            const int32_t e = live ? min(t0 + (int32_t)R, hi) : t0;               // outputs [t0, e): none for dead rows and runs past the span
            const int32_t s0 = e > t0 ? max(start, t0 - (int32_t)(W - 1)) : e;  // the run's window starts filling here
            auto ld = [&](int32_t s) { return xin[medp_pad(in0 + (uint32_t)(s - a))]; };  // (s - a >= -(W - 1): the front's words)
            int32_t s[N];
#pragma unroll
            for (uint32_t i = 0; i < N; ++i) s[i] = i < (N - 1) / 2 ? INT32_MIN : INT32_MAX;  // m = 0: Lo(0) = c
            // samples of group t .. t + G - 1: the new one and the one W back, the latter clamped to the run's start (below it the
            // window is not full and the value is not used); past e the words read are another run's, and no step follows
            int32_t vn[G], vo[G];
            if (s0 < e) {
#pragma unroll
                for (uint32_t j = 0; j < G; ++j) {
                    vn[j] = ld(s0 + (int32_t)j);
                    vo[j] = ld(max(s0 + (int32_t)j - (int32_t)W, s0));
                }
            }
            for (int32_t t = s0; t < e; t += G) {
                int32_t cn[G], co[G];
#pragma unroll
                for (uint32_t j = 0; j < G; ++j) {
                    cn[j] = vn[j];
                    co[j] = vo[j];
                }
                if (t + (int32_t)G < e) {  // the next group in flight while this one is swept
#pragma unroll
                    for (uint32_t j = 0; j < G; ++j) {
                        vn[j] = ld(t + (int32_t)(G + j));
                        vo[j] = ld(max(t + (int32_t)(G + j) - (int32_t)W, s0));
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < G; ++j) {
                    const int32_t tj = t + (int32_t)j;
                    if (tj < e) {
                        const uint32_t m = min((uint32_t)(tj - s0), W);
                        const int32_t y = med_step<N>(s, m, W, cn[j], co[j]);
                        if (tj >= t0) xout[medp_pad(out0 + (uint32_t)(tj - a))] = y;
                    }
                }
            }
            __syncthreads();  // every global read of the chunk precedes this barrier, every store follows it
            if (live) {
                int32_t* out = dst + row * g.ns + a;
                if (WIDE) {
                    for (uint32_t k = 4 * sub; k < n; k += 4 * g.lanes) {
                        const int32_t* y = xout + medp_pad(out0 + k);
                        *reinterpret_cast<int4*>(out + k) = make_int4(y[0], y[1], y[2], y[3]);
                    }
                } else {
                    for (uint32_t k = sub; k < n; k += g.lanes) out[k] = xout[medp_pad(out0 + k)];
                }
            }
            // (the next chunk refills xin, which no lane reads behind the barrier above, and writes xout behind its own first barrier)
        }
    }
}

// The carried generic path on the matrix: k_med_tile_sort<.., STREAM = true> and k_med_walk<.., STREAM = true> with the planar way
// to a row of the call.
__global__ __launch_bounds__(kMedThreads) void k_medp_tile_sort(const uint8_t* src, uint64_t* keys, uint32_t* rank, WinGeom g, uint64_t pair0, MedSeg sg) {
    constexpr int BPS = kMedPlanar;
    constexpr bool ALIGNED = true, STREAM = true;
#include "k_med_tile_sort_body.hpp"
}

__global__ __launch_bounds__(64) void k_medp_walk(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rank, uint8_t* dst, WinGeom g,
                                                  uint64_t pair0, MedSeg sg) {
    constexpr int BPS = kMedPlanar;
    constexpr bool ALIGNED = true, STREAM = true;
#include "k_med_walk_body.hpp"
}

// state <- the last W - 1 rows of (head rows ++ the call's run of N = nblocks * ns samples per channel), gathered from the
// matrix by the FIR's loop (planar_save_rows, fir_planar.hip); fill <- min(fill + N, W - 1).  The valid rows stay last and the
// zeros in front: what k_med_carry<true> writes for a native call.
__global__ __launch_bounds__(256) void k_medp_save(const int32_t* __restrict__ src, const uint8_t* __restrict__ head, uint8_t* __restrict__ state,
                                                   uint64_t n, uint32_t nch, uint32_t ns, uint64_t wm1, uint64_t N) {
    planar_save_rows(src, reinterpret_cast<const int32_t*>(head + 8), reinterpret_cast<int32_t*>(state + 8), n, nch, ns, wm1, N);
    if ((uint64_t)blockIdx.x * 256u + threadIdx.x == 0) *reinterpret_cast<uint64_t*>(state) = min(*reinterpret_cast<const uint64_t*>(head) + N, wm1);
}

}  // namespace rspt
