// median.hip -- the rolling-window median stage in front of the packers.
//
// Restates rolling_window_median<double>(W) (lib_rspt/lib_stat/rolling_window_median.h) as one fresh object per channel of
// every block, insert((double)x[c][t]) for t = 0 ... ns - 1, (int32_t) of every return value stored in the native sample width.
// That class returns the true median of the last min(t + 1, W) samples, so
//     lo = max(0, t - W + 1),  m = t - lo + 1,  s = sorted(x[c][lo .. t])
//     y[c][t] = m odd ? s[m / 2] : (int32_t)(((int64_t)s[m / 2 - 1] + s[m / 2]) / 2)      (C division: toward zero)
// which is exact in integers: int32 values sort as their doubles do, the sum of two of them is exact in a double, the halving
// is exact, and the truncation of (int32_t) is C's.  No floating point is used.
//
// Two regimes, switched at kMedShortMax (W = 1 is a plain copy on the host side):
//   short (2 <= W <= kMedShortMax), k_med_short: lane <-> (channel, run of kMedRun consecutive outputs), channel fastest, as in
//             k_fir.  The lane keeps its window sorted in N statically indexed registers (N = the smallest of 4, 8, 16, 32 that
//             holds W).  The N - W free slots hold INT32_MIN / INT32_MAX pads placed so that the median of the real samples is
//             always at slots c = (N - 1) / 2 and c + 1, whatever the window's fill (med_step says how); every step deletes one
//             value and inserts one with a branch-free sweep, one compare/select and one v_med3_i32 per slot.  A run starts W - 1
//             rows early to fill its window; the next group of samples is in flight while the current one is swept.
//   generic (any W >= 2, used above kMedShortMax): rank every sample of a channel by (value, index) with a hand-written sort
//             (k_med_tile_sort: a bitonic sort of kMedTile keys in LDS, then k_med_merge passes that place every key of two
//             sorted runs by a binary search of the other run), then walk spans of kMedSpan outputs of the time axis with a
//             two-level bitmap over ranks in LDS (k_med_walk).  A span sets the bits of its W predecessors in parallel,
//             finds the lower median by a wave-wide count, and from then on moves the median pointer by at most one set bit
//             per output -- the reference's own "move the iterator" idea.  The values of the pointed-to ranks are looked up
//             64 outputs at a time, one per lane.
//
// In place (d_dst == d_src) is safe by construction.  Short: a workgroup owns a span of rows of a channel group and walks it
// chunk by chunk from the LAST to the first; a chunk reads rows below its own end only, stages its outputs in LDS, and writes
// them behind a barrier that follows every read of the chunk.  The W - 1 rows in front of a span, which another workgroup
// owns, are copied into the handle's halo buffer by k_fir_halo before k_med_short starts.  Generic: only k_med_tile_sort reads
// the samples, and it runs before k_med_walk, which writes them, on the same stream; no kernel reads what another writes in
// the same launch.
//
// Carried state (rspt_hip_median_filter_stream_dev): the blocks of a call lie back to back, so the call is ONE run of
// N = nblocks * ns rows, and the reference's object between two calls is its window: the last min(rows so far, W - 1) inputs of
// every channel.  The state is [u64 fill][W - 1 rows], the valid rows last and zeros in front of them.  k_med_carry copies it
// into the handle's `head` buffer and then writes the new state, the tail of (old state ++ call) and min(fill + N, W - 1), from
// the staged head and d_src -- both in front of every kernel that stores to d_dst (stream order).  The kernels lay the call out
// as if all W - 1 head rows were there and skip the first W - 1 - fill of them: a run of k_med_short starts at row
// max(-fill, t0 - (W - 1)); the generic path never sets their bits and never counts them.
//   Generic: (head ++ call) is cut per channel into segments of S = W - 1 + L rows (S <= kMedMaxRanks): the W - 1 rows in front
// of L new ones.  A segment is ranked on its own with segment-local indices (shorter last segments are padded with keys above
// every sample's) and walked for its own new rows only.  The (segment, channel) items are worked through in pieces from the
// LAST segment to the first: a walk writes only its segment's new rows, which no segment sorted later reads, so in place needs
// no saved overlap rows.
#include "common.hpp"

namespace rspt {

constexpr uint32_t kMedShortMax = 32;    // the regime switch: W up to this uses k_med_short, W above it the generic path
constexpr uint32_t kMedThreads = 256;
constexpr uint32_t kMedRun = 32;         // consecutive outputs per lane (k_med_short)
constexpr uint32_t kMedTile = 4096;      // keys of one LDS sort (k_med_tile_sort): 32 KiB
constexpr uint32_t kMedSpan = 1024;      // outputs of one walk (k_med_walk)
constexpr uint32_t kMedMaxRanks = 1u << 18;  // the longest channel of the generic path: its bitmaps take 4 (ns / 32 + ns / 1024) bytes of LDS
constexpr uint32_t kMedMaxCarry = 1u << 17;  // the longest carried window (W - 1) of the generic path: half a segment stays new

// The segments of a carried-state call of the generic path (head == null: the stateless call, one pair = one channel of a block).
struct MedSeg {
    const uint8_t* head;  // [u64 fill][W - 1 rows]: the staged old state
    uint32_t L;           // new rows of a segment (the last one may hold fewer)
    uint32_t nseg;        // segments per channel: ceil(N / L)
    uint32_t N;           // rows of the call
    uint32_t bns;         // the planar matrix only: samples of a block's row (row r of the call is sample r % bns of block r / bns)
};

// BPS inside the bodies of k_med_tile_sort / k_med_walk where they work on the planar int32 matrix [nblocks][nch][ns]
// (k_medp_tile_sort / k_medp_walk, median_planar.hip): the sample is a whole aligned word, and row r of a carried call's run of
// channel ch lies at med_planar_at.
constexpr int kMedPlanar = 0;
__device__ __forceinline__ uint64_t med_planar_at(const MedSeg& sg, uint32_t nch, uint32_t ch, uint32_t r) {
    return planar_run_at(r, nch, ch, sg.bns) * 4u;
}

// ---- short windows ----

// Sorted window s[0..N-1] of the real samples and the pads.  Delete value o (present), insert value v: the slots below the
// first one >= o keep their values, the others take their upper neighbour's (d), and then every slot i becomes
// med3(d[i - 1], v, d[i]) -- v lands where it sorts and the slots above it move up by one.  Equal values are interchangeable,
// so deleting "an" o is deleting the o.
template <uint32_t N>
__device__ __forceinline__ void med_replace(int32_t (&s)[N], int32_t o, int32_t v) {
    int32_t dprev = INT32_MIN;
#pragma unroll
    for (uint32_t i = 0; i < N; ++i) {
        const int32_t up = i + 1 < N ? s[i + 1] : INT32_MAX;
        const int32_t d = s[i] < o ? s[i] : up;
        s[i] = max(dprev, min(v, d));  // (= med3(dprev, v, d): dprev <= d)
        dprev = d;
    }
}

// One step of a lane's window for the sample v, with m real samples in it before (0 <= m <= W), `old` the sample W rows back
// (used once m == W).  With m reals, the window holds Lo(m) = c - floor((m - 1) / 2) INT32_MIN pads (Lo(0) = c) below them and
// INT32_MAX pads above, so the reals' lower median sits at slot c and their upper one at c + 1 (m even) or c (m odd).  Going from
// m to m + 1 reals removes an INT32_MIN pad when m is even and at least 2, an INT32_MAX pad otherwise; once the window is full
// the oldest sample goes.  Returns the median of the m' = min(m + 1, W) reals.
template <uint32_t N>
__device__ __forceinline__ int32_t med_step(int32_t (&s)[N], uint32_t m, uint32_t W, int32_t v, int32_t old) {
    constexpr uint32_t c = (N - 1) / 2;
    const int32_t o = m >= W ? old : ((m >= 2 && !(m & 1)) ? INT32_MIN : INT32_MAX);
    med_replace<N>(s, o, v);
    const uint32_t mm = m >= W ? W : m + 1;
    const int64_t sum = (int64_t)s[c] + (int64_t)((mm & 1) ? s[c] : s[c + 1]);
    return (int32_t)(sum / 2);
}

// One span of one channel group of one block per unit.  `halo` is null out of place; in place it holds, for span w >= 1 of
// block b, the W - 1 rows in front of the span at halo + ((b * (nsplit - 1) + w - 1) * (W - 1)) * stride (k_fir_halo's layout).
// HEAD: a carried-state call (one block); `head` is the staged state [u64 fill][W - 1 rows], and span 0's runs start up to `fill`
// rows in front of row 0 and read those rows there.
template <uint32_t N, int BPS, bool ALIGNED, bool HEAD = false>
__global__ __launch_bounds__(kMedThreads) void k_med_short(const uint8_t* src, uint8_t* dst, const uint8_t* halo, WinGeom g, const uint8_t* head) {
    constexpr uint32_t R = kMedRun, G = 8;
    __shared__ int32_t stage[R * kMedThreads];  // [r][tid]: the chunk's outputs until every read of the chunk is done
    const uint32_t tid = threadIdx.x;
    const uint32_t cl = tid % g.cw, sub = tid / g.cw;
    const uint32_t W = g.K;
    const uint32_t C = g.subs * R;
    const uint32_t stride = g.stride;
    const int32_t smin = HEAD ? -(int32_t)*reinterpret_cast<const uint64_t*>(head) : 0;  // the first row of the recording a window may hold
    for (uint64_t u = blockIdx.x; u < g.units; u += gridDim.x) {
        const uint32_t w = (uint32_t)(u % g.nsplit);
        const uint64_t rest = u / g.nsplit;
        const uint32_t cg = (uint32_t)(rest % g.ncg);
        const uint64_t b = rest / g.ncg;
        const uint32_t ch = cg * g.cw + cl;
        const bool live = sub < g.subs && ch < g.nch;
        const uint32_t chc = live ? ch : cg * g.cw;
        const uint64_t blk = b * g.block_bytes;
        const int32_t lo = (int32_t)(w * g.span);
        const int32_t hi = min((int32_t)g.ns, lo + (int32_t)g.span);
        const int32_t lim = (halo && w) ? lo : 0;  // rows below lim come from a staged copy: the halo, or (rows below 0) the head
        const uintptr_t srow0 = reinterpret_cast<uintptr_t>(src + blk) + chc * BPS;
        const uintptr_t hrow0 = lim ? reinterpret_cast<uintptr_t>(halo) + ((b * (g.nsplit - 1) + w - 1) * (uint64_t)(W - 1)) * stride + chc * BPS -
                                          (uint64_t)(lo - (int32_t)(W - 1)) * stride
                                : HEAD ? reinterpret_cast<uintptr_t>(head) + 8 + (uint64_t)(W - 1) * stride + chc * BPS
                                       : srow0;
        auto ld = [&](int32_t s) {
            const uintptr_t base = s < lim ? hrow0 : srow0;
            return sample_load<BPS>(reinterpret_cast<const uint8_t*>(base + (uint64_t)(int64_t)s * stride), ALIGNED);
        };
        const uint32_t nq = ((uint32_t)(hi - lo) + C - 1) / C;
        for (uint32_t q = nq; q-- > 0;) {
            const int32_t a = lo + (int32_t)(q * C);
            const int32_t t0 = a + (int32_t)(sub * R);
            const int32_t e = live ? min(t0 + (int32_t)R, hi) : t0;          // outputs [t0, e): none for dead lanes and runs past the span
            const int32_t s0 = e > t0 ? max(smin, t0 - (int32_t)(W - 1)) : e;  // the run's window starts filling here (no rows read if e <= t0)
            int32_t s[N];
#pragma unroll
            for (uint32_t i = 0; i < N; ++i) s[i] = i < (N - 1) / 2 ? INT32_MIN : INT32_MAX;  // m = 0: Lo(0) = c
            // samples of group t .. t + G - 1: the new one (row t + j) and the one W rows back, both clamped into [s0, e) -- every row
            // read lies in the run's own range; a clamped value is never used (past e: no step; below s0: the window is not full)
            int32_t vn[G], vo[G];
            if (s0 < e) {
#pragma unroll
                for (uint32_t j = 0; j < G; ++j) {
                    vn[j] = ld(min(s0 + (int32_t)j, e - 1));
                    vo[j] = ld(min(max(s0 + (int32_t)j - (int32_t)W, s0), e - 1));
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
                        vn[j] = ld(min(t + (int32_t)(G + j), e - 1));
                        vo[j] = ld(min(max(t + (int32_t)(G + j) - (int32_t)W, s0), e - 1));
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < G; ++j) {
                    const int32_t tj = t + (int32_t)j;
                    if (tj < e) {
                        const uint32_t m = min((uint32_t)(tj - s0), W);
                        const int32_t y = med_step<N>(s, m, W, cn[j], co[j]);
                        if (tj >= t0) stage[(uint32_t)(tj - t0) * kMedThreads + tid] = y;
                    }
                }
            }
            __syncthreads();  // every lane of the workgroup has read the chunk's rows before any of them is overwritten
            if (live) {
                uint8_t* out = dst + blk + chc * BPS;
                for (int32_t t = t0; t < e; ++t)
                    sample_store<BPS>(out + (uint64_t)(uint32_t)t * stride, stage[(uint32_t)(t - t0) * kMedThreads + tid], ALIGNED);
            }
            __syncthreads();  // (the stage is refilled by the next chunk)
        }
    }
}

// ---- generic path: ranks ----

// key of sample x at index t of its channel: (x, t) in lexicographic order, unique within the channel
__device__ __forceinline__ uint64_t med_key(int32_t x, uint32_t t) { return ((uint64_t)((uint32_t)x ^ 0x80000000u) << 32) | t; }
__device__ __forceinline__ int32_t med_key_value(uint64_t k) { return (int32_t)((uint32_t)(k >> 32) ^ 0x80000000u); }

// Pair p = (block, channel) of the piece [pair0, pair0 + npairs): keys[p][0 .. ns) sorted in runs of kMedTile.  With
// `rank` (ns <= kMedTile: the sort is complete), also rank[p][t] = position of sample t.
// STREAM: pair = (segment counted from the last, channel), g.ns = the segment capacity S; index t of the segment is row
// j L - (W - 1) + t of the call, a row of the staged head where that is negative, and a pad (above every sample, unique) from the
// segment's own length on.  The body is a file of its own: k_medp_tile_sort (median_planar.hip) includes it with BPS = kMedPlanar,
// where the rows of the call lie in the planar matrix (med_planar_at) and the head's where they always do.
template <int BPS, bool ALIGNED, bool STREAM = false>
__global__ __launch_bounds__(kMedThreads) void k_med_tile_sort(const uint8_t* src, uint64_t* keys, uint32_t* rank, WinGeom g, uint64_t pair0, MedSeg sg) {
#include "k_med_tile_sort_body.hpp"
}

// One merge pass: runs of `width` sorted keys become runs of 2 width.  Every key finds its place by a binary search of the
// other run of its pair (keys are unique).  With `rank` (the last pass), also rank[p][t] = position of sample t.
__global__ __launch_bounds__(kMedThreads) void k_med_merge(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint32_t* rank, uint32_t ns,
                                                           uint32_t width, uint64_t total) {
    const uint64_t gi = (uint64_t)blockIdx.x * kMedThreads + threadIdx.x;
    if (gi >= total) return;
    const uint64_t p = gi / ns;
    const uint32_t i = (uint32_t)(gi % ns);
    const uint64_t* kp = in + p * ns;
    const uint64_t key = kp[i];
    const uint32_t r = i / width, j = i - r * width;
    const uint32_t other = (r ^ 1u) * width;  // (below 2^32: ns < 2^31)
    uint32_t lo = 0, n = other < ns ? min(width, ns - other) : 0;
    const uint64_t* o = kp + other;
    while (n > 0) {  // lo = number of keys of the other run below `key`
        const uint32_t h = n / 2;
        if (o[lo + h] < key) {
            lo += h + 1;
            n -= h + 1;
        } else {
            n = h;
        }
    }
    const uint32_t pos = (r & ~1u) * width + j + lo;
    out[p * ns + pos] = key;
    if (rank) rank[p * ns + (uint32_t)key] = pos;
}

// ---- generic path: the walk ----

// Two-level bitmap over the ranks of one channel in LDS: b0 one bit per rank, b1 one bit per non-empty word of b0.  Written by
// lane 0 (atomics: no return needed), read by every lane (one address: a broadcast).  LDS operations of a wave complete in order.
struct MedBits {
    uint32_t* b0;
    uint32_t* b1;
    uint32_t n1;  // words of b1
    __device__ void set(uint32_t r, bool writer) const {
        if (writer) {
            atomicOr(&b0[r >> 5], 1u << (r & 31));
            atomicOr(&b1[r >> 10], 1u << ((r >> 5) & 31));
        }
    }
    __device__ void clear(uint32_t r, bool writer) const {
        if (writer) {
            const uint32_t old = atomicAnd(&b0[r >> 5], ~(1u << (r & 31)));
            if ((old & ~(1u << (r & 31))) == 0) atomicAnd(&b1[r >> 10], ~(1u << ((r >> 5) & 31)));
        }
    }
    // smallest set rank above r, or ~0u
    __device__ uint32_t next(uint32_t r) const {
        const uint32_t w = r >> 5;
        const uint32_t bits = b0[w] & (0xFFFFFFFEu << (r & 31));
        if (bits) return (w << 5) | (uint32_t)__builtin_ctz(bits);
        uint32_t u = w + 1, u1 = u >> 5;
        if (u1 >= n1) return ~0u;
        uint32_t m = (u & 31) ? (b1[u1] & (0xFFFFFFFFu << (u & 31))) : b1[u1];
        while (!m) {
            if (++u1 >= n1) return ~0u;
            m = b1[u1];
        }
        const uint32_t wd = (u1 << 5) | (uint32_t)__builtin_ctz(m);
        return (wd << 5) | (uint32_t)__builtin_ctz(b0[wd]);
    }
    // largest set rank below r, or ~0u
    __device__ uint32_t prev(uint32_t r) const {
        const uint32_t w = r >> 5;
        const uint32_t bits = b0[w] & ((1u << (r & 31)) - 1u);
        if (bits) return (w << 5) | (31u - (uint32_t)__builtin_clz(bits));
        if (w == 0) return ~0u;
        const uint32_t u = w - 1;
        int32_t u1 = (int32_t)(u >> 5);
        uint32_t m = b1[u1] & (0xFFFFFFFFu >> (31 - (u & 31)));
        while (!m) {
            if (--u1 < 0) return ~0u;
            m = b1[u1];
        }
        const uint32_t wd = ((uint32_t)u1 << 5) | (31u - (uint32_t)__builtin_clz(m));
        return (wd << 5) | (31u - (uint32_t)__builtin_clz(b0[wd]));
    }
};

// One wave per (pair of the piece, span of kMedSpan outputs).  keys: the piece's sorted keys, rank: their inverse.  The state
// (p = rank of the lower median, below = window members with a smaller rank) is computed alike by every lane.
// STREAM: pair and g.ns as in k_med_tile_sort; the spans cover the segment's new rows only (indices W - 1 .. n - 1), and `v0` is
// the first index that holds a row of the recording: W - 1 - fill in the first segment, 0 in every other.
// The body is a file of its own: k_medp_walk (median_planar.hip) includes it with BPS = kMedPlanar and stores the segment's new
// rows into the planar matrix (med_planar_at).
template <int BPS, bool ALIGNED, bool STREAM = false>
__global__ __launch_bounds__(64) void k_med_walk(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rank, uint8_t* dst, WinGeom g,
                                                 uint64_t pair0, MedSeg sg) {
#include "k_med_walk_body.hpp"
}

// ---- carried state ----

// The two movers of a carried-state call, in units of T (bytes, or 32-bit words where everything is a multiple of 4): n = the
// state's W - 1 rows, call = the call's N rows.  `state` and `head` are [u64 fill][rows].
//   SAVE = false   head <- state
//   SAVE = true    state rows <- the last W - 1 rows of (head rows ++ call): the call's last W - 1 rows, or, where the call is
//                  shorter than that, the head's rows from N on and then the whole call (the valid rows stay last, the zeros in
//                  front); fill <- min(fill + N, W - 1)
// SAVE = true runs behind SAVE = false and in front of every kernel that writes d_dst (stream order): the state is never read
// while it is written, and d_src is still the input.
template <bool SAVE, class T>
__global__ __launch_bounds__(256) void k_med_carry(const T* __restrict__ src, uint8_t* head, uint8_t* state, uint64_t n, uint64_t call, uint64_t wm1,
                                                   uint64_t N) {
    const uint64_t i0 = (uint64_t)blockIdx.x * 256u + threadIdx.x, step = (uint64_t)gridDim.x * 256u;
    T* hrows = reinterpret_cast<T*>(head + 8);
    T* srows = reinterpret_cast<T*>(state + 8);
    if (!SAVE) {
        for (uint64_t i = i0; i < n; i += step) hrows[i] = srows[i];
        if (i0 == 0) *reinterpret_cast<uint64_t*>(head) = *reinterpret_cast<const uint64_t*>(state);
    } else {
        for (uint64_t i = i0; i < n; i += step) srows[i] = call >= n ? src[call - n + i] : i + call < n ? hrows[i + call] : src[i + call - n];
        if (i0 == 0) *reinterpret_cast<uint64_t*>(state) = min(*reinterpret_cast<const uint64_t*>(head) + N, wm1);
    }
}

}  // namespace rspt
