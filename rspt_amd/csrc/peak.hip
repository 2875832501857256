// peak.hip -- the R-peak detector stage and the Butterworth designer it is built on.
//
// Restates create_filter_iir (lib_rspt/lib_filter/iir_filter_design.cpp) on the host and three detectors of
// lib_rspt/peak_detector.h on the device: peak_detector::detect (ONLINE), peak_detector_1st_order::detect (ONLINE_1ST) and
// peak_detector_offline::detect_fw (OFFLINE_FW), and the zero-phase peak_detector_offline::detect (k_peak_offline, below).  A detector is a band-pass filter, squaring, an integrating low-pass, a
// low-pass threshold and a small state machine; every sample of a channel depends on the one before, so one lane holds one
// detector and walks its samples in order.  Lanes map to flat (block, channel) pairs (a fresh detector each), or to the
// channels alone when the caller keeps one detector per channel across blocks and calls (stateful mode).
//
// k_peak and k_peak_offline share one frame: their arguments (PeakArgs; PeakOffArgs adds the workspace), their detector state
// (PeakDet; PeakDet<OFFLINE_FW, true> adds the offline object's baseline in unused state slots), the alignment test
// (peak_aligned) and each (block, channel)'s output pointers (peak_out).  The few lines of lane mapping stay in each kernel: moved
// into a helper they changed k_peak's register allocation.
//
// Both kernels have a planar form (k_peak_planar, k_peak_offline_planar) on the converters' int32 matrix [nblocks][nch][ns]: the
// same bodies (k_peak_block_body.hpp, k_peak_offline_block_body.hpp, each included into the native function and into the planar
// one) with a row's address map, so that the native instantiations stay what they were.
//
// Double arithmetic in the reference's order of operations, every product and sum rounded on its own (no FMA: see the pragma),
// so every trace value and every event is bit-identical with the reference's x86-64 build.
#include <cmath>

#include "iir.hpp"

// NO contraction (iir.hpp says why): the filters' products and sums must each be rounded on their own.
#pragma clang fp contract(off)

namespace rspt {

enum : int { kPeakOnline = 0, kPeakOnline1st = 1, kPeakOfflineFw = 2 };
enum : int { kFiltHighPass = 0, kFiltLowPass = 1, kFiltBandPass = 2, kFiltBandStop = 3 };

// ---- the designer (host) ------------------------------------------------------------------------------------------------
// create_filter_iir(num, den, butterworth, type, order, fs, lo, hi): the four designs, in the reference's order of
// operations.  Returns the coefficient count (3, 2, 5 or 3), or 0 where the reference returns false.  pow(k, 2) is k * k (what
// both g++ -O2 and clang make of it); pow(k, 3) and pow(k, 4) stay calls of libm's pow.

// (z - 1)^n (sign < 0) or (z + 1)^n, highest power first: coefficient k is the product of (n - i + 1) / i over i = 1..k
static void binom_row(int n, int sign, double* out) {
    for (int k = 0; k <= n; ++k) {
        double c = 1.0;
        for (int i = 1; i <= k; ++i) c = c * ((double)(n - i + 1) / i);
        out[k] = (sign < 0 && (k & 1)) ? c * -1.0 : (sign < 0 ? c * 1.0 : c);
    }
}

// r[i + j] += p[i] * q[j], from zeros (r holds np + nq - 1 doubles)
static void poly_conv(const double* p, int np, const double* q, int nq, double* r) {
    for (int i = 0; i < np + nq - 1; ++i) r[i] = 0.0;
    for (int i = 0; i < np; ++i)
        for (int j = 0; j < nq; ++j) r[i + j] = r[i + j] + p[i] * q[j];
}

static int design_iir(int type, int order, double fs, double lo, double hi, double* num, double* den) {
    if (type < kFiltHighPass || type > kFiltBandStop) return 0;
    const double pi = M_PI;
    if (order == 2 && (type == kFiltLowPass || type == kFiltHighPass)) {
        if (fs <= 0 || lo <= 0) return 0;
        const double K = tan(pi * lo / fs);
        const double K2 = K * K;
        const double r2 = sqrt(2.0);
        const double a0 = 1.0 + r2 * K + K2;
        const double a1 = 2.0 * (K2 - 1.0);
        const double a2 = 1.0 - r2 * K + K2;
        if (type == kFiltLowPass) {
            num[0] = K2 / a0;
            num[1] = (2.0 * K2) / a0;
            num[2] = K2 / a0;
        } else {
            num[0] = 1.0 / a0;
            num[1] = -2.0 / a0;
            num[2] = 1.0 / a0;
        }
        den[0] = 1.0;
        den[1] = a1 / a0;
        den[2] = a2 / a0;
        return 3;
    }
    if (order == 2) {  // the band-pass from the second-order low-pass prototype: 4th order, 5 coefficients
        if (type != kFiltBandPass || fs <= 0 || lo <= 0 || hi <= lo) return 0;
        const double k = 2.0 / (1.0 / fs);  // bilinear transform s = k (z - 1) / (z + 1)
        const double w1 = k * tan(pi * lo / fs), w2 = k * tan(pi * hi / fs);
        const double bw = w2 - w1;
        const double w0 = sqrt(w1 * w2);
        // analog denominator s^4 + a3 s^3 + a2 s^2 + a1 s + a0 and numerator bw^2 s^2, each power of s taken to z
        const double a3 = sqrt(2.0) * bw;
        const double a2 = 2.0 * w0 * w0 + bw * bw;
        const double a1 = sqrt(2.0) * bw * w0 * w0;
        const double a0 = w0 * w0 * w0 * w0;
        double zm[5][5], zp[5][5];  // zm[n] = (z - 1)^n, zp[n] = (z + 1)^n
        for (int n = 1; n <= 4; ++n) {
            binom_row(n, -1, zm[n]);
            binom_row(n, +1, zp[n]);
        }
        double t[5][5];  // the five terms, unscaled: (z-1)^4, (z-1)^3 (z+1), (z-1)^2 (z+1)^2, (z-1) (z+1)^3, (z+1)^4
        for (int i = 0; i < 5; ++i) t[0][i] = zm[4][i];
        poly_conv(zm[3], 4, zp[1], 2, t[1]);
        poly_conv(zm[2], 3, zp[2], 3, t[2]);
        poly_conv(zm[1], 2, zp[3], 4, t[3]);
        for (int i = 0; i < 5; ++i) t[4][i] = zp[4][i];
        const double s[5] = {1.0 * pow(k, 4), a3 * pow(k, 3), a2 * (k * k), a1 * k, a0};
        double d[5];
        for (int i = 0; i < 5; ++i) d[i] = t[0][i] * s[0];
        for (int j = 1; j < 5; ++j)
            for (int i = 0; i < 5; ++i) d[i] = d[i] + t[j][i] * s[j];
        const double g = bw * bw * (k * k);
        const double nz[5] = {1.0, 0.0, -2.0, 0.0, 1.0};  // (z - 1)^2 (z + 1)^2
        const double norm = d[0];
        for (int i = 0; i < 5; ++i) {
            den[i] = d[i] / norm;
            num[i] = (nz[i] * g) / norm;
        }
        return 5;
    }
    if (order == 1 && (type == kFiltLowPass || type == kFiltHighPass)) {
        if (fs <= 0 || lo <= 0) return 0;
        const double K = tan(pi * lo / fs);
        const double a0 = 1.0 + K, a1 = 1.0 - K;
        num[0] = (type == kFiltLowPass ? K : 1.0) / a0;
        num[1] = (type == kFiltLowPass ? K : -1.0) / a0;
        den[0] = 1.0;
        den[1] = -a1 / a0;
        return 2;
    }
    if (order == 1) {  // band_pass -- and band_stop: the reference's first-order band-pass never looks at the type
        if (fs <= 0 || lo <= 0 || hi <= lo) return 0;
        const double K1 = tan(pi * lo / fs), K2 = tan(pi * hi / fs);
        // a first-order high-pass at lo in series with a first-order low-pass at hi
        const double hn0 = 1.0 / (1.0 + K1), hn1 = -1.0 / (1.0 + K1), hd1 = -(1.0 - K1) / (1.0 + K1);
        const double ln0 = K2 / (1.0 + K2), ln1 = K2 / (1.0 + K2), ld1 = -(1.0 - K2) / (1.0 + K2);
        const double n3[3] = {ln0 * hn0, ln0 * hn1 + ln1 * hn0, ln1 * hn1};
        const double d3[3] = {1.0 * 1.0, 1.0 * hd1 + ld1 * 1.0, ld1 * hd1};
        const double norm = d3[0];
        for (int i = 0; i < 3; ++i) {
            num[i] = n3[i] / norm;
            den[i] = d3[i] / norm;
        }
        return 3;
    }
    return 0;
}

// ---- the detector (device) ----------------------------------------------------------------------------------------------

// Everything a launch needs besides the pointers: the three filters' feed-forward (the designer's numerator, the struct's d)
// and feedback (its denominator, the struct's n) coefficients, and the constants.
struct PeakCoef {
    double bf[5], bb[5];  // band-pass
    double gf[3], gb[3];  // integrator
    double tf[3], tb[3];  // threshold
    double atten;         // 1 / (1 + A / fs)
    double marker;
    int32_t nslope;       // (int)(100 fs / 1000)
    int32_t hist;         // 4 * (int)fs: history calls of the band-pass
};

struct PeakArgs {
    const uint8_t* src;
    uint64_t block_bytes;
    uint32_t stride, nch, ns, nblocks;
    uint32_t lanes;        // nblocks * nch (fresh) or nch (stateful)
    uint8_t* state;        // stateful: the caller's state (PeakStateView), else null
    uint32_t* count;       // [nblocks][nch]
    int32_t* index;        // [nblocks][nch][max_peaks]
    double* value;
    uint64_t max_peaks;
    double* sig;           // [nblocks][ns][nch] (traces), or null
    double* thr;
};

// k_peak_offline's arguments: k_peak's and the workspace
struct PeakOffArgs : PeakArgs {
    uint8_t* work;         // ceil(lanes / 64) slabs of kPeakOffSlabBytesPerSample * ns bytes
};

// The state of one detector per channel, structure of arrays so that lanes of a wave touch consecutive words: 24 doubles
// [field][nch] -- band-pass x[5] y[5], integrator x[3] y[3], threshold x[3] y[3] (newest first), previous peak amplitude,
// previous signal value -- then 4 int32 [field][nch]: searching, samples after the peak, sample index, (unused).  All zero is
// a fresh detector: that is what the reference's constructor leaves.
constexpr uint32_t kPeakStateDoubles = 24, kPeakStateInts = 4;
constexpr uint32_t kPeakStateBytesPerChannel = kPeakStateDoubles * 8 + kPeakStateInts * 4;

// The detectors' filters are the iir_filter_*_order classes: the rings of IirState (iir.hpp), every sample through step_opt
// (their filter() is one expression, all feed-forward terms first), the designer's numerator as d and its denominator as n.
//
// Their init_history_values(x0, .): `steps` calls of filter(x0), where once the x ring holds only x0 the feed-forward sum is
// one number.  NOT IirState::init_history, and not to be merged with it: i_filter::filter interleaves feed-forward and feedback
// terms, while these classes add all feed-forward terms into one number first and then apply the feedback terms -- other
// roundings, other bits.
template <int N>
__device__ void peak_history(IirState<N>& r, const double* n, const double* d, double x0, int32_t steps) {
    int32_t i = 0;
    for (; i < steps && i < N; ++i) r.step_opt(n, d, x0);
    if (i >= steps) return;
    double ff = d[0] * x0;
#pragma unroll
    for (int k = 1; k < N; ++k) ff = ff + d[k] * x0;
    for (; i < steps; ++i) r.feedback(n, ff);
}

// BL: with the baseline filter bl of the offline object (k_peak_offline).  It lives in band-pass slots 3-4 of the state (x) and
// 8-9 (y), which OFFLINE_FW's three-coefficient band-pass never reads or writes: one state can take detect_fw and detect calls
// in turn.  (A base of its own, so that the detectors without it keep their layout.)
template <bool BL>
struct PeakBaseline {};
template <>
struct PeakBaseline<true> {
    IirState<2> bl;
};

template <int V, bool BL = false>
struct PeakDet : PeakBaseline<BL> {
    static constexpr int NB = V == kPeakOnline ? 5 : 3;  // iir_filter_4th_order / iir_filter_2nd_order
    static constexpr int NG = V == kPeakOnline ? 3 : 2;  // iir_filter_2nd_order / iir_filter_1st_order
    static_assert(!BL || V == kPeakOfflineFw, "the baseline belongs to the offline object");
    IirState<NB> bp;
    IirState<NG> ig;
    IirState<3> th;
    double prev_amp, prev_sig;
    int32_t searching, after;
    uint32_t idx;  // sample_indx_ (an int: wraps)

    __device__ void clear() {
        bp.clear();
        ig.clear();
        th.clear();
        prev_amp = prev_sig = 0.0;
        searching = after = 0;
        idx = 0;
        if constexpr (BL) this->bl.clear();
    }
    __device__ void load(const uint8_t* st, uint32_t nch, uint32_t c) {
        const double* d = reinterpret_cast<const double*>(st);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            bp.x[i] = d[(size_t)i * nch + c];
            bp.y[i] = d[(size_t)(5 + i) * nch + c];
        }
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            ig.x[i] = d[(size_t)(10 + i) * nch + c];
            ig.y[i] = d[(size_t)(13 + i) * nch + c];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            th.x[i] = d[(size_t)(16 + i) * nch + c];
            th.y[i] = d[(size_t)(19 + i) * nch + c];
        }
        prev_amp = d[(size_t)22 * nch + c];
        prev_sig = d[(size_t)23 * nch + c];
        const int32_t* w = reinterpret_cast<const int32_t*>(d + (size_t)kPeakStateDoubles * nch);
        searching = w[c];
        after = w[(size_t)nch + c];
        idx = (uint32_t)w[(size_t)2 * nch + c];
        if constexpr (BL) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                this->bl.x[i] = d[(size_t)(3 + i) * nch + c];
                this->bl.y[i] = d[(size_t)(8 + i) * nch + c];
            }
        }
    }
    __device__ void save(uint8_t* st, uint32_t nch, uint32_t c) const {
        double* d = reinterpret_cast<double*>(st);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            d[(size_t)i * nch + c] = bp.x[i];
            d[(size_t)(5 + i) * nch + c] = bp.y[i];
        }
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            d[(size_t)(10 + i) * nch + c] = ig.x[i];
            d[(size_t)(13 + i) * nch + c] = ig.y[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            d[(size_t)(16 + i) * nch + c] = th.x[i];
            d[(size_t)(19 + i) * nch + c] = th.y[i];
        }
        d[(size_t)22 * nch + c] = prev_amp;
        d[(size_t)23 * nch + c] = prev_sig;
        int32_t* w = reinterpret_cast<int32_t*>(d + (size_t)kPeakStateDoubles * nch);
        w[c] = searching;
        w[(size_t)nch + c] = after;
        w[(size_t)2 * nch + c] = (int32_t)idx;
        if constexpr (BL) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                d[(size_t)(3 + i) * nch + c] = this->bl.x[i];
                d[(size_t)(8 + i) * nch + c] = this->bl.y[i];
            }
        }
    }

    // Everything of detect() behind the band-pass output s: squaring and the integrator, the threshold, the state machine
    // (branch-free, as written in the reference).  Returns whether the sample is an event; sig / h: the two trace values.
    __device__ __forceinline__ bool tail(const PeakCoef& c, double s_bp, double& sig, double& h) {
        const double s = ig.step_opt(c.gb, c.gf, s_bp * s_bp);
        h = th.step_opt(c.tb, c.tf, s);
        sig = s;
        return machine(c, s, h);
    }
    // The state machine alone, on the integrator output s and the threshold h of one sample.
    __device__ __forceinline__ bool machine(const PeakCoef& c, double s, double h) {
        const bool c1 = searching && (s > h * 1.5) && (prev_sig > s);
        const bool take = c1 && ((prev_amp == 0.0) || (prev_sig > prev_amp * 0.5));
        const double damped = prev_amp * c.atten;
        const bool rise = !c1 && (prev_sig < s);
        prev_amp = take ? prev_sig : (c1 ? damped : prev_amp);
        after = take ? 1 : (rise ? 0 : after);
        searching = take ? 0 : (rise ? 1 : searching);
        prev_sig = s;
        after = after ? (int32_t)((uint32_t)after + 1u) : 0;
        const bool fire = after == c.nslope;
        after = fire ? 0 : after;
        return fire;
    }
};

// Two doubles side by side in a trace row: one 16-byte store.  A row of doubles starts on an 8-byte boundary and no better
// (row * ns may be odd), which is all a global store of four dwords needs.
typedef double peak_d2 __attribute__((ext_vector_type(2), aligned(8)));
__device__ __forceinline__ void store_d2(double* q, double a, double b) {
    peak_d2 v;
    v.x = a;
    v.y = b;
    *reinterpret_cast<peak_d2*>(q) = v;
}

// Runs one detector through one block (ns samples at p, row stride `stride`); events and traces of this (block, channel).
template <int BPS, int V, bool TR>
__device__ void peak_block(PeakDet<V>& D, const PeakCoef& c, const uint8_t* p, uint32_t stride, uint32_t ns, bool aligned, uint32_t* count,
                           int32_t* index, double* value, uint64_t max_peaks, double* sig, double* thr, uint32_t nch) {
    constexpr bool PLANAR = false;
    const int32_t* row = nullptr;  // (the planar form's arguments: named in the body's planar statements only)
    const bool vec = false;
#include "k_peak_block_body.hpp"
}

// peak_block on a row of the planar int32 matrix: the detector's ns samples side by side at `row` (the whole int32 is the
// sample), its traces the rows sig / thr of ns doubles.  vec: every row of the matrix starts on a 16-byte boundary.
template <int V, bool TR>
__device__ void peak_block_planar(PeakDet<V>& D, const PeakCoef& c, const int32_t* row, uint32_t ns, bool vec, uint32_t* count, int32_t* index,
                                  double* value, uint64_t max_peaks, double* sig, double* thr) {
    constexpr int BPS = 4;
    constexpr bool PLANAR = true;
    const uint8_t* p = nullptr;  // (the native form's arguments: named in the body's native statements only)
    constexpr uint32_t stride = 0, nch = 1;
    constexpr bool aligned = true;
#include "k_peak_block_body.hpp"
}

// Whether both kernels' sample loads may be whole words: wave-uniform, as every block base and row start is aligned when the
// first one is and the sizes are multiples.
template <int BPS>
__device__ __forceinline__ bool peak_aligned(const PeakArgs& a) {
    return (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(a.src) % BPS) == 0 && (a.block_bytes % BPS) == 0;
}

// What the detector of channel ch writes for block b: its count, its first max_peaks events and (TR) its traces, whose samples
// are nch doubles apart.
struct PeakOut {
    uint32_t* count;
    int32_t* index;
    double* value;
    double* sig;
    double* thr;
};
template <bool TR>
__device__ __forceinline__ PeakOut peak_out(const PeakArgs& a, uint32_t b, uint32_t ch) {
    const uint64_t pair = (uint64_t)b * a.nch + ch;
    const uint64_t tr = (uint64_t)b * a.ns * a.nch + ch;
    return PeakOut{a.count + pair, a.index + pair * a.max_peaks, a.value + pair * a.max_peaks, TR ? a.sig + tr : nullptr, TR ? a.thr + tr : nullptr};
}

// One lane per detector: lane q = (block q / nch, channel q % nch) fresh, or channel q through every block (stateful).
template <int BPS, int V, bool TR>
__global__ __launch_bounds__(64) void k_peak(PeakArgs a, PeakCoef c) {
    const uint32_t q = blockIdx.x * 64u + threadIdx.x;
    if (q >= a.lanes) return;
    const bool aligned = peak_aligned<BPS>(a);
    PeakDet<V> D;
    uint32_t b0, b1, ch;
    if (a.state) {
        ch = q;
        b0 = 0;
        b1 = a.nblocks;
        D.load(a.state, a.nch, ch);
    } else {
        b0 = q / a.nch;
        ch = q - b0 * a.nch;
        b1 = b0 + 1;
        D.clear();
    }
    for (uint32_t b = b0; b < b1; ++b) {
        const PeakOut o = peak_out<TR>(a, b, ch);
        peak_block<BPS, V, TR>(D, c, a.src + (size_t)b * a.block_bytes + (size_t)ch * BPS, a.stride, a.ns, aligned, o.count, o.index, o.value,
                               a.max_peaks, o.sig, o.thr, a.nch);
    }
    if (a.state) D.save(a.state, a.nch, ch);
}

// ---- the planar forms ---------------------------------------------------------------------------------------------------
// The samples are the converters' int32 matrix [nblocks][nch][ns] at a.src and the traces matrices of doubles of that shape:
// detector (b, ch) reads row b * nch + ch and writes that row of each trace.  a.block_bytes and a.stride are not used.

// Whether every row of the matrix starts on a 16-byte boundary (wave-uniform): then a lane's chunks may be 16-byte loads.
__device__ __forceinline__ bool peak_rows_vec(const PeakArgs& a) { return (reinterpret_cast<uintptr_t>(a.src) % 16) == 0 && (a.ns % 4u) == 0; }

template <bool TR>
__device__ __forceinline__ PeakOut peak_out_planar(const PeakArgs& a, uint64_t rowi) {
    const uint64_t tr = rowi * a.ns;
    return PeakOut{a.count + rowi, a.index + rowi * a.max_peaks, a.value + rowi * a.max_peaks, TR ? a.sig + tr : nullptr, TR ? a.thr + tr : nullptr};
}

// One lane per detector, as k_peak: lane q is row q (fresh), or channel q through rows q, nch + q, ... (stateful).
template <int V, bool TR>
__global__ __launch_bounds__(64) void k_peak_planar(PeakArgs a, PeakCoef c) {
    const uint32_t q = blockIdx.x * 64u + threadIdx.x;
    if (q >= a.lanes) return;
    const bool vec = peak_rows_vec(a);
    const int32_t* m = reinterpret_cast<const int32_t*>(a.src);
    PeakDet<V> D;
    uint64_t r0 = q, r1 = (uint64_t)q + 1;  // the lane's rows: r0, r0 + step, ... below r1
    if (a.state) {
        r1 = (uint64_t)a.nblocks * a.nch;
        D.load(a.state, a.nch, q);
    } else {
        D.clear();
    }
    for (uint64_t r = r0; r < r1; r += a.nch) {
        const PeakOut o = peak_out_planar<TR>(a, r);
        peak_block_planar<V, TR>(D, c, m + r * a.ns, a.ns, vec, o.count, o.index, o.value, a.max_peaks, o.sig, o.thr);
    }
    if (a.state) D.save(a.state, a.nch, q);
}

// ---- peak_detector_offline::detect (zero-phase) -------------------------------------------------------------------------
// One lane per detector, as k_peak, but every filter runs forward and then backward over the block, so a lane keeps its
// block in a caller-owned workspace.  A wave's slab holds, for its 64 lanes, three double arrays V, F, T and one int32 array
// E, each [ns][64]: the 64 lanes touch 512 consecutive bytes for one t, whatever nch is.  Per block:
//   asc   baseline forward -> V, band-pass forward (state only)
//   desc  baseline backward in place, V = x - baseline; band-pass backward on x -> F
//   asc   integrator forward on F^2 -> F            desc  integrator backward -> F (filt_signal)
//   asc   threshold forward (state only)            desc  threshold backward -> T (threshold_signal)
//   asc   the state machine over (F, T): peak_signal p written over T (T[t] is read before p[t] is written), with the
//         shift folded in (below); E lists the non-zero positions of p
//   the relocation, event by event, on the dense p; then one ascending pass over p for the counts and events.
// The shift loop moves p[i] to p[i - nslope + 1] for ascending i >= nslope.  Its target is never ahead of i and its source
// is never a target of an earlier move, so performing each move at the moment the state machine writes p[i] is the same
// thing; with nslope 1 the move is onto itself, and p[i] = 0 then removes it, as in the reference.

struct PeakOffCoef {
    PeakCoef c;              // band-pass (3 coefficients), integrator (2), threshold (3), atten, marker, nslope, hist
    double lf[2], lb[2];     // baseline low-pass (0.5 Hz, order 1)
    int32_t radius;          // (int)(10 fs / 1000)
};

// bytes of a wave's slab per sample: three double arrays and one int32 array of 64 lanes
constexpr uint64_t kPeakOffSlabBytesPerSample = 64ull * (3 * 8 + 4);

// Walks t over [0, ns) (ascending) or (ns, 0] (descending), CH samples at a time, the next chunk's loads in flight while this
// one runs.  load(t) may read what body writes: the chunk loaded ahead is never the one being written.
template <int CH, bool DESC, class Ld, class Body>
__device__ __forceinline__ void off_walk(uint32_t ns, Ld load, Body body) {
    using T = decltype(load(0u));
    T cur[CH], nxt[CH];
    const uint32_t nfull = ns / CH;
    auto at = [&](uint32_t i) { return DESC ? ns - 1u - i : i; };
    if (nfull) {
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) cur[e] = load(at(e));
    }
    for (uint32_t k = 0; k < nfull; ++k) {
        if (k + 1 < nfull) {
#pragma unroll
            for (uint32_t e = 0; e < CH; ++e) nxt[e] = load(at((k + 1) * CH + e));
        }
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) body(at(k * CH + e), cur[e]);
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) cur[e] = nxt[e];
    }
    for (uint32_t i = nfull * CH; i < ns; ++i) body(at(i), load(at(i)));
}

struct OffPair {
    double a, b;
};
// the planar walks' steps of four samples: the 16 bytes of the row with their four V values; four (F, T) pairs
struct OffXV4 {
    int4 x;
    double v[4];
};
struct OffFT4 {
    OffPair v[4];
};

// Runs detect() once: one block of one detector (band-pass, integrator, threshold, state machine and the baseline D.bl).
// V, F, T, E: this lane's column of its wave's slab (element t at [t * 64]).
template <int BPS, bool TR>
__device__ void peak_offline_block(PeakDet<kPeakOfflineFw, true>& D, const PeakOffCoef& k, const uint8_t* p, uint32_t stride,
                                   uint32_t ns, bool aligned, double* V, double* F, double* T, int32_t* E, uint32_t* count, int32_t* index,
                                   double* value, uint64_t max_peaks, double* sig, double* thr, uint32_t nch) {
    constexpr bool PLANAR = false;
    const int32_t* row = nullptr;  // (the planar form's arguments, as in peak_block)
    const bool vec = false;
#include "k_peak_offline_block_body.hpp"
}

// One lane per detector: lane q = (block q / nch, channel q % nch) fresh, or channel q through every block (stateful).
template <int BPS, bool TR>
__global__ __launch_bounds__(64) void k_peak_offline(PeakOffArgs a, PeakOffCoef k) {
    const uint32_t q = blockIdx.x * 64u + threadIdx.x;
    if (q >= a.lanes) return;
    const bool aligned = peak_aligned<BPS>(a);
    double* V = reinterpret_cast<double*>(a.work + (size_t)blockIdx.x * kPeakOffSlabBytesPerSample * a.ns) + threadIdx.x;
    double* F = V + (size_t)64 * a.ns;
    double* T = F + (size_t)64 * a.ns;
    int32_t* E = reinterpret_cast<int32_t*>(T - threadIdx.x + (size_t)64 * a.ns) + threadIdx.x;
    PeakDet<kPeakOfflineFw, true> D;
    uint32_t b0, b1, ch;
    if (a.state) {
        ch = q;
        b0 = 0;
        b1 = a.nblocks;
        D.load(a.state, a.nch, ch);
    } else {
        b0 = q / a.nch;
        ch = q - b0 * a.nch;
        b1 = b0 + 1;
        D.clear();
    }
    for (uint32_t b = b0; b < b1; ++b) {
        const PeakOut o = peak_out<TR>(a, b, ch);
        peak_offline_block<BPS, TR>(D, k, a.src + (size_t)b * a.block_bytes + (size_t)ch * BPS, a.stride, a.ns, aligned, V, F, T, E, o.count,
                                    o.index, o.value, a.max_peaks, o.sig, o.thr, a.nch);
    }
    if (a.state) D.save(a.state, a.nch, ch);
}

// peak_offline_block on a row of the planar int32 matrix (arguments as peak_block_planar's; the workspace is the native one).
template <bool TR>
__device__ void peak_offline_block_planar(PeakDet<kPeakOfflineFw, true>& D, const PeakOffCoef& k, const int32_t* row, uint32_t ns, bool vec, double* V,
                                          double* F, double* T, int32_t* E, uint32_t* count, int32_t* index, double* value, uint64_t max_peaks,
                                          double* sig, double* thr) {
    constexpr int BPS = 4;
    constexpr bool PLANAR = true;
    const uint8_t* p = nullptr;  // (the native form's arguments, as in peak_block_planar)
    constexpr uint32_t stride = 0, nch = 1;
    constexpr bool aligned = true;
#include "k_peak_offline_block_body.hpp"
}

// One lane per detector, as k_peak_planar; the slabs as k_peak_offline's.
template <bool TR>
__global__ __launch_bounds__(64) void k_peak_offline_planar(PeakOffArgs a, PeakOffCoef k) {
    const uint32_t q = blockIdx.x * 64u + threadIdx.x;
    if (q >= a.lanes) return;
    const bool vec = peak_rows_vec(a);
    const int32_t* m = reinterpret_cast<const int32_t*>(a.src);
    double* V = reinterpret_cast<double*>(a.work + (size_t)blockIdx.x * kPeakOffSlabBytesPerSample * a.ns) + threadIdx.x;
    double* F = V + (size_t)64 * a.ns;
    double* T = F + (size_t)64 * a.ns;
    int32_t* E = reinterpret_cast<int32_t*>(T - threadIdx.x + (size_t)64 * a.ns) + threadIdx.x;
    PeakDet<kPeakOfflineFw, true> D;
    uint64_t r0 = q, r1 = (uint64_t)q + 1;
    if (a.state) {
        r1 = (uint64_t)a.nblocks * a.nch;
        D.load(a.state, a.nch, q);
    } else {
        D.clear();
    }
    for (uint64_t r = r0; r < r1; r += a.nch) {
        const PeakOut o = peak_out_planar<TR>(a, r);
        peak_offline_block_planar<TR>(D, k, m + r * a.ns, a.ns, vec, V, F, T, E, o.count, o.index, o.value, a.max_peaks, o.sig, o.thr);
    }
    if (a.state) D.save(a.state, a.nch, q);
}

}  // namespace rspt
