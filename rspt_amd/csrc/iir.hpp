// iir.hpp -- the reference's IIR filter object, stated once for the IIR, cascade and peak kernels.
//
// Restates i_filter::new_iir / init_history_values / filter / filter_opt of lib_rspt/lib_filter/iir_filter.cpp:46-116: two
// rings of up to five doubles, x[i] = input i samples ago, y[i] = output i samples ago.  Double arithmetic in the reference's
// order of operations, every product and sum rounded on its own, so a result is bit-identical with the reference's.
// The tests judge these kernels against the same object stated once in numpy: tests/iir_model.py.
#pragma once
#include <type_traits>

#include "common.hpp"

// NO contraction.  hipcc's default is -ffp-contract=fast, and HIP's __dmul_rn / __dadd_rn are plain operators (not
// the contraction barriers their CUDA namesakes are): left alone, the compiler fuses the recurrence's products and sums into
// v_fma_f64 (83 of them in the round-2 kernel).  One fused rounding is ~1e-16 relative -- but this band-pass has poles at
// 0.9994 and coefficients that cancel (3.14 y1 - 3.70 y2 + 1.97 y3 - 0.41 y4), which amplifies it to ~1e-7 absolute, enough to
// move the truncated output by one count about once in 2 million samples (found on the 64 x 65536 bench batch; the small
// fixtures never hit it).  With contraction off every product and sum is rounded on its own, as in the reference's x86-64 build.
// The pragma holds for this header's body, and a file that uses these filters in expressions of its own sets it again behind
// its includes.  At its end the header goes back to `fast`, which is hipcc's default and what this library is built with: a
// build with another -ffp-contract would have it overridden behind this header.
#pragma clang fp contract(off)

namespace rspt {

struct IirCoef {
    double n[5], d[5];  // feedback (n[0] unused) and feed-forward coefficients
    uint32_t nc;        // 2..5
    int32_t init_steps;  // 4 * nr_samples of init_history_values (iir_filter.cpp:106-110)
};

// The carried state of one filter (layout: rspt_hip.h): the rings as the reference's object holds them between two filter_opt
// calls, newest first, the y ring as untruncated doubles.  All-zero bytes: a filter that has not started (its first call runs
// init_history_values).
struct IirCarry {
    double x[5], y[5];
    uint64_t started;
};
static_assert(sizeof(IirCarry) == 88, "rspt_hip.h documents 88 bytes per channel");

// f(std::integral_constant<int, NC>()) for a coefficient count of 2..5 (on the device nc is wave-uniform: a scalar branch)
template <class F>
__host__ __device__ __forceinline__ void by_nc(uint32_t nc, F&& f) {
    switch (nc) {
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        default: f(std::integral_constant<int, 5>{}); break;
    }
}

// The filter object (x_ring_ / y_ring_ of iir_filter.cpp:46-62).  n: feedback coefficients (n[0] unused), d: feed-forward.
template <int NC>
struct IirState {
    double x[NC], y[NC];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < NC; ++i) x[i] = y[i] = 0.0;
    }
    __device__ __forceinline__ void shift(double in) {  // iir_filter.cpp:66-71
#pragma unroll
        for (int i = NC - 1; i > 0; --i) {
            x[i] = x[i - 1];
            y[i] = y[i - 1];
        }
        x[0] = in;
    }
    // i_filter::filter (iir_filter.cpp:64-77): the terms join the sum one by one, feed-forward and feedback interleaved
    __device__ __forceinline__ double step(const double* n, const double* d, double in) {
        shift(in);
        double acc = (d[0] * x[0]);
#pragma unroll
        for (int i = 1; i < NC; ++i) {
            acc = (acc + (d[i] * x[i]));
            acc = (acc - (n[i] * y[i]));
        }
        y[0] = acc;
        return acc;
    }
    // i_filter::filter_opt (iir_filter.cpp:79-104 with :23-41), and filter() of the iir_filter_*_order classes: ONE expression
    // evaluated left to right, all feed-forward terms first,
    //     ff = (((d0 x0 + d1 x1) + d2 x2) + d3 x3) + d4 x4            -- no output in it: it can be formed ahead of time (iir_ff)
    //     y  = (((ff - n1 y1) - n2 y2) - n3 y3) - n4 y4                -- the serial part (feedback)
    __device__ __forceinline__ double step_opt(const double* n, const double* d, double in) {
        shift(in);
        double a = d[0] * x[0];
#pragma unroll
        for (int i = 1; i < NC; ++i) a = a + d[i] * x[i];
#pragma unroll
        for (int i = 1; i < NC; ++i) a = a - n[i] * y[i];
        y[0] = a;
        return a;
    }
    // the feedback half of a filter_opt step whose feed-forward sum ff is known; the x ring is the caller's to keep
    __device__ __forceinline__ double feedback(const double* n, double ff) {
        double a = ff;
#pragma unroll
        for (int i = 1; i < NC; ++i) a = a - n[i] * y[i - 1];  // (y[i-1] now = y[i] of the step being taken)
#pragma unroll
        for (int i = NC - 1; i > 0; --i) y[i] = y[i - 1];
        y[0] = a;
        return a;
    }
    // step() once the whole x ring holds one value: the feed-forward products d[i] * x[i] are the same numbers every time
    // -- P[i], computed once -- and only the feedback products are new
    __device__ __forceinline__ void step_const(const double* n, const double (&P)[NC]) {
#pragma unroll
        for (int i = NC - 1; i > 0; --i) y[i] = y[i - 1];
        double acc = P[0];
#pragma unroll
        for (int i = 1; i < NC; ++i) {
            acc = (acc + P[i]);
            acc = (acc - (n[i] * y[i]));
        }
        y[0] = acc;
    }
    // init_history_values (iir_filter.cpp:106-110): init_steps = 4 * nr_samples calls of filter() on x0.
    // (k_iir_pipe and casc_start carry this same loop written out: called from them it compiles to other instructions, and the
    // pipelined kernels are kept instruction for instruction what was timed.  Change the three together.)
    __device__ __forceinline__ void init_history(const IirCoef& c, double x0) {
        int32_t i = 0;
        for (; i < c.init_steps && i < NC; ++i) step(c.n, c.d, x0);  // (until the x ring holds nothing but x0)
        if (i < c.init_steps) {
            double P[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) P[k] = c.d[k] * x0;
            // (unrolled by the ring's length: the shifts of y become register names instead of moves)
#pragma unroll 4
            for (; i < c.init_steps; ++i) step_const(c.n, P);
        }
    }
    // the rings outside the code that knows their length: five places each, newest first; store leaves those past NC - 1 zero
    __device__ __forceinline__ void load(const double (&rx)[5], const double (&ry)[5]) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            x[i] = rx[i];
            y[i] = ry[i];
        }
    }
    __device__ __forceinline__ void store(double (&rx)[5], double (&ry)[5]) const {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            rx[i] = i < NC ? x[i < NC ? i : 0] : 0.0;
            ry[i] = i < NC ? y[i < NC ? i : 0] : 0.0;
        }
    }
};

// The feed-forward sum ((d0 x0 + d1 x1) + d2 x2) + ... of the sample at xs[0]; xs[-i] is the input i samples before it.
template <int NC>
__device__ __forceinline__ double iir_ff(const double* d, const double* xs) {
    double a = d[0] * xs[0];
#pragma unroll
    for (int i = 1; i < NC; ++i) a = a + d[i] * xs[-i];
    return a;
}

// Place i of the x ring of a fresh filter behind init_history(c, x0): what stands i + 1 samples in front of a run for whoever
// forms the run's feed-forward sums -- x0 in the first min(init_steps, nc) places, 0.0 behind them.
__device__ __forceinline__ double iir_front(const IirCoef& c, double x0, int i) { return i < c.init_steps && i < (int)c.nc ? x0 : 0.0; }

}  // namespace rspt

#pragma clang fp contract(fast)  // (hipcc's default: see the top)
