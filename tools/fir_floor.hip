// fir_floor.hip -- the f64 issue-rate floor of tools/fir_rate.py: how fast the device retires one v_mul_f64 and one v_add_f64
// per tap and output, the work the FIR stage (rspt_amd/csrc/fir.hip) cannot avoid.  Every lane runs 16 independent
// accumulator chains acc = acc + x * k, as k_fir does, with the same 256-thread workgroups; no loads in the loop.
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

__global__ __launch_bounds__(256) void k_fir_floor(double* out, const double* __restrict__ coef, int iters) {
    double acc[16], x[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        acc[r] = 0.0;
        x[r] = (double)(threadIdx.x + r);
    }
    for (int i = 0; i < iters; ++i) {
        const double k = coef[i & 15];  // (wave-uniform: a scalar load, as in k_fir)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = acc[r] + x[r] * k;
    }
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < 16; ++r) s = s + acc[r];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

// f64 operations (mul + add) issued per launch: grid * 256 * iters * 16 * 2
extern "C" int fir_floor_launch(double* out, const double* coef, int grid, int iters, void* stream) {
    hipLaunchKernelGGL(k_fir_floor, dim3(grid), dim3(256), 0, (hipStream_t)stream, out, coef, iters);
    return (int)hipGetLastError();
}
