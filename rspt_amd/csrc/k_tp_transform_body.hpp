// The transform part of the fused probes -- k_target_probe, k_planar_target_probe (target.hip, through k_target_probe_body.hpp) and
// k_budget_probe (budget.hip) -- stated once: one workgroup per (channel, block) reads its row once, keeps it in registers
// (kTpPer samples a thread) and leaves W = WHT(x - mean) mod 2^32 in the first padded LDS buffer, the row's average_32 mean in
// `mean`.  From the kernel: orig, g and the constant kPlanarCut (k_target_probe_body.hpp).  Leaves: W, T (the second buffer, for
// the kernels whose launch gives them one), o[], mean, tid, nt, nw, c, b, n, block_sum4.  Ends behind a barrier.
    extern __shared__ __attribute__((aligned(16))) int32_t sh_i[];
    __shared__ unsigned long long s_part[16][4];
    uint32_t* W = reinterpret_cast<uint32_t*>(sh_i);
    const uint32_t tid = threadIdx.x, nt = blockDim.x, nw = nt >> 6;
    const uint32_t c = blockIdx.x, b = blockIdx.y, n = g.ns;
    uint32_t* T = W + tp_pad(n);
    const int32_t* row = orig + (size_t)b * g.N + (size_t)c * n;

    // a block-wide sum of four 64-bit values per thread, for thread 0 .. 3 the total of value tid
    auto block_sum4 = [&](unsigned long long (&v)[4]) -> unsigned long long {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = q_wave_sum(v[j]);
        if ((tid & 63u) == 0) {
#pragma unroll
            for (int j = 0; j < 4; ++j) s_part[tid >> 6][j] = v[j];
        }
        __syncthreads();
        unsigned long long s = 0;
        if (tid < 4)
            for (uint32_t w = 0; w < nw; ++w) s += s_part[w][tid];
        __syncthreads();
        return s;
    };

    int32_t o[kTpPer];
    unsigned long long first[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t j = 0; j < kTpPer; ++j) {
        const uint32_t i = tid + j * nt;
        o[j] = i < n ? (kPlanarCut ? (int32_t)cut_to_width((uint32_t)row[i], 32u - 8u * g.bps) : row[i]) : 0;
        if (i < n) W[tp_pad(i)] = (uint32_t)o[j];
        first[0] += (unsigned long long)(long long)o[j];
    }
    __shared__ int32_t s_mean;
    {
        const unsigned long long s = block_sum4(first);  // (its first barrier also covers the stores to W)
        if (tid == 0) s_mean = mean_from_sum((long long)s, n);
    }
    __syncthreads();
    const int32_t mean = s_mean;
    tp_fwht(W, n, tid, nt);
    if (tid == 0) W[0] -= (uint32_t)mean * n;  // WHT(x - m) = WHT(x) - m*n*delta_0 (exact mod 2^32)
    __syncthreads();
