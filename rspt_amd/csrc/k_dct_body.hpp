// The body of k_dct and k_dct_l (transforms.hip), included into both so that the kernel of one setting stays the code that was
// timed.  From the kernel: in, g, means, tab, scale0, scale1, cs0, out.
    __shared__ float s_src[kDctCh][kDctChunk];
    __shared__ long long s_red[4];
    __shared__ int32_t s_mean[kDctCh];
    const uint32_t tid = threadIdx.x;
    const uint32_t n = g.ns;
    const uint32_t i = blockIdx.x * 256 + tid;
    const uint32_t c0 = blockIdx.y * kDctCh;
    const uint32_t b = blockIdx.z;
    const uint32_t nc = min((uint32_t)kDctCh, g.nch - c0);

    if (FORWARD) {
        for (uint32_t cc = 0; cc < nc; ++cc) {
            long long t = block_sum_row(in + (size_t)b * g.N + (size_t)(c0 + cc) * n, n, s_red);
            if (tid == 0) {
                const int32_t m = mean_from_sum(t, n);
                s_mean[cc] = m;
                if (blockIdx.x == 0) store_mean_hdr(means, g, b, c0 + cc, m);
            }
        }
    } else if (tid < nc) {
        s_mean[tid] = load_mean_hdr(means, g, b, c0 + tid);
    }
    __syncthreads();

    double sum[kDctCh] = {0, 0, 0, 0};
    for (uint32_t x0 = 0; x0 < n; x0 += kDctChunk) {
        const uint32_t cn = min(kDctChunk, n - x0);
        for (uint32_t cc = 0; cc < nc; ++cc)
            for (uint32_t x = tid; x < cn; x += 256) {
                int32_t v = in[(size_t)b * g.N + (size_t)(c0 + cc) * n + x0 + x];
                float f;
                if (FORWARD) {
                    v = (int32_t)((uint32_t)v - (uint32_t)s_mean[cc]);  // offset_32(-mean), dct.cpp:108-109
                    f = (float)v;                                        // `int * float`: the int converts to float
                } else {
                    f = (float)v;
                    if (x0 + x == 0) f = __fmul_rn(cs0, f);  // Cs[x]*dct[x] in float, Cs[0]=(float)(1/sqrt 2) (dct.cpp:95)
                }
                s_src[cc][x] = f;
            }
        __syncthreads();
        if (i < n) {
            for (uint32_t x = 0; x < cn; ++x) {
                const float cv = tab[(size_t)(x0 + x) * n + i];
#pragma unroll
                for (int cc = 0; cc < kDctCh; ++cc) {
                    // float product, then sequential accumulation in double, no contraction
                    sum[cc] = __dadd_rn(sum[cc], (double)__fmul_rn(s_src[cc][x], cv));
                }
            }
        }
        __syncthreads();
    }
    if (i < n) {
        for (uint32_t cc = 0; cc < nc; ++cc) {
            double s;
            if (FORWARD)
                s = __dmul_rn(sum[cc], i == 0 ? scale0 : scale1);  // sum *= Cs[i]*sqrt(2/n)/128 (dct.cpp:84)
            else
                s = __dmul_rn(sum[cc], scale1);                    // sum *= sqrt(2/n)*128 (dct.cpp:97)
            int32_t r = trunc_i32_c(s);                              // C truncation (dct.cpp:85,98)
            if (!FORWARD) r = (int32_t)((uint32_t)r + (uint32_t)s_mean[cc]);
            out[(size_t)b * g.N + (size_t)(c0 + cc) * n + i] = r;
        }
    }
