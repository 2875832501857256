// The body of k_fwht, k_fwht_q and k_fwht_l (transforms.hip), included into each so that the quality-1 kernel stays the code that was
// timed.  From the kernel: planar, g, means; QUANT (constexpr bool) and, where it is set, div (the kernel's last argument).
    extern __shared__ __attribute__((aligned(16))) int32_t sh[];
    __shared__ long long s_red[16];
    const uint32_t tid = threadIdx.x;
    const uint32_t c = blockIdx.x, b = blockIdx.y;
    const uint32_t n = g.ns;
    int32_t* row = planar + (size_t)b * g.N + (size_t)c * n;
    const uint32_t k = 31u - (uint32_t)__builtin_clz(n);

    int32_t mean;
    if (FORWARD) {
        mean = mean_from_sum(block_sum_row(row, n, s_red), n);
        if (tid == 0) store_mean_hdr(means, g, b, c, mean);
    } else {
        mean = load_mean_hdr(means, g, b, c);
    }

    const uint32_t hn = n > 32768u ? 32768u : n;
    const uint32_t halves = QUANT ? 1u : n / hn;  // 1 or 2 (the host sends n = 65536 to k_fwht64k: the general quantiser leaves that form out)
    int32_t keep[32];                // results of half 0 while half 1's inputs are still being read
    for (uint32_t h = 0; h < halves; ++h) {
        for (uint32_t i = tid; i < hn; i += 1024) {
            uint32_t a = (uint32_t)row[i];
            if (halves == 2) {
                const uint32_t bb = (uint32_t)row[i + hn];
                a = h == 0 ? a + bb : a - bb;
            }
            sh[i] = (int32_t)a;
        }
        __syncthreads();
        if (h == 1) {
#pragma unroll
            for (int jj = 0; jj < 32; ++jj) row[tid + 1024u * jj] = keep[jj];
        }
        // (lo,hi) -> (lo+hi, lo-hi) per stage (fwht.c:19-22); the stages commute exactly in wrap-around arithmetic, so
        // three of them are taken at a time on eight values held in registers: a third of the LDS traffic and barriers
        uint32_t w = hn >> 1;
        while (w >= 4) {  // stages w, w/2, w/4 together: elements base + {0..7} * (w/4)
            const uint32_t st = w >> 2;
            for (uint32_t q = tid; q < (hn >> 3); q += 1024) {
                const uint32_t base = ((q & ~(st - 1)) << 3) | (q & (st - 1));
                uint32_t v[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = (uint32_t)sh[base + i * st];
#pragma unroll
                for (int d = 4; d >= 1; d >>= 1) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        if (!(i & d)) {
                            const uint32_t x = v[i], y = v[i + d];
                            v[i] = x + y;
                            v[i + d] = x - y;
                        }
                    }
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) sh[base + i * st] = (int32_t)v[i];
            }
            __syncthreads();
            w >>= 3;
        }
        for (; w >= 1; w >>= 1) {  // the one or two stages left
            for (uint32_t q = tid; q < (hn >> 1); q += 1024) {
                const uint32_t lo = ((q & ~(w - 1)) << 1) | (q & (w - 1));
                const uint32_t x = (uint32_t)sh[lo], y = (uint32_t)sh[lo + w];
                sh[lo] = (int32_t)(x + y);
                sh[lo + w] = (int32_t)(x - y);
            }
            __syncthreads();
        }
        auto finish = [&](uint32_t idx, int32_t y) -> int32_t {
            if (FORWARD) {
                // WHT(x - m) = WHT(x) - m*n*delta_0 (exact mod 2^32)
                if (idx == 0) y = (int32_t)((uint32_t)y - (uint32_t)mean * n);
                if (QUANT) return fwht_quant(y, div);
                // fwht_normalize (fwht.c:30-34): int /= (n/1.0) = truncation toward zero
                return (y + ((y >> 31) & (int32_t)(n - 1))) >> k;
            }
            if (QUANT) y = fwht_quant(y, div);
            return (int32_t)((uint32_t)y + (uint32_t)mean);
        };
        if (halves == 2 && h == 0) {
#pragma unroll
            for (int jj = 0; jj < 32; ++jj) keep[jj] = finish(tid + 1024u * jj, sh[tid + 1024u * jj]);
        } else {
            for (uint32_t i = tid; i < hn; i += 1024) row[h * hn + i] = finish(h * hn + i, sh[i]);
        }
        __syncthreads();
    }
