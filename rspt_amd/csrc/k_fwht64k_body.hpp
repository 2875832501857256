// The body of k_fwht64k, k_fwht64k_q and k_fwht64k_l (transforms.hip), included into each so that the quality-1 kernel stays the code that
// was timed.  From the kernel: planar, g, means, planes, nzflag, nplanes; QUANT (constexpr bool) and, where it is set, div.
    extern __shared__ __attribute__((aligned(16))) int32_t sh_i[];
    uint32_t* sh = reinterpret_cast<uint32_t*>(sh_i);
    __shared__ long long s_red[16];
    const uint32_t tid = threadIdx.x;
    const uint32_t c = blockIdx.x, b = blockIdx.y;
    constexpr uint32_t n = 65536u, k = 16u;
    int32_t* row = planar + (size_t)b * g.N + (size_t)c * n;

    uint32_t v[64];  // layout 1: v[4 q + e] = row[4096 q + 4 tid + e]
#pragma unroll
    for (uint32_t q = 0; q < 16; ++q) {
        const uint4 x = reinterpret_cast<const uint4*>(row)[q * 1024 + tid];
        v[4 * q] = x.x;
        v[4 * q + 1] = x.y;
        v[4 * q + 2] = x.z;
        v[4 * q + 3] = x.w;
    }
    int32_t mean;
    if (FORWARD) {
        long long sum = 0;
#pragma unroll
        for (int i = 0; i < 64; ++i) sum += (int32_t)v[i];
        sum = wave_add_i64(sum);
        if ((tid & 63u) == 0) s_red[tid >> 6] = sum;
        __syncthreads();
        long long t = 0;
        for (uint32_t i = 0; i < 16; ++i) t += s_red[i];
        mean = mean_from_sum(t, n);
        if (tid == 0) store_mean_hdr(means, g, b, c, mean);
    } else {
        mean = load_mean_hdr(means, g, b, c);
    }
    fwht_regs<0, 6>(v);  // bits 0, 1, 12..15
    // (pinned: left alone the scheduler sinks the last stage's differences -- needed in the second round only -- behind the first
    //  round's LDS reads and keeps both of their inputs instead: 64 + 64 live registers and two dozen of them in scratch memory)
#pragma unroll
    for (int i = 32; i < 64; ++i) asm volatile("" : "+v"(v[i]));

    // transpose 1: layout 1 -> layout 2
    uint32_t w[64];
    const uint32_t half = tid >> 9;  // bit 15 of the elements this thread holds in layouts 2 and 3
    const uint32_t base2 = (((tid >> 6) & 7u) << 12) | (((tid >> 2) & 15u) << 8) | (tid & 3u);
    const uint32_t swz2 = (base2 >> 8) & 7u;  // what fwht_swz flips in bits 2..4 of this thread's layout-2 addresses
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
#pragma unroll
        for (uint32_t qq = 0; qq < 8; ++qq) {
            const uint32_t q = h * 8 + qq;
            *reinterpret_cast<uint4*>(&sh[fwht_swz((qq << 12) | (tid << 2))]) = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        }
        __syncthreads();
        if (half == h) {
            // fwht_swz(base2 | r << 2) = base2 + ((r & 7 ^ c) << 2) + (r >> 3 << 5) with c = bits 8..10 of base2: eight addresses and
            // immediate offsets (sixty-four computed addresses are sixty-four registers the three arrays do not leave)
#pragma unroll
            for (uint32_t n = 0; n < 8; ++n) {
                const uint32_t* pn = sh + (base2 | ((n ^ swz2) << 2));
#pragma unroll
                for (uint32_t m = 0; m < 8; ++m) w[8 * m + n] = pn[m << 5];
            }
        }
        __syncthreads();
    }
    fwht_regs<0, 6>(w);  // bits 2..7

    // transpose 2: layout 2 -> layout 3 (each half: written and read by the same 512 threads).  Read back INTO w: with an
    // array of its own the second round's stores still need w while the first round's loads are live -- 128 registers for the
    // compiler, which cannot know that no thread takes part in both rounds, and 22 of them went to scratch memory (104
    // scratch instructions per thread next to 64 loads and stores of data).
    uint32_t(&u)[64] = w;
    const uint32_t base3 = (((tid >> 6) & 7u) << 12) | ((tid & 63u) << 2);
#pragma unroll
    for (uint32_t h = 0; h < 2; ++h) {
        if (half == h) {
#pragma unroll
            for (uint32_t n = 0; n < 8; ++n) {
                uint32_t* pn = sh + (base2 | ((n ^ swz2) << 2));
#pragma unroll
                for (uint32_t m = 0; m < 8; ++m) pn[m << 5] = w[8 * m + n];
            }
        }
        __syncthreads();
        if (half == h) {
#pragma unroll
            for (uint32_t pp = 0; pp < 16; ++pp) {
                const uint4 x = *reinterpret_cast<const uint4*>(&sh[fwht_swz(base3 | (pp << 8))]);
                u[4 * pp] = x.x;
                u[4 * pp + 1] = x.y;
                u[4 * pp + 2] = x.z;
                u[4 * pp + 3] = x.w;
            }
        }
        __syncthreads();
    }
    fwht_regs<2, 6>(u);  // bits 8..11 (register-index bits 2..5; bits 0, 1 of the index are done)
#pragma unroll
    for (int i = 0; i < 64; ++i) asm volatile("" : "+v"(u[i]));  // (the output phase starts from 64 finished values, not in the middle of the butterflies)

    const uint32_t i0 = ((tid >> 6) << 12) | ((tid & 63u) << 2);  // bits 15..12 and 7..2
    uint32_t nzk[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t pp = 0; pp < 16; ++pp) {
        const uint32_t idx = i0 | (pp << 8);
        uint32_t o[4];
#pragma unroll
        for (uint32_t e = 0; e < 4; ++e) {
            int32_t y = (int32_t)u[4 * pp + e];
            if (FORWARD) {
                // WHT(x - m) = WHT(x) - m*n*delta_0 (exact mod 2^32); fwht_normalize (fwht.c:30-34): truncation toward zero
                if (idx + e == 0) y = (int32_t)((uint32_t)y - (uint32_t)mean * n);
                if (QUANT)
                    y = fwht_quant(y, div);
                else
                    y = (y + ((y >> 31) & (int32_t)(n - 1))) >> k;
            } else {
                if (QUANT) y = fwht_quant(y, div);
                y = (int32_t)((uint32_t)y + (uint32_t)mean);
            }
            o[e] = (uint32_t)y;
        }
        if (!PLANES) {
            *reinterpret_cast<uint4*>(row + idx) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            // 4 x 4 byte transpose (preprocess.hip: transform_item): one dword per plane
            const uint32_t lo01 = __builtin_amdgcn_perm(o[1], o[0], 0x05010400u), hi01 = __builtin_amdgcn_perm(o[1], o[0], 0x07030602u);
            const uint32_t lo23 = __builtin_amdgcn_perm(o[3], o[2], 0x05010400u), hi23 = __builtin_amdgcn_perm(o[3], o[2], 0x07030602u);
            const uint32_t pl[4] = {__builtin_amdgcn_perm(lo23, lo01, 0x05040100u), __builtin_amdgcn_perm(lo23, lo01, 0x07060302u),
                                    __builtin_amdgcn_perm(hi23, hi01, 0x05040100u), __builtin_amdgcn_perm(hi23, hi01, 0x07060302u)};
#pragma unroll
            for (uint32_t kk = 0; kk < 4; ++kk) {
                if (kk < nplanes) {
                    *reinterpret_cast<uint32_t*>(planes + ((size_t)b * kMaxPlanes + kk) * g.plane_stride + (size_t)c * n + idx) = pl[kk];
                    nzk[kk] |= pl[kk];
                }
            }
            asm volatile("" ::: "memory");  // (one quad of outputs at a time: interleaved, their temporaries spill)
        }
    }
    if (PLANES) {
        const uint32_t flat = c * n + i0;  // this wave's outputs: [flat & ~4095, +4096)
        for (uint32_t kk = 0; kk < nplanes; ++kk)
            if (__ballot(nzk[kk] != 0) && (tid & 63u) == 0) atomicOr(&nzflag[hb_index(g, b, kk, flat >> 16)], 1u << ((flat >> 12) & 15u));
    }
