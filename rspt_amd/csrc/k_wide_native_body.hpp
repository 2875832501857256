// The body of k_wide_native and k_wide_native_l (convert.hip), included into both so that the kernel of every block stays the code
// that was timed.  From the kernel: planar, g, dst.
    constexpr uint32_t RW = 16u * BPS;  // dwords of a full output row of the tile: 64 samples of BPS bytes
    constexpr uint32_t RS = RW + 1u;    // row stride: the spare word is what the last dword of an unaligned row reads beyond it
    __shared__ uint32_t tile[64][65];
    __shared__ uint32_t rows_mem[64 * RS + 2];
    uint32_t* rows = rows_mem + 1;  // (the first dword of an unaligned row reads the word in front of it)
    const uint32_t tid = threadIdx.x, b = blockIdx.z;
    const uint32_t s0 = blockIdx.x * 64u, c0 = blockIdx.y * 64u;
    const uint32_t nt = min(64u, g.ns - s0), nc = min(64u, g.nch - c0);
    const int32_t* in = planar + (size_t)b * g.N + (size_t)c0 * g.ns + s0;
    if ((g.ns & 3u) == 0 && (reinterpret_cast<uintptr_t>(planar) & 15u) == 0) {  // (then N, s0 and nt are multiples of 4 too)
        const uint32_t t4 = tid & 15u;
        for (uint32_t c = tid >> 4; c < 64u; c += 16u) {
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (c < nc && 4u * t4 < nt) v = *reinterpret_cast<const uint4*>(in + (size_t)c * g.ns + 4u * t4);
            uint32_t* r = &tile[c][4u * t4];
            r[0] = v.x;
            r[1] = v.y;
            r[2] = v.z;
            r[3] = v.w;
        }
    } else {
        const uint32_t t = tid & 63u;
        for (uint32_t c = tid >> 6; c < 64u; c += 4u) tile[c][t] = (c < nc && t < nt) ? (uint32_t)in[(size_t)c * g.ns + t] : 0u;
    }
    __syncthreads();
    {
        const uint32_t c4 = tid & 15u;
        for (uint32_t t = tid >> 4; t < 64u; t += 16u) {
            uint32_t v[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                v[k] = tile[4u * c4 + k][t];
                if (BPS > 1 && g.be) v[k] = __builtin_amdgcn_perm(v[k], v[k], 0x00010203u) >> (8 * (4 - BPS));  // the low BPS bytes reversed
            }
            uint32_t* w = rows + t * RS + c4 * BPS;
            if (BPS == 4) {
                w[0] = v[0];
                w[1] = v[1];
                w[2] = v[2];
                w[3] = v[3];
            } else if (BPS == 3) {
                w[0] = (v[0] & 0xFFFFFFu) | (v[1] << 24);
                w[1] = ((v[1] >> 8) & 0xFFFFu) | (v[2] << 16);
                w[2] = ((v[2] >> 16) & 0xFFu) | (v[3] << 8);
            } else if (BPS == 2) {
                w[0] = (v[0] & 0xFFFFu) | (v[1] << 16);
                w[1] = (v[2] & 0xFFFFu) | (v[3] << 16);
            } else {
                w[0] = (v[0] & 0xFFu) | ((v[1] & 0xFFu) << 8) | ((v[2] & 0xFFu) << 16) | (v[3] << 24);
            }
        }
    }
    __syncthreads();
    const size_t rowb = (size_t)g.nch * BPS;
    uint8_t* out = dst + (size_t)b * g.block_bytes + ((size_t)s0 * g.nch + c0) * BPS;
    const uint32_t L = nc * BPS;  // bytes of the tile's piece of a sample row
    if (((reinterpret_cast<uintptr_t>(out) | rowb | L) & 15u) == 0) {
        constexpr uint32_t PW = 4u * BPS;  // 16-byte pieces of a full row
        for (uint32_t u = tid; u < 64u * PW; u += 256u) {
            const uint32_t t = u / PW, k = u - t * PW;
            if (t < nt && 16u * k < L) {
                const uint32_t* r = rows + t * RS + 4u * k;
                *reinterpret_cast<uint4*>(out + t * rowb + 16u * k) = make_uint4(r[0], r[1], r[2], r[3]);
            }
        }
        return;
    }
    constexpr uint32_t JW = RW + 1u;  // aligned dwords that a row of RW * 4 bytes can touch
    for (uint32_t u = tid; u < 64u * JW; u += 256u) {
        const uint32_t t = u / JW, j = u - t * JW;
        if (t >= nt) break;
        uint8_t* ro = out + t * rowb;
        const uint32_t a = (uint32_t)(reinterpret_cast<uintptr_t>(ro) & 3u);
        const int32_t first = (int32_t)(4u * j) - (int32_t)a;  // the row byte that aligned dword j starts at
        if (first >= (int32_t)L) continue;
        const uint32_t* r = rows + ((int32_t)(t * RS) + (first >> 2));  // (first >= -3: the word in front of the row at most)
        const uint32_t val = __builtin_amdgcn_alignbyte(r[1], r[0], (4u - a) & 3u);
        uint8_t* q = ro + first;
        if (first >= 0 && first + 4 <= (int32_t)L) {
            *reinterpret_cast<uint32_t*>(q) = val;
        } else {  // a row's ragged first or last dword
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (first + i >= 0 && first + i < (int32_t)L) q[i] = (uint8_t)(val >> (8 * i));
        }
    }
