// The body of k_med_tile_sort<BPS, ALIGNED, STREAM> (median.hip) and of k_medp_tile_sort (median_planar.hip, BPS = kMedPlanar):
// included into both, so that the native instantiations are compiled from the text they always were.
// In scope: src, keys, rank, g, pair0, sg; BPS, ALIGNED, STREAM.
    __shared__ uint64_t sk[kMedTile];
    const uint32_t tiles = (g.ns + kMedTile - 1) / kMedTile;
    const uint64_t p = blockIdx.x / tiles;
    const uint32_t t0 = (blockIdx.x % tiles) * kMedTile;
    const uint64_t pair = pair0 + p;
    const uint32_t ch = (uint32_t)(pair % g.nch);
    constexpr bool PLANAR = BPS == kMedPlanar;
    constexpr int SB = PLANAR ? 4 : BPS;  // bytes of a stored sample
    static_assert(!PLANAR || STREAM, "planar: the carried form only; the stateless call runs the bps = 4 kernels on rows of one channel");
    if (STREAM) {
        const uint32_t j = sg.nseg - 1u - (uint32_t)(pair / g.nch);
        const uint32_t n = g.K - 1u + min(sg.L, sg.N - j * sg.L);
        const int64_t first = (int64_t)j * sg.L - (int64_t)(g.K - 1u);  // the call's row of index 0
        const uint8_t* hrow0 = sg.head + 8 + (uint64_t)(g.K - 1u) * g.stride + ch * SB;  // where row 0 would be in the head
        for (uint32_t i = threadIdx.x; i < kMedTile; i += kMedThreads) {
            const uint32_t t = t0 + i;
            uint64_t k = ~0ull;
            if (t < n) {
                const int64_t r = first + (int64_t)t;
                const uint8_t* at;
                if constexpr (PLANAR) at = r < 0 ? hrow0 - (uint64_t)(-r) * g.stride : src + med_planar_at(sg, g.nch, ch, (uint32_t)r);
                else at = r < 0 ? hrow0 - (uint64_t)(-r) * g.stride : src + (uint64_t)r * g.stride + ch * BPS;
                k = med_key(sample_load<SB>(at, PLANAR || ALIGNED), t);
            } else if (t < g.ns) {
                k = 0xFFFFFFFF00000000ull | t;
            }
            sk[i] = k;
        }
    } else {
        const uint8_t* base = src + (pair / g.nch) * g.block_bytes + ch * SB;
        for (uint32_t i = threadIdx.x; i < kMedTile; i += kMedThreads) {
            const uint32_t t = t0 + i;
            sk[i] = t < g.ns ? med_key(sample_load<SB>(base + (uint64_t)t * g.stride, ALIGNED), t) : ~0ull;  // (padding sorts last)
        }
    }
    __syncthreads();
    for (uint32_t k = 2; k <= kMedTile; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < kMedTile; i += kMedThreads) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t x = sk[i], y = sk[ixj];
                    if (((i & k) == 0) == (x > y)) {
                        sk[i] = y;
                        sk[ixj] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    uint64_t* kp = keys + p * g.ns;
    for (uint32_t i = threadIdx.x; i < kMedTile && t0 + i < g.ns; i += kMedThreads) {
        kp[t0 + i] = sk[i];
        if (rank) rank[p * g.ns + (uint32_t)sk[i]] = t0 + i;
    }
