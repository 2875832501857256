// The body of k_med_walk<BPS, ALIGNED, STREAM> (median.hip) and of k_medp_walk (median_planar.hip, BPS = kMedPlanar): included
// into both, so that the native instantiations are compiled from the text they always were.
// In scope: keys, rank, dst, g, pair0, sg; BPS, ALIGNED, STREAM.
    extern __shared__ uint32_t med_lds[];
    const uint32_t lane = threadIdx.x;
    const bool writer = lane == 0;
    const uint32_t ns = g.ns, W = g.K;
    const uint32_t spans = ((STREAM ? sg.L : ns) + kMedSpan - 1) / kMedSpan;
    const uint64_t p = blockIdx.x / spans;
    const uint64_t pair = pair0 + p;
    uint32_t lo = (blockIdx.x % spans) * kMedSpan, n = ns, v0 = 0;
    uintptr_t out0;  // address of index 0 of the pair's channel in dst (STREAM: only indices from W - 1 on are stored); not PLANAR
    constexpr bool PLANAR = BPS == kMedPlanar;
    constexpr int SB = PLANAR ? 4 : BPS;
    static_assert(!PLANAR || STREAM, "planar: the carried form only; the stateless call runs the bps = 4 kernels on rows of one channel");
    uint32_t first = 0;  // PLANAR: index W - 1 of the segment is row `first` of the call
    if (STREAM) {
        const uint32_t j = sg.nseg - 1u - (uint32_t)(pair / g.nch);
        n = W - 1u + min(sg.L, sg.N - j * sg.L);
        lo += W - 1u;
        if (lo >= n) return;  // (a span past a short last segment)
        if (j == 0) v0 = W - 1u - (uint32_t)*reinterpret_cast<const uint64_t*>(sg.head);
        if constexpr (PLANAR) first = j * sg.L;  // (a row of the call has no address linear in its index: med_planar_at)
        else out0 = reinterpret_cast<uintptr_t>(dst) + (uint32_t)(pair % g.nch) * SB + (uint64_t)((int64_t)j * sg.L - (int64_t)(W - 1u)) * g.stride;
    } else {
        out0 = reinterpret_cast<uintptr_t>(dst) + (pair / g.nch) * g.block_bytes + (uint32_t)(pair % g.nch) * SB;
    }
    const uint32_t hi = min(n, lo + kMedSpan);
    const uint32_t n0 = (ns + 31) / 32;
    MedBits bm{med_lds, med_lds + n0, (n0 + 31) / 32};
    for (uint32_t i = lane; i < n0 + bm.n1; i += 64) med_lds[i] = 0;
    __syncthreads();
    const uint32_t* rk = rank + p * ns;
    const uint64_t* kp = keys + p * ns;
    // the window of output lo - 1: samples [s0, lo)
    const uint32_t s0 = lo >= W + v0 ? lo - W : v0;
    for (uint32_t t = s0 + lane; t < lo; t += 64) {
        const uint32_t r = rk[t];
        atomicOr(&bm.b0[r >> 5], 1u << (r & 31));
        atomicOr(&bm.b1[r >> 10], 1u << ((r >> 5) & 31));
    }
    __syncthreads();
    uint32_t m = lo - s0;  // reals in the window
    uint32_t pm = 0, below = 0;
    if (m) {  // the lower median: set bit number (m - 1) / 2, by a wave-wide count over the words of b0
        const uint32_t k = (m - 1) / 2;
        const uint32_t per = (n0 + 63) / 64, w0 = lane * per, w1 = min(n0, w0 + per);
        uint32_t cnt = 0;
        for (uint32_t w = w0; w < w1; ++w) cnt += __builtin_popcount(bm.b0[w]);
        uint32_t incl = cnt;
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        const uint32_t excl = incl - cnt;
        uint32_t found = 0;
        if (excl <= k && k < incl) {  // exactly one lane
            uint32_t left = k - excl;
            for (uint32_t w = w0; w < w1; ++w) {
                uint32_t bits = bm.b0[w];
                const uint32_t c = __builtin_popcount(bits);
                if (left < c) {
                    for (; left; --left) bits &= bits - 1;
                    found = (w << 5) | (uint32_t)__builtin_ctz(bits);
                    break;
                }
                left -= c;
            }
        }
        const uint64_t who = __ballot(excl <= k && k < incl);
        pm = __shfl(found, (int)__builtin_ctzll(who), 64);
        below = k;
    }
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t n = min(64u, hi - base);
        const uint32_t t = base + lane;
        const uint32_t rn = t < hi ? rk[t] : 0;
        const uint32_t ro = (t < hi && t >= W + v0) ? rk[t - W] : 0;
        uint32_t myp = 0, myq = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const uint32_t tj = base + j;
            const uint32_t r = __shfl(rn, (int)j, 64);
            bm.set(r, writer);
            if (m == 0) {
                pm = r;
                below = 0;
            } else if (r < pm) {
                ++below;
            }
            ++m;
            if (tj >= W + v0) {  // the window is full: sample tj - W leaves
                const uint32_t o = __shfl(ro, (int)j, 64);
                --m;
                bm.clear(o, writer);
                if (o < pm) {
                    --below;
                } else if (o == pm) {
                    const uint32_t nx = bm.next(pm);
                    if (nx != ~0u) {
                        pm = nx;
                    } else {
                        pm = bm.prev(pm);
                        --below;
                    }
                }
            }
            const uint32_t k = (m - 1) / 2;
            while (below < k) {
                pm = bm.next(pm);
                ++below;
            }
            while (below > k) {
                pm = bm.prev(pm);
                --below;
            }
            const uint32_t q = (m & 1) ? pm : bm.next(pm);
            if (lane == j) {
                myp = pm;
                myq = q;
            }
        }
        if (lane < n) {
            const int64_t sum = (int64_t)med_key_value(kp[myp]) + (int64_t)med_key_value(kp[myq]);
            if constexpr (PLANAR)
                *reinterpret_cast<int32_t*>(dst + med_planar_at(sg, g.nch, (uint32_t)(pair % g.nch), first + (t - (W - 1u)))) = (int32_t)(sum / 2);
            else sample_store<BPS>(reinterpret_cast<uint8_t*>(out0 + (uint64_t)t * g.stride), (int32_t)(sum / 2), ALIGNED);
        }
    }
