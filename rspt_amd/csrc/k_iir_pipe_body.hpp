// k_iir_pipe_body.hpp -- the body of k_iir_pipe and of k_iir_pipe_planar (filter.hip, which says why it is a file): included
// into a kernel that declares BPS, NC, SHARED, ALIGNED, CARRY and PLANAR and takes (buf, nch, ns, block_bytes, c, nblocks,
// lanes_per_wg, state).  Not a header: no include guard, included twice on purpose.
    static_assert(NC >= 2 && NC <= 5, "IirPipeLds::xlast holds five inputs per channel");
    static_assert(!(SHARED && CARRY), "a carried state is one filter per channel");
    __shared__ IirPipeLds L;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t role = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // lanes_per_wg < 64 spreads the lanes over more workgroups: in shared mode a lane is a BLOCK, its accesses are 16 MiB apart
    // from its neighbours', and 64 of them per CU would ask one CU's memory path for more than it can give
    const uint32_t unit = blockIdx.x * lanes_per_wg + lane;
    uint32_t b, ch0, nser;
    if (SHARED) {
        b = unit;
        ch0 = 0;
        nser = nch;
    } else {
        b = unit / nch;
        ch0 = unit - b * nch;
        nser = 1;
    }
    // six waves on four SIMDs: the wave with the recurrence shares its SIMD with a producer -- it goes first whenever it can issue
    if (role == 0u) __builtin_amdgcn_s_setprio(3);
    const bool valid = lane < lanes_per_wg && b < nblocks;  // (lanes past the batch read block 0 along with the others and store nothing)
    const size_t stride = (size_t)nch * BPS;
    constexpr bool aligned = ALIGNED;  // (the host has looked at the base address: one load / store instruction per sample)
    uint8_t* base = buf + (size_t)(valid ? b : 0u) * block_bytes + (size_t)(valid ? ch0 : 0u) * BPS;
    if constexpr (PLANAR) base = buf + (size_t)(valid ? b : 0u) * block_bytes + (size_t)(valid ? ch0 : 0u) * planar_run<!CARRY>(buf, nch, ns, block_bytes).hns * 4u;
    const uint32_t nchunks = (ns + kIirChunk - 1) / kIirChunk;
    IirState<NC> f;
    f.clear();
    constexpr int H = NC - 1;            // inputs in front of a sample that its feed-forward sum needs
    constexpr uint32_t SET = kIirPart + H;  // a producer's samples per chunk: its part and the H in front of it
    constexpr uint32_t kWriter = 1 + kIirProd;
    // (lanes past the shape look at channel 0's state along with it and write nothing)
    IirCarry* const cs = CARRY ? state + (valid ? ch0 : 0u) : nullptr;
    const bool started = CARRY && cs->started != 0;
    for (uint32_t sc = 0; sc < nser; ++sc) {
        uint8_t* p = base + (size_t)sc * BPS;
        if constexpr (PLANAR) p = base + (size_t)sc * ns * 4u;  // (shared mode is stateless: a row is ns samples)
        const double x0 = (double)sample_load<BPS>(p, aligned);
        int32_t cur[SET], nxt[SET], nx2[SET];
        // element j of a producer's set in chunk t is sample t * 64 + (role - 1) * 16 - H + j; in front of the channel: the history (x0, see below)
        auto load_set = [&](int32_t (&v)[SET], uint32_t t) {
            const int32_t s0 = (int32_t)(t * kIirChunk + (role - 1u) * kIirPart) - H;
            if constexpr (PLANAR) {
                planar_load_set<(uint32_t)H, !CARRY>(planar_run<!CARRY>(p, nch, ns, block_bytes), ns, s0, v);
            } else if (s0 >= 0 && s0 + (int32_t)SET <= (int32_t)ns) {  // (wave-uniform; all but a channel's first and last sets)
                const uint8_t* q = p + (size_t)s0 * stride;
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) v[j] = sample_load<BPS>(q + (size_t)j * stride, aligned);
            } else {
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) {
                    int32_t si = s0 + (int32_t)j;
                    si = si < 0 ? 0 : si >= (int32_t)ns ? (int32_t)ns - 1 : si;  // (clamped: what lies outside is never used as such)
                    v[j] = sample_load<BPS>(p + (size_t)si * stride, aligned);
                }
            }
        };
        const bool producer = role >= 1u && role <= kIirProd;
        if (producer) {
            load_set(cur, 0);
            if (nchunks > 1) load_set(nxt, 1);
        }
        for (uint32_t t = 0; t < nchunks + 2; ++t) {
            if (role == 0u) {
                if (CARRY && t == 0 && started) {  // (the y ring alone: this wave never reads x, the first producer takes it from the state)
#pragma unroll
                    for (int i = 0; i < NC; ++i) f.y[i] = cs->y[i];
                } else if (t == 0) {
                    // IirState::init_history, written out: as a call it compiles to other code here (see above the kernel)
                    int32_t i = 0;
                    for (; i < c.init_steps && i < NC; ++i) f.step(c.n, c.d, x0);  // (until the x ring holds nothing but x0)
                    if (i < c.init_steps) {
                        double P[NC];
#pragma unroll
                        for (int k = 0; k < NC; ++k) P[k] = c.d[k] * x0;
                        // (unrolled by the ring's length: the shifts of y become register names instead of moves)
#pragma unroll 4
                        for (; i < c.init_steps; ++i) f.step_const(c.n, P);
                    }
                } else if (t <= nchunks) {
                    const uint32_t k = t - 1, bi = k & 1u;
                    const uint32_t cnt = min(kIirChunk, ns - k * kIirChunk);
                    auto rec = [&](double ff) { return f.feedback(c.n, ff); };
                    if (cnt == kIirChunk) {
                        // sixteen samples at a time: their feed-forward sums are read from LDS together (one wait), the results
                        // written together -- per sample the wave issues the recurrence and little else.  The truncation is the
                        // GPU's own (saturating) conversion here; C's as the reference's build does it (trunc_i32_c, common.hpp) differs
                        // from it only where this conversion returns INT_MAX (the double is >= 2^31 or +inf) and where the double
                        // is NaN (this conversion: 0).  The largest result of the chunk is tracked (half an instruction per sample
                        // instead of two); a NaN needs no tracking, because it is absorbing: the step after it multiplies it by
                        // n[1], so every later output is NaN and the chunk's last one says whether any was (its high word: an
                        // all-ones exponent, NaN or +-inf).  A chunk that reaches INT_MAX -- full-scale input through a filter that
                        // overshoots -- or ends non-finite -- an unstable filter, non-finite coefficients -- is done once more, exactly.
                        double ysave[NC];
#pragma unroll
                        for (int i = 0; i < NC; ++i) ysave[i] = f.y[i];
                        int32_t mx = (int32_t)0x80000000u;
#pragma unroll 1
                        for (uint32_t e0 = 0; e0 < kIirChunk; e0 += 16) {
                            double a[16];
                            int32_t o[16];
#pragma unroll
                            for (uint32_t e = 0; e < 16; ++e) a[e] = L.ff[bi][e0 + e][lane];
#pragma unroll
                            for (uint32_t e = 0; e < 16; ++e) o[e] = (int32_t)rec(a[e]);
#pragma unroll
                            for (uint32_t e = 0; e < 16; e += 2) mx = max(mx, max(o[e], o[e + 1]));  // (v_max3_i32)
#pragma unroll
                            for (uint32_t e = 0; e < 16; ++e) L.out[bi][e0 + e][lane] = o[e];
                        }
                        if (__builtin_expect(__builtin_amdgcn_ballot_w64(mx == 0x7FFFFFFF || (__double2hiint(f.y[0]) & 0x7FF00000) == 0x7FF00000) != 0ull, 0)) {
#pragma unroll
                            for (int i = 0; i < NC; ++i) f.y[i] = ysave[i];
#pragma unroll 1
                            for (uint32_t e = 0; e < kIirChunk; ++e) L.out[bi][e][lane] = trunc_i32_c(rec(L.ff[bi][e][lane]));
                        }
                    } else {
                        for (uint32_t e = 0; e < cnt; ++e) L.out[bi][e][lane] = trunc_i32_c(rec(L.ff[bi][e][lane]));  // C truncation (rspt_test.cpp:130)
                    }
                    if (SHARED && t == nchunks) {  // the x ring the next channel's initialisation starts from (its first NC - 1 calls see it)
#pragma unroll
                        for (int i = 0; i < NC; ++i) f.x[i] = L.xlast[i][lane];
                    }
                    if (CARRY && t == nchunks && valid) {  // the object as it stands behind the call's last sample
#pragma unroll
                        for (int i = 0; i < NC; ++i) {
                            cs->x[i] = L.xlast[i][lane];
                            cs->y[i] = f.y[i];
                        }
                        cs->started = 1;
                    }
                }
            } else if (role == kWriter) {
                if (t >= 2) {
                    const uint32_t k = t - 2, bi = k & 1u;
                    const uint32_t cnt = min(kIirChunk, ns - k * kIirChunk);
                    uint8_t* q = p + (size_t)k * kIirChunk * stride;
                    if constexpr (PLANAR) {
                        const PlanarRun run = planar_run<!CARRY>(p, nch, ns, block_bytes);
#pragma unroll 1
                        for (uint32_t e0 = 0; e0 < cnt; e0 += 16) {
                            int32_t v[16];
#pragma unroll
                            for (uint32_t e = 0; e < 16; ++e) v[e] = L.out[bi][e0 + e][lane];
                            planar_store_part<!CARRY>(run, k * kIirChunk + e0, min(16u, cnt - e0), v, valid);
                        }
                    } else if (cnt == kIirChunk) {
#pragma unroll 1
                        for (uint32_t e0 = 0; e0 < kIirChunk; e0 += 16) {
                            int32_t v[16];
#pragma unroll
                            for (uint32_t e = 0; e < 16; ++e) v[e] = L.out[bi][e0 + e][lane];
                            if (valid) {
#pragma unroll
                                for (uint32_t e = 0; e < 16; ++e) sample_store<BPS>(q + (size_t)(e0 + e) * stride, v[e], aligned);
                            }
                        }
                    } else {
                        for (uint32_t e = 0; e < cnt; ++e) {
                            const int32_t v = L.out[bi][e][lane];
                            if (valid) sample_store<BPS>(q + (size_t)e * stride, v, aligned);
                        }
                    }
                }
            } else if (t < nchunks) {
                if (t + 2 < nchunks) load_set(nx2, t + 2);  // (two chunks ahead: the loads have two ticks to arrive)
                // the inputs as doubles; in front of the channel's first sample the x ring holds x0 (init_steps >= NC - 1: the host checks)
                const int32_t s0 = (int32_t)(t * kIirChunk + (role - 1u) * kIirPart) - H;
                double xs[SET];
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) xs[j] = (double)cur[j];
                if (s0 < 0) {  // (wave-uniform: the first producer's first set only)
#pragma unroll
                    for (uint32_t j = 0; j < SET; ++j) xs[j] = (s0 + (int32_t)j < 0) ? x0 : xs[j];
                    if (CARRY) {  // (s0 = -H: element j < H is the input H - j samples in front of the call, place H - 1 - j of the x ring)
#pragma unroll
                        for (int j = 0; j < H; ++j) xs[j] = started ? cs->x[H - 1 - j] : (H - 1 - j < c.init_steps ? x0 : 0.0)  /* iir_front: the place is below NC */;
                    }
                }
#pragma unroll
                for (uint32_t e = 0; e < kIirPart; ++e) {  // (iir_ff, written out)
                    double a = c.d[0] * xs[H + e];
#pragma unroll
                    for (int i = 1; i < NC; ++i) a = a + c.d[i] * xs[H + e - i];
                    L.ff[t & 1u][(role - 1u) * kIirPart + e][lane] = a;
                }
                if ((SHARED || CARRY) && t + 1 == nchunks) {  // whoever holds the channel's last sample hands its last inputs on
                    const int32_t last = (int32_t)ns - 1 - (s0 + H);  // index of sample ns-1 in this wave's part
                    if (last >= 0 && last < (int32_t)kIirPart) {
#pragma unroll
                        for (int i = 0; i < NC; ++i) {
                            double v = 0.0;
#pragma unroll
                            for (uint32_t j = 0; j < SET; ++j)
                                if ((int32_t)j == last + H - i) v = xs[j];
                            L.xlast[i][lane] = v;
                        }
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < SET; ++j) {
                    cur[j] = nxt[j];
                    nxt[j] = nx2[j];
                }
            }
            __syncthreads();
        }
    }
