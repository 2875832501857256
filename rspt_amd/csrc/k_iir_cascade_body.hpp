// k_iir_cascade_body.hpp -- the body of k_iir_cascade and of k_iir_cascade_planar (iir_cascade.hip; filter.hip says why it is a
// file): included into a kernel that declares BPS, CARRY and PLANAR and takes (buf, nch, ns, block_bytes, a, nblocks, state).
// Not a header: no include guard, included twice on purpose.
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    const uint32_t b = t / nch, ch = t - b * nch;
    if (b >= nblocks) return;
    const size_t stride = (size_t)nch * BPS;
    const bool aligned = (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(buf) % BPS) == 0 && (block_bytes % BPS) == 0;
    uint8_t* p = buf + (size_t)b * block_bytes + (size_t)ch * BPS;
    if constexpr (PLANAR) p = buf + (size_t)b * block_bytes + (size_t)ch * planar_run<!CARRY>(buf, nch, ns, block_bytes).hns * 4u;
    IirCarry* const cs = CARRY ? state + (size_t)ch * a.nsec : nullptr;
    const bool started = CARRY && cs[0].started != 0;
    const double x0 = (double)sample_load<BPS>(p, aligned);
    double x[kCascMaxSections][5], y[kCascMaxSections][5];
#pragma unroll
    for (uint32_t k = 0; k < kCascMaxSections; ++k) {
        if (k < a.nsec) casc_start(a.s[k], x0, started, CARRY ? cs + k : nullptr, x[k], y[k]);
    }
    for (uint32_t s = 0; s < ns; ++s) {
        uint8_t* q = p + (size_t)s * stride;
        if constexpr (PLANAR) q = reinterpret_cast<uint8_t*>(CARRY ? planar_run<false>(p, nch, ns, block_bytes).at(s) : reinterpret_cast<int32_t*>(p) + s);
        double v = (double)sample_load<BPS>(q, aligned);
#pragma unroll
        for (uint32_t k = 0; k < kCascMaxSections; ++k) {
            if (k >= a.nsec) continue;
            const bool filt = (a.use_filter >> k) & 1u;
            by_nc(a.s[k].nc, [&](auto ncv) {
                IirState<decltype(ncv)::value> f;
                f.load(x[k], y[k]);
                v = filt ? f.step(a.s[k].n, a.s[k].d, v) : f.step_opt(a.s[k].n, a.s[k].d, v);
                f.store(x[k], y[k]);
            });
        }
        sample_store<BPS>(q, trunc_i32_c(v), aligned);  // C truncation, once, behind the last section
    }
    if (CARRY) {
#pragma unroll
        for (uint32_t k = 0; k < kCascMaxSections; ++k) {
            if (k >= a.nsec) continue;
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                cs[k].x[i] = x[k][i];
                cs[k].y[i] = y[k][i];
            }
            cs[k].started = 1;
        }
    }
