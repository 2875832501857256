// k_iir_cascade_pipe_body.hpp -- the body of k_iir_cascade_pipe and of k_iir_cascade_pipe_planar (iir_cascade.hip; filter.hip says
// why it is a file): included into a kernel that declares BPS, ALIGNED, CARRY and PLANAR and takes (buf, nch, ns, block_bytes, a,
// nblocks, state).  Not a header: no include guard, included twice on purpose.
    __shared__ CascLds L;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t S = a.nsec;
    std::conditional_t<PLANAR, CascWavePlanar, CascWave> w;
    w.lane = threadIdx.x & 63u;
    const uint32_t unit = blockIdx.x * 64u + w.lane;
    const uint32_t b = unit / nch, ch0 = unit - b * nch;
    w.valid = b < nblocks;
    w.stride = (size_t)nch * BPS;
    w.p = buf + (size_t)(w.valid ? b : 0u) * block_bytes + (size_t)(w.valid ? ch0 : 0u) * BPS;
    if constexpr (PLANAR) casc_planar_start<!CARRY>(w, buf, nch, ns, block_bytes, w.valid ? b : 0u, w.valid ? ch0 : 0u);
    w.ns = ns;
    w.nchunks = (ns + kCascChunk - 1) / kCascChunk;
    w.nticks = w.nchunks + 2 * S;
    w.tiles = L.v;
    w.x0 = (double)sample_load<BPS>(w.p, ALIGNED);
    IirCarry* const cs0 = CARRY ? state + (size_t)(w.valid ? ch0 : 0u) * S : nullptr;
    w.started = CARRY && cs0->started != 0;
    auto section = [&](uint32_t k) {
        w.cs = CARRY ? cs0 + k : nullptr;
        w.filt = ((a.use_filter >> k) & 1u) != 0;
        return a.s[k];
    };
    if (wave < S) {
        __builtin_amdgcn_s_setprio(3);  // a recurrence wave goes first whenever it can issue
        w.off = 2 * wave + 1;
        casc_wave_rec<CARRY>(w, section(wave));
    } else if (wave < 2 * S - 1) {
        const uint32_t k = wave - S + 1;
        w.off = 2 * k;
        casc_wave_ff<CARRY>(w, section(k));
    } else if (wave < 2 * S + 1) {
        w.off = 0;
        casc_wave_prod<BPS, ALIGNED, CARRY>(w, section(0), wave - (2 * S - 1));
    } else {
        w.off = 2 * S;
        casc_wave_store<BPS, ALIGNED, CARRY>(w);
    }
