// k_iir_zp_pipe_body.hpp -- the body of k_iir_zp_pipe and of k_iir_zp_pipe_planar (iir_zero_phase.hip, which says why it is a
// file): included once into each, with BPS, NC, ALIGNED and PLANAR in scope.  The planar statements are under
// `if constexpr (PLANAR)`; everything else is the native kernel's, statement for statement.
    __shared__ ZpLds L;
    const uint32_t role = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    ZpWave w;
    w.lane = threadIdx.x & 63u;
    const uint32_t unit = blockIdx.x * 64u + w.lane;
    const uint32_t b = unit / nch, ch = unit - b * nch;
    w.valid = b < nblocks;
    w.stride = (size_t)nch * BPS;
    w.p = buf + (size_t)(w.valid ? b : 0u) * block_bytes + (size_t)(w.valid ? ch : 0u) * BPS;
    if constexpr (PLANAR) {  // the lane's row of the source: samples side by side, the channels' rows ns samples apart
        w.stride = 4;
        w.p = buf + (size_t)(w.valid ? b : 0u) * block_bytes + (size_t)(w.valid ? ch : 0u) * ns * 4u;
    }
    w.W = work + (size_t)blockIdx.x * ns * 64u + w.lane;
    w.ns = ns;
    w.nchunks = (ns + kZpChunk - 1) / kZpChunk;
    w.x0 = (double)sample_load<BPS>(w.p, ALIGNED);  // (from the source, in front of every store: no lane stores before its backward pass)
    if (role == 0u) {
        // six waves on four SIMDs: the wave with the recurrence shares its SIMD with a producer -- it goes first whenever it can issue
        __builtin_amdgcn_s_setprio(3);
        zp_wave_rec<NC>(L, w, c, back_steps);
    } else if (role == kZpWriter) {
        if constexpr (PLANAR) w.p = dst + (w.p - buf);  // the same row of the destination (the writer's forward pass stores to the workspace only)
        zp_wave_write<BPS, ALIGNED, PLANAR>(L, w);
    } else {
        zp_wave_prod<BPS, NC, ALIGNED, PLANAR>(L, w, c, back_steps, role - 1u);
    }
