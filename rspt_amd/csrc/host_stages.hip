// host_stages.hip -- the host side of the analysis stages: IIR, IIR cascade, zero-phase IIR, FIR, median, PRDN, converters, R-peak detectors; each stage's
// launchers directly in front of its entries.  Included by rspt_hip.hip.

// The widest handle the filter, median, peak and PRDN stages are verified on (tests/test_gpu_wide_channels.py): beyond it they
// return RSPT_HIP_ERR_UNSUPPORTED before anything is launched.
static constexpr uint32_t kStageMaxChannels = 8191;
static bool stage_too_wide(const rspt_hip_packer* p) { return p->g.nch > kStageMaxChannels; }

// A batch whose (block, channel) pairs the stages count in 32 bits: at least one block and nblocks * nch < 2^31 (nch >= 1:
// rspt_hip_packer_create), as a division so that no nblocks wraps the product.
static bool batch_count_ok(const rspt_hip_packer* p, size_t nblocks) { return nblocks != 0 && nblocks <= 0x7FFFFFFFu / p->g.nch; }

// Whole-sample loads and stores: int16 / int32 samples in buffers on a sample boundary (block_bytes is a multiple of bps).
static bool native_aligned(uint32_t bps, const void* src, const void* dst) {
    return (bps == 4 || bps == 2) && reinterpret_cast<uintptr_t>(src) % bps == 0 && reinterpret_cast<uintptr_t>(dst) % bps == 0;
}

// A carried-state call takes its blocks as one run of nblocks * ns rows, indexed in 32 bits with a chunk's reach beyond the last
// row: runs of 2^31 - 2^17 rows and more are refused, and the caller splits the call (with a state that split is exact).
static constexpr uint64_t kStreamMaxRows = (1ull << 31) - (1ull << 17);

// ---- IIR pre-filter (filter.hip) ----
template <int BPS, int NC>
static void launch_iir(rspt_hip_packer* p, uint8_t* buf, uint32_t B, const IirCoef& c, int per_channel, hipStream_t st) {
    const Geom& g = p->g;
    if (g.ns >= kIirChunk && c.init_steps >= NC - 1) {  // the pipelined form: recurrence, feed-forward sums and stores on waves of their own
        const bool al = (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(buf) % BPS) == 0;  // (block_bytes is a multiple of BPS)
        if (per_channel) {
            const uint32_t units = B * g.nch;
            auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((units + 63) / 64), dim3(kIirThreads), 0, st, buf, g.nch, g.ns, (uint64_t)g.block_bytes, c, B, 64u, (IirCarry*)nullptr); };
            if (al) go(&k_iir_pipe<BPS, NC, false, (BPS == 4 || BPS == 2)>);
            else go(&k_iir_pipe<BPS, NC, false, false>);
        } else {
            // shared mode: lane <-> block; few lanes per workgroup so that the blocks' scattered accesses spread over the CUs
            uint32_t lpw = (B + (uint32_t)p->num_cu - 1) / (uint32_t)p->num_cu;
            lpw = lpw < 1 ? 1 : lpw > 64 ? 64 : lpw;
            auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((B + lpw - 1) / lpw), dim3(kIirThreads), 0, st, buf, g.nch, g.ns, (uint64_t)g.block_bytes, c, B, lpw, (IirCarry*)nullptr); };
            if (al) go(&k_iir_pipe<BPS, NC, true, (BPS == 4 || BPS == 2)>);
            else go(&k_iir_pipe<BPS, NC, true, false>);
        }
        return;
    }
    if (per_channel) {
        const uint32_t threads = B * g.nch;
        hipLaunchKernelGGL((k_iir<BPS, NC, false>), dim3((threads + 63) / 64), dim3(64), 0, st, buf, g.nch, g.ns, (uint64_t)g.block_bytes, c, B);
    } else {
        hipLaunchKernelGGL((k_iir<BPS, NC, true>), dim3((B + 63) / 64), dim3(64), 0, st, buf, g.nch, g.ns, (uint64_t)g.block_bytes, c, B);
    }
}

// The carried form (rspt_hip_iir_prefilter_stream_dev): the call's blocks as one run of `rows` rows, lane <-> channel, the
// filters in `state`.  Whether a channel is fresh is known on the device only, so the route depends on the run's length alone.
template <int BPS, int NC>
static void launch_iir_stream(rspt_hip_packer* p, uint8_t* buf, uint32_t rows, const IirCoef& c, IirCarry* state, hipStream_t st) {
    const Geom& g = p->g;
    const dim3 grid((g.nch + 63) / 64);
    if (rows >= kIirChunk) {
        const bool al = (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(buf) % BPS) == 0;
        const uint64_t run_bytes = (uint64_t)rows * g.nch * BPS;
        auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(kIirThreads), 0, st, buf, g.nch, rows, run_bytes, c, 1u, 64u, state); };
        if (al) go(&k_iir_pipe<BPS, NC, false, (BPS == 4 || BPS == 2), true>);
        else go(&k_iir_pipe<BPS, NC, false, false, true>);
        return;
    }
    hipLaunchKernelGGL((k_iir_carry<BPS, NC>), grid, dim3(64), 0, st, buf, g.nch, rows, c, state);
}

// The planar entries (rspt_hip_iir_prefilter_planar_*_dev): the native routes on the int32 matrix [B][nch][ns], whatever the
// handle's bps.  A kernel takes block_bytes as one block of the matrix; a carried call is one run of B * ns rows through B of them.
template <int NC>
static void launch_iir_planar(rspt_hip_packer* p, int32_t* d_planar, uint32_t B, const IirCoef& c, int per_channel, IirCarry* state, hipStream_t st) {
    const Geom& g = p->g;
    uint8_t* buf = reinterpret_cast<uint8_t*>(d_planar);
    const uint64_t block_bytes = (uint64_t)g.nch * g.ns * 4u;
    if (state) {
        const dim3 grid((g.nch + 63) / 64);
        const uint32_t rows = B * g.ns;  // (below kStreamMaxRows: iir_call)
        if (rows >= kIirChunk)
            hipLaunchKernelGGL((k_iir_pipe_planar<NC, false, true>), grid, dim3(kIirThreads), 0, st, buf, g.nch, rows, block_bytes, c, 1u, 64u, state);
        else
            hipLaunchKernelGGL((k_iir_planar_carry<NC>), grid, dim3(64), 0, st, d_planar, g.nch, g.ns, B, c, state);
        return;
    }
    if (g.ns >= kIirChunk && c.init_steps >= NC - 1) {
        if (per_channel) {
            const uint32_t units = B * g.nch;
            hipLaunchKernelGGL((k_iir_pipe_planar<NC, false, false>), dim3((units + 63) / 64), dim3(kIirThreads), 0, st, buf, g.nch, g.ns, block_bytes, c, B,
                               64u, (IirCarry*)nullptr);
        } else {  // (lanes per workgroup as in launch_iir: a lane is a block)
            uint32_t lpw = (B + (uint32_t)p->num_cu - 1) / (uint32_t)p->num_cu;
            lpw = lpw < 1 ? 1 : lpw > 64 ? 64 : lpw;
            hipLaunchKernelGGL((k_iir_pipe_planar<NC, true, false>), dim3((B + lpw - 1) / lpw), dim3(kIirThreads), 0, st, buf, g.nch, g.ns, block_bytes, c, B,
                               lpw, (IirCarry*)nullptr);
        }
        return;
    }
    if (per_channel) hipLaunchKernelGGL((k_iir_planar<NC, false>), dim3((B * g.nch + 63) / 64), dim3(64), 0, st, d_planar, g.nch, g.ns, c, B);
    else hipLaunchKernelGGL((k_iir_planar<NC, true>), dim3((B + 63) / 64), dim3(64), 0, st, d_planar, g.nch, g.ns, c, B);
}

// All four IIR entries: d_state == NULL is the stateless call on nblocks blocks, else the blocks are one run behind the state;
// planar: d_buf is the int32 matrix.
static int iir_call(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, size_t nr_coefficients, int init_nr_samples,
                    int per_channel, void* d_state, void* stream, bool planar = false) {
    if (!p || !d_buf || !n || !d || !batch_count_ok(p, nblocks)) return RSPT_HIP_ERR_ARG;
    if (planar && reinterpret_cast<uintptr_t>(d_buf) % 4) return RSPT_HIP_ERR_ARG;
    if (nr_coefficients < 2 || nr_coefficients > 5 || init_nr_samples < 0 || init_nr_samples > (1 << 28)) return RSPT_HIP_ERR_ARG;  // filter_opt covers 2..5 (iir_filter.cpp:87-103)
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    const uint64_t rows = (uint64_t)nblocks * p->g.ns;
    if (d_state && rows >= kStreamMaxRows) return RSPT_HIP_ERR_UNSUPPORTED;
    HIPCHK(p, hipSetDevice(p->device));
    IirCoef c{};
    for (size_t i = 0; i < nr_coefficients; ++i) {
        c.n[i] = n[i];
        c.d[i] = d[i];
    }
    c.nc = (uint32_t)nr_coefficients;
    c.init_steps = 4 * init_nr_samples;
    hipStream_t st = (hipStream_t)stream;
    if (planar) {
        by_nc(c.nc, [&](auto ncv) { launch_iir_planar<decltype(ncv)::value>(p, (int32_t*)d_buf, (uint32_t)nblocks, c, per_channel, (IirCarry*)d_state, st); });
        HIPCHK(p, hipGetLastError());
        return RSPT_HIP_OK;
    }
    by_bps(p->g.bps, [&](auto bps) {
        by_nc(c.nc, [&](auto ncv) {
            constexpr int BPS = decltype(bps)::value, NC = decltype(ncv)::value;
            if (d_state) launch_iir_stream<BPS, NC>(p, (uint8_t*)d_buf, (uint32_t)rows, c, (IirCarry*)d_state, st);
            else launch_iir<BPS, NC>(p, (uint8_t*)d_buf, (uint32_t)nblocks, c, per_channel, st);
        });
    });
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_iir_prefilter_batch_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, size_t nr_coefficients,
                                     int init_nr_samples, int per_channel, void* stream) {
    return iir_call(p, d_buf, nblocks, n, d, nr_coefficients, init_nr_samples, per_channel, nullptr, stream);
}

int rspt_hip_iir_state_bytes(rspt_hip_packer* p, size_t* bytes) {
    if (!p || !bytes) return RSPT_HIP_ERR_ARG;
    *bytes = (size_t)p->g.nch * sizeof(IirCarry);
    return RSPT_HIP_OK;
}

int rspt_hip_iir_prefilter_stream_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, size_t nr_coefficients,
                                      int init_nr_samples, void* d_state, void* stream) {
    if (!d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    return iir_call(p, d_buf, nblocks, n, d, nr_coefficients, init_nr_samples, 0, d_state, stream);
}

int rspt_hip_iir_prefilter_planar_batch_dev(rspt_hip_packer* p, int32_t* d_planar, size_t nblocks, const double* n, const double* d,
                                            size_t nr_coefficients, int init_nr_samples, int per_channel, void* stream) {
    return iir_call(p, d_planar, nblocks, n, d, nr_coefficients, init_nr_samples, per_channel, nullptr, stream, true);
}

int rspt_hip_iir_prefilter_planar_stream_dev(rspt_hip_packer* p, int32_t* d_planar, size_t nblocks, const double* n, const double* d,
                                             size_t nr_coefficients, int init_nr_samples, void* d_state, void* stream) {
    if (!d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    return iir_call(p, d_planar, nblocks, n, d, nr_coefficients, init_nr_samples, 0, d_state, stream, true);
}

// ---- IIR cascade (iir_cascade.hip) ----
// One run of `ns` rows per (block, channel): the stateless call's nblocks blocks of g.ns rows, or (CARRY) the call's blocks as one
// block of nblocks * g.ns rows.  Whether a channel is fresh is known on the device only and the pipelined kernel starts from any
// init_nr_samples, so the route depends on the run's length alone.
template <int BPS, bool CARRY>
static void launch_iir_cascade(rspt_hip_packer* p, uint8_t* buf, uint32_t B, uint32_t ns, uint64_t block_bytes, const CascadeArgs& a, IirCarry* state,
                               hipStream_t st) {
    const dim3 grid((B * p->g.nch + 63) / 64);
    if (ns >= kCascChunk) {
        const bool al = (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(buf) % BPS) == 0;  // (block_bytes is a multiple of BPS)
        auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(64 * casc_waves(a.nsec)), 0, st, buf, p->g.nch, ns, block_bytes, a, B, state); };
        if (al) go(&k_iir_cascade_pipe<BPS, (BPS == 4 || BPS == 2), CARRY>);
        else go(&k_iir_cascade_pipe<BPS, false, CARRY>);
        return;
    }
    hipLaunchKernelGGL((k_iir_cascade<BPS, CARRY>), grid, dim3(64), 0, st, buf, p->g.nch, ns, block_bytes, a, B, state);
}

// The planar entries: the same routes on the int32 matrix [B][nch][hns]; block_bytes is one block of it, and a carried call
// (B = 1 for the kernel) is one run of ns rows through ns / hns of them.
template <bool CARRY>
static void launch_iir_cascade_planar(rspt_hip_packer* p, int32_t* d_planar, uint32_t B, uint32_t ns, const CascadeArgs& a, IirCarry* state, hipStream_t st) {
    uint8_t* buf = reinterpret_cast<uint8_t*>(d_planar);
    const uint64_t block_bytes = (uint64_t)p->g.nch * p->g.ns * 4u;
    const dim3 grid((B * p->g.nch + 63) / 64);
    if (ns >= kCascChunk)
        hipLaunchKernelGGL((k_iir_cascade_pipe_planar<CARRY>), grid, dim3(64 * casc_waves(a.nsec)), 0, st, buf, p->g.nch, ns, block_bytes, a, B, state);
    else
        hipLaunchKernelGGL((k_iir_cascade_planar<CARRY>), grid, dim3(64), 0, st, buf, p->g.nch, ns, block_bytes, a, B, state);
}

// All four cascade entries: d_state == NULL is the stateless call on nblocks blocks, else the blocks are one run behind the
// state; planar: d_buf is the int32 matrix.
static int iir_cascade_call(rspt_hip_packer* p, void* d_buf, size_t nblocks, size_t nsections, const double* n, const double* d,
                            const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* d_state, void* stream,
                            bool planar = false) {
    if (!p || !d_buf || !n || !d || !nr_coefficients || !init_nr_samples || !batch_count_ok(p, nblocks)) return RSPT_HIP_ERR_ARG;
    if (planar && reinterpret_cast<uintptr_t>(d_buf) % 4) return RSPT_HIP_ERR_ARG;
    if (nsections < 1 || nsections > kCascMaxSections) return RSPT_HIP_ERR_ARG;
    CascadeArgs a{};
    a.nsec = (uint32_t)nsections;
    for (size_t k = 0; k < nsections; ++k) {
        const uint32_t nc = nr_coefficients[k];
        if (nc < 2 || nc > 5 || init_nr_samples[k] < 0 || init_nr_samples[k] > (1 << 28)) return RSPT_HIP_ERR_ARG;
        for (uint32_t i = 0; i < nc; ++i) {  // (places past nc_k are not read)
            a.s[k].n[i] = n[5 * k + i];
            a.s[k].d[i] = d[5 * k + i];
        }
        a.s[k].nc = nc;
        a.s[k].init_steps = 4 * init_nr_samples[k];
        if (use_filter && use_filter[k]) a.use_filter |= 1u << k;
    }
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    const uint64_t rows = (uint64_t)nblocks * p->g.ns;
    if (d_state && rows >= kStreamMaxRows) return RSPT_HIP_ERR_UNSUPPORTED;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    if (planar) {
        if (d_state) launch_iir_cascade_planar<true>(p, (int32_t*)d_buf, 1u, (uint32_t)rows, a, (IirCarry*)d_state, st);
        else launch_iir_cascade_planar<false>(p, (int32_t*)d_buf, (uint32_t)nblocks, p->g.ns, a, nullptr, st);
        HIPCHK(p, hipGetLastError());
        return RSPT_HIP_OK;
    }
    by_bps(p->g.bps, [&](auto bps) {
        constexpr int BPS = decltype(bps)::value;
        if (d_state) launch_iir_cascade<BPS, true>(p, (uint8_t*)d_buf, 1u, (uint32_t)rows, rows * p->g.nch * BPS, a, (IirCarry*)d_state, st);
        else launch_iir_cascade<BPS, false>(p, (uint8_t*)d_buf, (uint32_t)nblocks, p->g.ns, (uint64_t)p->g.block_bytes, a, nullptr, st);
    });
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_iir_cascade_batch_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, size_t nsections, const double* n, const double* d,
                                   const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* stream) {
    return iir_cascade_call(p, d_buf, nblocks, nsections, n, d, nr_coefficients, init_nr_samples, use_filter, nullptr, stream);
}

int rspt_hip_iir_cascade_state_bytes(rspt_hip_packer* p, size_t nsections, size_t* bytes) {
    if (!p || !bytes || nsections < 1 || nsections > kCascMaxSections) return RSPT_HIP_ERR_ARG;
    *bytes = (size_t)p->g.nch * nsections * sizeof(IirCarry);
    return RSPT_HIP_OK;
}

int rspt_hip_iir_cascade_stream_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, size_t nsections, const double* n, const double* d,
                                    const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* d_state,
                                    void* stream) {
    if (!d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    return iir_cascade_call(p, d_buf, nblocks, nsections, n, d, nr_coefficients, init_nr_samples, use_filter, d_state, stream);
}

int rspt_hip_iir_cascade_planar_batch_dev(rspt_hip_packer* p, int32_t* d_planar, size_t nblocks, size_t nsections, const double* n, const double* d,
                                          const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* stream) {
    return iir_cascade_call(p, d_planar, nblocks, nsections, n, d, nr_coefficients, init_nr_samples, use_filter, nullptr, stream, true);
}

int rspt_hip_iir_cascade_planar_stream_dev(rspt_hip_packer* p, int32_t* d_planar, size_t nblocks, size_t nsections, const double* n, const double* d,
                                           const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* d_state,
                                           void* stream) {
    if (!d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    return iir_cascade_call(p, d_planar, nblocks, nsections, n, d, nr_coefficients, init_nr_samples, use_filter, d_state, stream, true);
}

// ---- zero-phase IIR (iir_zero_phase.hip) ----
// The workspace of a call: one slab double [ns][64] per wave of 64 (block, channel) lanes.  False where the byte count does not
// fit size_t.
static bool iir_zero_phase_bytes(const rspt_hip_packer* p, size_t nblocks, uint64_t* bytes) {
    const uint64_t slabs = ((uint64_t)nblocks * p->g.nch + 63) / 64;  // (batch_count_ok: below 2^25 + 1)
    const uint64_t per = (uint64_t)p->g.ns * 64 * sizeof(double);     // (ns < 2^31)
    if (slabs > (uint64_t)SIZE_MAX / per) return false;
    *bytes = slabs * per;
    return true;
}

// Blocks of a chunk and more whose forward history fills the ring's tail take the pipelined kernel, the others one thread per
// (block, channel): the one choice of both layouts.  PLANAR: src / dst are the int32 matrix [B][nch][ns] whatever the handle's
// bps (dst == src in place); native: one buffer, BPS the handle's.
template <int BPS, int NC, bool PLANAR>
static void launch_iir_zero_phase(rspt_hip_packer* p, uint8_t* src, uint8_t* dst, uint32_t B, const IirCoef& c, int init_nr_samples, int32_t back_steps,
                                  double* work, hipStream_t st) {
    const Geom& g = p->g;
    const dim3 grid((B * g.nch + 63) / 64);
    const bool pipe = g.ns >= kZpChunk && init_nr_samples >= NC - 1;
    if constexpr (PLANAR) {
        if (pipe)
            hipLaunchKernelGGL((k_iir_zp_pipe_planar<NC>), grid, dim3(kZpThreads), 0, st, src, dst, g.nch, g.ns, (uint64_t)g.nch * g.ns * 4u, c, back_steps, B, work);
        else
            hipLaunchKernelGGL((k_iir_zp_planar<NC>), grid, dim3(64), 0, st, (const int32_t*)src, (int32_t*)dst, g.ns, c, back_steps, B * g.nch, work);
    } else if (pipe) {
        const bool al = (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(src) % BPS) == 0;  // (block_bytes is a multiple of BPS)
        auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(kZpThreads), 0, st, src, g.nch, g.ns, (uint64_t)g.block_bytes, c, back_steps, B, work); };
        if (al) go(&k_iir_zp_pipe<BPS, NC, (BPS == 4 || BPS == 2)>);
        else go(&k_iir_zp_pipe<BPS, NC, false>);
    } else {
        hipLaunchKernelGGL((k_iir_zp<BPS, NC>), grid, dim3(64), 0, st, src, g.nch, g.ns, (uint64_t)g.block_bytes, c, back_steps, B, work);
    }
}

int rspt_hip_iir_zero_phase_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t* bytes) {
    if (!p || !bytes || !batch_count_ok(p, nblocks)) return RSPT_HIP_ERR_ARG;
    uint64_t n;
    if (!iir_zero_phase_bytes(p, nblocks, &n)) return RSPT_HIP_ERR_UNSUPPORTED;
    *bytes = (size_t)n;
    return RSPT_HIP_OK;
}

// Both zero-phase entries.  Native: d_src is the blocks' buffer and d_dst the same.  Planar: d_src is the int32 matrix and d_dst
// where the result goes -- the matrix itself, or one of its own that does not overlap it.
static int iir_zero_phase_call(rspt_hip_packer* p, void* d_src, void* d_dst, size_t nblocks, const double* n, const double* d, size_t nr_coefficients,
                               int init_nr_samples, int backward_init_nr_samples, void* d_work, size_t work_bytes, void* stream, bool planar) {
    if (!p || !d_src || !d_dst || !n || !d || !batch_count_ok(p, nblocks)) return RSPT_HIP_ERR_ARG;
    if (planar) {
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
        if (s0 % 4 || d0 % 4) return RSPT_HIP_ERR_ARG;
        const uint64_t bytes = (uint64_t)nblocks * p->g.nch * p->g.ns * sizeof(int32_t);  // (nblocks * nch < 2^31, ns < 2^31)
        if (s0 != d0 && s0 < d0 + bytes && d0 < s0 + bytes) return RSPT_HIP_ERR_ARG;  // the two matrices overlap without being the same
    }
    if (nr_coefficients < 2 || nr_coefficients > 5 || init_nr_samples < 0 || init_nr_samples > (1 << 28)) return RSPT_HIP_ERR_ARG;
    if (backward_init_nr_samples < 0 || backward_init_nr_samples > (1 << 28)) return RSPT_HIP_ERR_ARG;
    if (!d_work || reinterpret_cast<uintptr_t>(d_work) % 8) return RSPT_HIP_ERR_ARG;
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    uint64_t need;
    if (!iir_zero_phase_bytes(p, nblocks, &need)) return RSPT_HIP_ERR_UNSUPPORTED;
    if (work_bytes < need) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    IirCoef c{};
    for (size_t i = 0; i < nr_coefficients; ++i) {
        c.n[i] = n[i];
        c.d[i] = d[i];
    }
    c.nc = (uint32_t)nr_coefficients;
    c.init_steps = 4 * init_nr_samples;
    auto go = [&](auto bps, auto ncv, auto pl) {
        launch_iir_zero_phase<decltype(bps)::value, decltype(ncv)::value, decltype(pl)::value>(p, (uint8_t*)d_src, (uint8_t*)d_dst, (uint32_t)nblocks, c, init_nr_samples,
                                                                                               4 * backward_init_nr_samples, (double*)d_work, (hipStream_t)stream);
    };
    if (planar) by_nc(c.nc, [&](auto ncv) { go(std::integral_constant<int, 4>{}, ncv, std::true_type{}); });
    else by_bps(p->g.bps, [&](auto bps) { by_nc(c.nc, [&](auto ncv) { go(bps, ncv, std::false_type{}); }); });
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_iir_zero_phase_batch_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, size_t nr_coefficients,
                                      int init_nr_samples, int backward_init_nr_samples, void* d_work, size_t work_bytes, void* stream) {
    return iir_zero_phase_call(p, d_buf, d_buf, nblocks, n, d, nr_coefficients, init_nr_samples, backward_init_nr_samples, d_work, work_bytes, stream, false);
}

int rspt_hip_iir_zero_phase_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, int32_t* d_out, size_t nblocks, const double* n, const double* d,
                                             size_t nr_coefficients, int init_nr_samples, int backward_init_nr_samples, void* d_work, size_t work_bytes,
                                             void* stream) {
    int32_t* src = const_cast<int32_t*>(d_planar);  // (only read unless d_out is the matrix itself)
    return iir_zero_phase_call(p, src, d_out ? d_out : src, nblocks, n, d, nr_coefficients, init_nr_samples, backward_init_nr_samples, d_work, work_bytes, stream,
                               true);
}

// ---- the frame of the sliding-window stages (FIR, median), on the native block and on the planar int32 matrix ----
// How far a sliding-window stage splits the time axis: spans until there are about four workgroups per CU -- each span at least
// 4 (K - 1) samples, so that what an in-place call stages in front of its spans is at most a quarter of the batch, and a multiple
// of the chunk of C outputs.  base_units: the call's workgroups before any split; ns: the samples along the axis.
struct WinSplit {
    uint32_t span, nsplit;
};
static WinSplit win_split(int num_cu, uint64_t base_units, uint32_t ns, uint32_t K, uint32_t C) {
    const uint64_t want = 4ull * (uint64_t)num_cu;
    uint64_t nsplit = base_units >= want ? 1 : (want + base_units - 1) / base_units;
    const uint64_t min_span = K > 1 ? 4ull * (K - 1) : 1;
    const uint64_t max_split = ns / (min_span > C ? min_span : C);
    nsplit = nsplit > max_split ? max_split : nsplit;
    nsplit = nsplit < 1 ? 1 : nsplit;
    const uint64_t span = ((ns + nsplit - 1) / nsplit + C - 1) / C * C;
    return {(uint32_t)span, (uint32_t)((ns + span - 1) / span)};
}

// The decomposition on the native block (WinGeom): channel groups of up to `threads` lanes' channels, runs of `run` outputs per
// lane (kFirThreads / kFirR, kMedThreads / kMedRun), and spans of rows (win_split).  run_rows != 0 (a carried-state call): the
// nblocks blocks, back to back, taken as ONE block of run_rows = nblocks * ns rows.
static WinGeom win_geom(const rspt_hip_packer* p, size_t nblocks, uint32_t K, uint32_t threads, uint32_t run, uint32_t run_rows = 0) {
    Geom g = p->g;
    if (run_rows) {
        g.ns = run_rows;
        g.block_bytes = (uint64_t)run_rows * g.nch * g.bps;
        nblocks = 1;
    }
    WinGeom f{};
    f.block_bytes = g.block_bytes;
    f.stride = g.nch * g.bps;  // (window_call_checks checks the chunk's row offsets before a launch)
    f.nch = g.nch;
    f.ns = g.ns;
    f.K = K;
    f.cw = g.nch < threads ? g.nch : threads;
    f.subs = threads / f.cw;
    f.ncg = (g.nch + f.cw - 1) / f.cw;
    const uint64_t base_units = (uint64_t)nblocks * f.ncg;
    const WinSplit s = win_split(p->num_cu, base_units, g.ns, K, f.subs * run);
    f.span = s.span;
    f.nsplit = s.nsplit;
    f.units = base_units * f.nsplit;
    return f;
}

// The decomposition on the matrix (PlanarWin): a row = (block, channel) of ns samples, `lanes` lanes of `run` outputs along it --
// the smallest power of two that covers the row, at most `threads` --, threads / lanes rows to a workgroup, and spans of samples
// (win_split).  Only rows of more than one chunk are ever split.  `min_lanes` (a power of two) bounds the rows of a workgroup for
// a kernel that keeps something per row.
static PlanarWin planar_win(const rspt_hip_packer* p, size_t nblocks, uint32_t K, uint32_t threads, uint32_t run, bool in_place, bool carried,
                            uint32_t min_lanes) {
    const Geom& g = p->g;
    PlanarWin f{};
    f.rows = (uint64_t)nblocks * g.nch;
    f.total = f.rows * g.ns;
    f.nch = g.nch;
    f.ns = g.ns;
    f.K = K;
    const uint64_t runs = ((uint64_t)g.ns + run - 1) / run;
    f.lanes = min_lanes;
    while (f.lanes < threads && f.lanes < runs) f.lanes *= 2;
    f.rpw = threads / f.lanes;
    const uint64_t groups = (f.rows + f.rpw - 1) / f.rpw;
    const WinSplit s = win_split(p->num_cu, groups, g.ns, K, f.lanes * run);
    f.span = s.span;
    f.nsplit = s.nsplit;
    f.units = groups * f.nsplit;
    f.in_place = in_place;
    f.carried = carried;
    f.npiece = (in_place ? f.nsplit - 1 : 0u) + (carried ? 1u : 0u);
    return f;
}

// A windowed call that passed its checks: whether it is in place, and its decomposition in its layout's form (the other stays zero).
struct WinCall {
    bool in_place;
    WinGeom f;     // native
    PlanarWin pf;  // planar
};

// The checks of all eight windowed entry points (FIR and median, native and planar, stateless and carried), in the order they
// return.  ERR_ARG: a null handle or buffer, nblocks == 0 or nblocks * nch >= 2^31, a planar buffer off its 4-byte alignment,
// and buffers that overlap without being the same.  Then ERR_UNSUPPORTED: a handle too wide; rows that the kernels index in 32
// bits with a chunk's reach beyond the last one -- a carried call's run of nblocks * ns rows in either layout, a row of ns samples
// of a stateless call on the matrix --; and on the native block a chunk's row offsets, which k_fir and k_med_short compute in 32
// bits (2^24 channels and more).  Sets the decomposition for the window K; min_lanes: planar_win's.
static int window_call_checks(const rspt_hip_packer* p, bool planar, const void* d_src, const void* d_dst, size_t nblocks, bool carried, uint32_t K,
                              uint32_t threads, uint32_t run, WinCall* w, uint32_t min_lanes = 1) {
    if (!p || !d_src || !d_dst || !batch_count_ok(p, nblocks)) return RSPT_HIP_ERR_ARG;
    const Geom& g = p->g;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
    if (planar && (s0 % 4 || d0 % 4)) return RSPT_HIP_ERR_ARG;
    const uint64_t bytes = (uint64_t)nblocks * (planar ? (uint64_t)g.nch * g.ns * 4u : g.block_bytes);
    *w = WinCall{};
    w->in_place = s0 == d0;
    if (!w->in_place && s0 < d0 + bytes && d0 < s0 + bytes) return RSPT_HIP_ERR_ARG;  // in place, or apart
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    const uint64_t run_rows = (uint64_t)nblocks * g.ns;
    if ((carried ? run_rows : planar ? (uint64_t)g.ns : 0) >= kStreamMaxRows) return RSPT_HIP_ERR_UNSUPPORTED;
    if (planar) {
        w->pf = planar_win(p, nblocks, K, threads, run, w->in_place, carried, min_lanes);
        return RSPT_HIP_OK;
    }
    w->f = win_geom(p, nblocks, K, threads, run, carried ? (uint32_t)run_rows : 0u);
    if ((uint64_t)w->f.subs * run * w->f.stride >= (1ull << 31)) return RSPT_HIP_ERR_UNSUPPORTED;
    return RSPT_HIP_OK;
}

// The grid of a mover of n elements: 256 to a workgroup, at most 4096 workgroups (the movers stride by their grid).
static dim3 mover_grid(uint64_t n) { return dim3((uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 4096)); }

// A carried state of either stage in either layout: a u64 header, then K - 1 rows of nch samples, to a multiple of 8 bytes.
static size_t window_state_bytes(const rspt_hip_packer* p, size_t K, bool planar) {
    return 8 + (((K - 1) * p->g.nch * (planar ? 4u : p->g.bps) + 7) & ~(size_t)7);
}

// The halo of an in-place call with more than one span per block: the K - 1 rows in front of every span but the first,
// nblocks (nsplit - 1) pieces of (K - 1) rows.
static uint64_t halo_pieces(const WinGeom& f, size_t nblocks, bool in_place) {
    return in_place && f.nsplit > 1 ? (uint64_t)nblocks * (f.nsplit - 1) : 0;  // (a carried-state call: one block)
}

static hipError_t launch_halo(const WinGeom& f, const void* d_src, uint8_t* halo, uint64_t pieces, hipStream_t st) {
    const bool words = (reinterpret_cast<uintptr_t>(d_src) % 4) == 0 && (f.block_bytes % 4) == 0 && (f.stride % 4) == 0;
    const uint32_t grid = (uint32_t)(pieces < 65536 ? pieces : 65536);
    if (words) hipLaunchKernelGGL(k_fir_halo<true>, dim3(grid), dim3(256), 0, st, (const uint8_t*)d_src, halo, f, pieces);
    else hipLaunchKernelGGL(k_fir_halo<false>, dim3(grid), dim3(256), 0, st, (const uint8_t*)d_src, halo, f, pieces);
    return hipGetLastError();
}

// The end of a windowed call from the point where it has enqueued work: record `last` behind it, and report the first error.
static int finish_window_call(rspt_hip_packer* p, LastCall& last, hipError_t e, hipStream_t st) {
    const hipError_t er = last.record(st);
    if (e == hipSuccess) e = er;
    if (e != hipSuccess) {
        p->last_hip_error = (int)e;
        return RSPT_HIP_ERR_LAUNCH;
    }
    return RSPT_HIP_OK;
}

// ---- FIR pre-filter (fir.hip; on the matrix fir_planar.hip) ----
template <int BPS>
static void launch_fir(const WinGeom& f, const uint8_t* src, uint8_t* dst, const uint8_t* halo, const double* coef, bool aligned, hipStream_t st,
                       const uint8_t* head = nullptr) {
    const uint32_t grid = (uint32_t)(f.units < (1u << 20) ? f.units : (1u << 20));
    if (aligned) hipLaunchKernelGGL((k_fir<BPS, (BPS == 4 || BPS == 2)>), dim3(grid), dim3(kFirThreads), 0, st, src, dst, halo, coef, f, head);
    else hipLaunchKernelGGL((k_fir<BPS, false>), dim3(grid), dim3(kFirThreads), 0, st, src, dst, halo, coef, f, head);
}

// Stage the head of a carried-state call and write the new state (k_fir_carry, fir.hip); the state: [u64 started][K - 1 rows].
static hipError_t launch_fir_carry(const WinGeom& f, const void* d_src, uint8_t* head, void* d_state, hipStream_t st) {
    uint64_t* started = (uint64_t*)d_state;
    uint8_t* rows = (uint8_t*)d_state + 8;
    const uint64_t n = (uint64_t)(f.K - 1) * f.stride;
    if (n) hipLaunchKernelGGL(k_fir_carry<false>, mover_grid(n), dim3(256), 0, st, (const uint8_t*)d_src, head, started, rows, n, f.stride, f.K, f.ns);
    hipLaunchKernelGGL(k_fir_carry<true>, mover_grid(n), dim3(256), 0, st, (const uint8_t*)d_src, head, started, rows, n, f.stride, f.K, f.ns);
    return hipGetLastError();
}

// What a native call enqueues behind its coefficients: the carry movers, the halo (`pieces` of it), k_fir.
static hipError_t launch_fir_native(rspt_hip_packer* p, const WinGeom& f, const void* d_src, void* d_dst, uint64_t pieces, const double* coef,
                                    void* d_state, hipStream_t st) {
    FirStage& fs = p->fir;
    hipError_t e = d_state ? launch_fir_carry(f, d_src, fs.head, d_state, st) : hipSuccess;
    if (e == hipSuccess && pieces) e = launch_halo(f, d_src, fs.halo, pieces, st);
    if (e != hipSuccess) return e;
    const bool aligned = native_aligned(p->g.bps, d_src, d_dst);
    by_bps(p->g.bps, [&](auto b) {
        launch_fir<decltype(b)::value>(f, (const uint8_t*)d_src, (uint8_t*)d_dst, pieces ? (const uint8_t*)fs.halo : nullptr, coef, aligned, st,
                                       d_state && f.K > 1 ? (const uint8_t*)fs.head : nullptr);
    });
    return hipGetLastError();
}

// What a planar call enqueues behind its coefficients: the state's movers (head_n samples of the head), the fronts (front_n
// samples in the handle's `halo`), k_fir_planar.  N: the samples per channel of a carried call's run.
static hipError_t launch_fir_planar(rspt_hip_packer* p, const PlanarWin& f, const int32_t* d_src, int32_t* d_dst, uint64_t front_n, const double* coef,
                                    void* d_state, uint64_t N, hipStream_t st) {
    FirStage& fs = p->fir;
    int32_t* head = reinterpret_cast<int32_t*>((uint8_t*)fs.head);
    int32_t* front = reinterpret_cast<int32_t*>((uint8_t*)fs.halo);
    if (d_state) {
        uint64_t* started = (uint64_t*)d_state;
        int32_t* rows = reinterpret_cast<int32_t*>((uint8_t*)d_state + 8);
        const uint64_t head_n = (uint64_t)(f.K - 1) * f.nch;
        if (head_n) hipLaunchKernelGGL(k_firp_head, mover_grid(head_n), dim3(256), 0, st, d_src, head, started, rows, head_n, f.nch, f.ns);
        hipLaunchKernelGGL(k_firp_save, mover_grid(head_n), dim3(256), 0, st, d_src, head, started, rows, head_n, f.nch, f.ns, f.K, N);
        if (hipError_t e = hipGetLastError()) return e;
    }
    if (front_n) {
        hipLaunchKernelGGL(k_firp_front, mover_grid(front_n), dim3(256), 0, st, d_src, head, front, f);
        if (hipError_t e = hipGetLastError()) return e;
    }
    const uint32_t grid = (uint32_t)(f.units < (1u << 20) ? f.units : (1u << 20));
    const bool wide = reinterpret_cast<uintptr_t>(d_src) % 16 == 0 && reinterpret_cast<uintptr_t>(d_dst) % 16 == 0 && f.ns % 4 == 0;
    if (wide) hipLaunchKernelGGL(k_fir_planar<true>, dim3(grid), dim3(kFirThreads), 0, st, d_src, d_dst, front, coef, f);
    else hipLaunchKernelGGL(k_fir_planar<false>, dim3(grid), dim3(kFirThreads), 0, st, d_src, d_dst, front, coef, f);
    return hipGetLastError();
}

// What every FIR call does before it enqueues: grow the handle's staging buffers (`halo`, `head`) behind the stage's earlier
// calls, and copy the coefficients into the next slot -- the host waits only when kSlots calls are still ahead on the device.
// From RSPT_HIP_OK on every path of the caller ends in finish_window_call on (*slot)->last: the copy that the caller enqueues
// reads the page-locked slot.
static int fir_take_slot(rspt_hip_packer* p, const double* kernel, size_t kernel_size, uint64_t halo_bytes, uint64_t head_bytes,
                         FirStage::CoefSlot** slot) {
    FirStage& fs = p->fir;
    if (halo_bytes > fs.halo.cap || head_bytes > fs.head.cap) {
        fs.wait_all();  // (no earlier call may still read a buffer being replaced)
        if (halo_bytes > fs.halo.cap && fs.halo.grow(halo_bytes)) return RSPT_HIP_ERR_ALLOC;
        if (head_bytes > fs.head.cap && fs.head.grow(head_bytes)) return RSPT_HIP_ERR_ALLOC;
    }
    FirStage::CoefSlot& cs = fs.slot[fs.next];
    HIPCHK(p, cs.last.wait());
    if (cs.cap < kernel_size) {
        cs.cap = 0;
        if (hipHostMalloc((void**)cs.host.out(), kernel_size * sizeof(double), hipHostMallocDefault) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
        if (hipMalloc(cs.dev.out(), kernel_size * sizeof(double)) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
        cs.cap = kernel_size;
    }
    if (!cs.last.make_event()) return RSPT_HIP_ERR_ALLOC;
    memcpy(cs.host, kernel, kernel_size * sizeof(double));
    fs.next = (fs.next + 1) % FirStage::kSlots;
    *slot = &cs;
    return RSPT_HIP_OK;
}

// All four FIR entries: d_state == NULL is the stateless call on nblocks blocks, else the blocks are one run behind the state;
// planar: the buffers are int32 matrices, and the blocks of a carried call consecutive pieces of one recording.  The handle's
// `halo` holds what is staged in front of the spans -- native, the halo's pieces of K - 1 rows; planar, the fronts of K - 1 samples
// per row and piece -- and `head` the staged state, K - 1 rows of nch samples.
static int fir_call(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, const double* kernel, size_t kernel_size, void* d_state,
                    void* stream, bool planar = false) {
    if (!kernel || kernel_size == 0 || kernel_size > kFirMaxTaps) return RSPT_HIP_ERR_ARG;
    const uint32_t K = (uint32_t)kernel_size;
    WinCall w;
    if (int rc = window_call_checks(p, planar, d_src, d_dst, nblocks, d_state != nullptr, K, kFirThreads, kFirR, &w)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const uint64_t row_bytes = (uint64_t)p->g.nch * (planar ? 4u : p->g.bps);  // nch samples
    const uint64_t pieces = planar ? w.pf.rows * w.pf.npiece : halo_pieces(w.f, d_state ? 1 : nblocks, w.in_place);
    const uint64_t halo_bytes = pieces * (uint64_t)(K - 1) * (planar ? 4u : row_bytes);
    const uint64_t head_bytes = d_state ? (uint64_t)(K - 1) * row_bytes : 0;
    FirStage::CoefSlot* slot;
    if (int rc = fir_take_slot(p, kernel, kernel_size, halo_bytes, head_bytes, &slot)) return rc;
    FirStage::CoefSlot& cs = *slot;
    hipError_t e = hipMemcpyAsync(cs.dev, cs.host, kernel_size * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = planar ? launch_fir_planar(p, w.pf, (const int32_t*)d_src, (int32_t*)d_dst, pieces * (uint64_t)(K - 1), cs.dev, d_state,
                                       (uint64_t)nblocks * p->g.ns, st)
                   : launch_fir_native(p, w.f, d_src, d_dst, pieces, cs.dev, d_state, st);
    return finish_window_call(p, cs.last, e, st);
}

int rspt_hip_fir_prefilter_batch_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, const double* kernel, size_t kernel_size,
                                     void* stream) {
    return fir_call(p, d_src, d_dst, nblocks, kernel, kernel_size, nullptr, stream);
}

static int fir_state_bytes(rspt_hip_packer* p, size_t kernel_size, size_t* bytes, bool planar) {
    if (!p || !bytes || kernel_size == 0 || kernel_size > kFirMaxTaps) return RSPT_HIP_ERR_ARG;
    *bytes = window_state_bytes(p, kernel_size, planar);
    return RSPT_HIP_OK;
}

int rspt_hip_fir_state_bytes(rspt_hip_packer* p, size_t kernel_size, size_t* bytes) { return fir_state_bytes(p, kernel_size, bytes, false); }

int rspt_hip_fir_prefilter_stream_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, const double* kernel, size_t kernel_size,
                                      void* d_state, void* stream) {
    if (!d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    return fir_call(p, d_src, d_dst, nblocks, kernel, kernel_size, d_state, stream);
}

int rspt_hip_fir_prefilter_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, const double* kernel,
                                            size_t kernel_size, void* stream) {
    return fir_call(p, d_src, d_dst, nblocks, kernel, kernel_size, nullptr, stream, true);
}

int rspt_hip_fir_planar_state_bytes(rspt_hip_packer* p, size_t kernel_size, size_t* bytes) { return fir_state_bytes(p, kernel_size, bytes, true); }

int rspt_hip_fir_prefilter_planar_stream_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, const double* kernel,
                                             size_t kernel_size, void* d_state, void* stream) {
    if (!d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    return fir_call(p, d_src, d_dst, nblocks, kernel, kernel_size, d_state, stream, true);
}

// ---- rolling median (median.hip; on the matrix median_planar.hip) ----
template <uint32_t N, int BPS, bool HEAD>
static void launch_med_short(const WinGeom& f, const uint8_t* src, uint8_t* dst, const uint8_t* halo, bool aligned, hipStream_t st, const uint8_t* head) {
    const uint32_t grid = (uint32_t)(f.units < (1u << 20) ? f.units : (1u << 20));
    if (aligned) hipLaunchKernelGGL((k_med_short<N, BPS, (BPS == 4 || BPS == 2), HEAD>), dim3(grid), dim3(kMedThreads), 0, st, src, dst, halo, f, head);
    else hipLaunchKernelGGL((k_med_short<N, BPS, false, HEAD>), dim3(grid), dim3(kMedThreads), 0, st, src, dst, halo, f, head);
}

// k_med_short by its register bucket: the smallest of 4, 8, 16, 32 that holds W.
template <bool HEAD>
static hipError_t launch_med_short_w(uint32_t bps, const WinGeom& f, const void* d_src, void* d_dst, const uint8_t* halo, bool aligned, hipStream_t st,
                                     const uint8_t* head) {
    const uint32_t W = f.K;
    by_bps(bps, [&](auto bb) {
        constexpr int B = decltype(bb)::value;
        if (W <= 4) launch_med_short<4, B, HEAD>(f, (const uint8_t*)d_src, (uint8_t*)d_dst, halo, aligned, st, head);
        else if (W <= 8) launch_med_short<8, B, HEAD>(f, (const uint8_t*)d_src, (uint8_t*)d_dst, halo, aligned, st, head);
        else if (W <= 16) launch_med_short<16, B, HEAD>(f, (const uint8_t*)d_src, (uint8_t*)d_dst, halo, aligned, st, head);
        else launch_med_short<32, B, HEAD>(f, (const uint8_t*)d_src, (uint8_t*)d_dst, halo, aligned, st, head);
    });
    return hipGetLastError();
}

// The generic path on the pairs [pair0, pair0 + npairs) of the batch: sort (tile sort, merge passes), then walk.  STREAM: a pair
// is a (segment, channel) of a carried-state call and f.ns the segment capacity (median.hip).  BPS = kMedPlanar: the carried call
// on the planar matrix, through k_medp_tile_sort / k_medp_walk (median_planar.hip).
template <int BPS, bool STREAM = false>
static hipError_t launch_med_generic(rspt_hip_packer* p, const WinGeom& f, const uint8_t* src, uint8_t* dst, uint64_t pair0, uint64_t npairs,
                                     bool aligned, hipStream_t st, const MedSeg& sg = MedSeg{}) {
    MedianStage& ms = p->med;
    const uint32_t ns = f.ns;
    const uint32_t tiles = (ns + kMedTile - 1) / kMedTile;
    uint64_t* a = ms.keys_a;
    uint64_t* b = ms.keys_b;
    uint32_t* rank = ms.rank;
    const bool one_tile = tiles == 1;
    if constexpr (BPS == kMedPlanar)
        hipLaunchKernelGGL(k_medp_tile_sort, dim3((uint32_t)(npairs * tiles)), dim3(kMedThreads), 0, st, src, a, one_tile ? rank : nullptr, f, pair0, sg);
    else if (aligned) hipLaunchKernelGGL((k_med_tile_sort<BPS, (BPS == 4 || BPS == 2), STREAM>), dim3((uint32_t)(npairs * tiles)), dim3(kMedThreads), 0, st, src,
                                    a, one_tile ? rank : nullptr, f, pair0, sg);
    else hipLaunchKernelGGL((k_med_tile_sort<BPS, false, STREAM>), dim3((uint32_t)(npairs * tiles)), dim3(kMedThreads), 0, st, src, a,
                            one_tile ? rank : nullptr, f, pair0, sg);
    hipError_t e = hipGetLastError();
    const uint64_t total = npairs * ns;
    for (uint32_t width = kMedTile; e == hipSuccess && width < ns; width *= 2) {
        const bool last = (uint64_t)width * 2 >= ns;
        hipLaunchKernelGGL(k_med_merge, dim3((uint32_t)((total + kMedThreads - 1) / kMedThreads)), dim3(kMedThreads), 0, st, a, b, last ? rank : nullptr, ns,
                           width, total);
        e = hipGetLastError();
        std::swap(a, b);
    }
    if (e != hipSuccess) return e;
    const uint32_t spans = ((STREAM ? sg.L : ns) + kMedSpan - 1) / kMedSpan;
    const uint32_t n0 = (ns + 31) / 32;
    const size_t lds = (size_t)(n0 + (n0 + 31) / 32) * sizeof(uint32_t);
    if constexpr (BPS == kMedPlanar) hipLaunchKernelGGL(k_medp_walk, dim3((uint32_t)(npairs * spans)), dim3(64), lds, st, a, rank, dst, f, pair0, sg);
    else if (aligned) hipLaunchKernelGGL((k_med_walk<BPS, (BPS == 4 || BPS == 2), STREAM>), dim3((uint32_t)(npairs * spans)), dim3(64), lds, st, a, rank, dst, f,
                                    pair0, sg);
    else hipLaunchKernelGGL((k_med_walk<BPS, false, STREAM>), dim3((uint32_t)(npairs * spans)), dim3(64), lds, st, a, rank, dst, f, pair0, sg);
    return hipGetLastError();
}

// The median stage's buffers for a call: each grows behind the stage's last call, and `last` has its event from here on.
static int median_reserve(MedianStage& ms, uint64_t halo_bytes, uint64_t head_bytes, uint64_t key_samples) {
    if (halo_bytes > ms.halo.cap || head_bytes > ms.head.cap || key_samples > ms.key_cap) {
        ms.last.wait();  // (no earlier call may still use a buffer being replaced)
        if (halo_bytes > ms.halo.cap && ms.halo.grow(halo_bytes)) return RSPT_HIP_ERR_ALLOC;
        if (head_bytes > ms.head.cap && ms.head.grow(head_bytes)) return RSPT_HIP_ERR_ALLOC;
        if (key_samples > ms.key_cap) {
            ms.key_cap = 0;
            ms.rank.reset();
            ms.keys_b.reset();
            if (hipMalloc(ms.keys_a.out(), key_samples * sizeof(uint64_t)) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
            if (hipMalloc(ms.keys_b.out(), key_samples * sizeof(uint64_t)) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
            if (hipMalloc(ms.rank.out(), key_samples * sizeof(uint32_t)) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
            ms.key_cap = key_samples;
        }
    }
    return ms.last.make_event() ? RSPT_HIP_OK : RSPT_HIP_ERR_ALLOC;
}

static int median_state_bytes(rspt_hip_packer* p, size_t window, size_t* bytes, bool planar) {
    if (!p || !bytes || window == 0) return RSPT_HIP_ERR_ARG;
    if (window > kMedShortMax && window - 1 > kMedMaxCarry) return RSPT_HIP_ERR_UNSUPPORTED;
    *bytes = window_state_bytes(p, window, planar);
    return RSPT_HIP_OK;
}

// Stage the old state in the handle's head buffer and write the new one (k_med_carry, median.hip): in words where every
// address and length is a multiple of 4.
static hipError_t launch_med_carry(const WinGeom& f, const void* d_src, uint8_t* head, void* d_state, uint64_t rows, hipStream_t st) {
    uint64_t n = (uint64_t)(f.K - 1) * f.stride, call = rows * f.stride;
    const bool words = reinterpret_cast<uintptr_t>(d_src) % 4 == 0 && f.stride % 4 == 0;
    if (words) n /= 4, call /= 4;
    const dim3 grid = mover_grid(n);
    uint8_t* state = (uint8_t*)d_state;
    if (words) {
        hipLaunchKernelGGL((k_med_carry<false, uint32_t>), grid, dim3(256), 0, st, (const uint32_t*)d_src, head, state, n, call, f.K - 1, rows);
        hipLaunchKernelGGL((k_med_carry<true, uint32_t>), grid, dim3(256), 0, st, (const uint32_t*)d_src, head, state, n, call, f.K - 1, rows);
    } else {
        hipLaunchKernelGGL((k_med_carry<false, uint8_t>), grid, dim3(256), 0, st, (const uint8_t*)d_src, head, state, n, call, f.K - 1, rows);
        hipLaunchKernelGGL((k_med_carry<true, uint8_t>), grid, dim3(256), 0, st, (const uint8_t*)d_src, head, state, n, call, f.K - 1, rows);
    }
    return hipGetLastError();
}

// The segment capacity S = W - 1 + L of a carried-state call of the generic path: 8 (W - 1) rounded up to 2^16, 2^17 or 2^18 --
// at most one row in eight is sorted twice up to W - 1 = 2^15, one in two at the limit W - 1 = 2^17 -- and never more than the
// call needs (one segment of W - 1 + N rows).  2^16 is the channel length the stateless path is measured at:
// shorter segments save merge passes but pay a bitmap clear and W set bits per 1024 outputs more often than they save.
static uint32_t median_segment_rows(uint32_t W, uint64_t rows) {
    const uint64_t want = 8ull * (W - 1);
    const uint64_t S = want <= (1u << 16) ? (1u << 16) : want <= (1u << 17) ? (1u << 17) : kMedMaxRanks;
    return (uint32_t)std::min<uint64_t>(S, (uint64_t)(W - 1) + rows);
}

// The movers of a carried call on the matrix: stage the state as it is (k_med_carry<false>, in words), then gather the new one
// from the tails of the blocks' rows (k_medp_save).
static hipError_t launch_medp_carry(const PlanarWin& f, const int32_t* d_src, uint8_t* head, void* d_state, uint64_t rows, hipStream_t st) {
    const uint64_t wm1 = f.K - 1, head_n = wm1 * f.nch;  // samples of the staged state
    hipLaunchKernelGGL((k_med_carry<false, uint32_t>), mover_grid(head_n), dim3(256), 0, st, (const uint32_t*)d_src, head, (uint8_t*)d_state, head_n,
                       (uint64_t)0, wm1, rows);
    hipLaunchKernelGGL(k_medp_save, mover_grid(head_n), dim3(256), 0, st, d_src, (const uint8_t*)head, (uint8_t*)d_state, head_n, f.nch, f.ns, wm1, rows);
    return hipGetLastError();
}

template <uint32_t N>
static void launch_med_planar(const PlanarWin& f, const int32_t* src, int32_t* dst, const int32_t* front, bool wide, hipStream_t st, const uint8_t* head) {
    const uint32_t grid = (uint32_t)(f.units < (1u << 20) ? f.units : (1u << 20));
    if (wide) hipLaunchKernelGGL((k_med_planar<N, true>), dim3(grid), dim3(kMedThreads), 0, st, src, dst, front, f, head);
    else hipLaunchKernelGGL((k_med_planar<N, false>), dim3(grid), dim3(kMedThreads), 0, st, src, dst, front, f, head);
}

// The short path on the matrix: the fronts (front_n samples of them, k_firp_front), then k_med_planar by its register bucket.
// head: the staged state of a carried call, else null.
static hipError_t launch_med_short_planar(const PlanarWin& f, const int32_t* d_src, int32_t* d_dst, int32_t* front, uint64_t front_n, const uint8_t* head,
                                          hipStream_t st) {
    if (front_n) {
        hipLaunchKernelGGL(k_firp_front, mover_grid(front_n), dim3(256), 0, st, d_src, reinterpret_cast<const int32_t*>(head ? head + 8 : nullptr), front, f);
        if (hipError_t e = hipGetLastError()) return e;
    }
    const bool wide = reinterpret_cast<uintptr_t>(d_src) % 16 == 0 && reinterpret_cast<uintptr_t>(d_dst) % 16 == 0 && f.ns % 4 == 0;
    const uint32_t W = f.K;
    if (W <= 4) launch_med_planar<4>(f, d_src, d_dst, front, wide, st, head);
    else if (W <= 8) launch_med_planar<8>(f, d_src, d_dst, front, wide, st, head);
    else if (W <= 16) launch_med_planar<16>(f, d_src, d_dst, front, wide, st, head);
    else launch_med_planar<32>(f, d_src, d_dst, front, wide, st, head);
    return hipGetLastError();
}

// All four median entries: d_state == NULL is the stateless call on nblocks blocks, where a window of ns or more is the expanding
// median of the channel; else the blocks are one run behind the state, and the window is the recording's (not clamped to ns).
// planar: the buffers are int32 matrices, a stateless row = (block, channel) a fresh window, the blocks of a carried call
// consecutive pieces of one recording.  The handle's `halo` holds what the short path stages in front of its spans -- native, the
// halo's pieces of W - 1 rows; planar, the fronts of W - 1 samples per row and piece --, `head` the staged state.
static int median_call(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, size_t window, void* d_state, void* stream,
                       bool planar = false) {
    if (!p || window == 0) return RSPT_HIP_ERR_ARG;
    const Geom& g = p->g;
    const bool carried = d_state != nullptr;
    const uint32_t W = (uint32_t)std::min<size_t>(window, carried ? (size_t)kMedMaxCarry + 2 : g.ns);
    WinCall w;
    if (int rc = window_call_checks(p, planar, d_src, d_dst, nblocks, carried, W, kMedThreads, kMedRun, &w, kMedpMinLanes)) return rc;
    const bool is_short = W <= kMedShortMax;
    // (the generic path's bitmaps live in LDS; with a state, at least half of every segment is new rows)
    if (!is_short && (carried ? W - 1 > kMedMaxCarry : g.ns > kMedMaxRanks)) return RSPT_HIP_ERR_UNSUPPORTED;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const uint64_t rows = (uint64_t)nblocks * g.ns;         // of a carried call's run (below 2^31 - 2^17: window_call_checks)
    const uint32_t stride = g.nch * (planar ? 4u : g.bps);  // bytes of nch samples: a row of the native block, of a state
    if (W == 1) {  // a copy, sample width kept; a state is its header and stays zero
        if (w.in_place) return RSPT_HIP_OK;
        HIPCHK(p, hipMemcpyAsync(d_dst, d_src, rows * stride, hipMemcpyDeviceToDevice, st));
        return RSPT_HIP_OK;
    }
    MedianStage& ms = p->med;
    const uint32_t bps = g.bps;
    const bool aligned = planar || native_aligned(bps, d_src, d_dst);
    // buffers: what the short path stages in front of its spans, a state's staged copy, the generic path's keys and ranks
    const uint64_t pieces = !is_short ? 0 : planar ? w.pf.rows * w.pf.npiece : halo_pieces(w.f, carried ? 1 : nblocks, w.in_place);
    const uint64_t halo_bytes = pieces * (uint64_t)(W - 1) * (planar ? 4u : stride);
    const uint64_t head_bytes = carried ? 8 + (uint64_t)(W - 1) * stride : 0;
    // generic: (block, channel) items of ns keys -- with a state (segment, channel) items of S keys -- in pieces of up to 2^25 keys.
    // Its kernels read block_bytes, stride, nch, ns and K of a WinGeom and nothing else.  Native that is the block, or the run as
    // one block; on the matrix a stateless row is a block of one channel of 4-byte samples, and a carried call keeps the block of
    // the matrix (k_medp_tile_sort / k_medp_walk find a row of the run by med_planar_at).
    MedSeg sg{};
    WinGeom fg{};
    fg.nch = planar && !carried ? 1u : g.nch;
    fg.stride = planar ? fg.nch * 4u : stride;
    fg.block_bytes = planar ? (uint64_t)g.ns * fg.stride : w.f.block_bytes;
    fg.ns = g.ns;
    fg.K = W;
    uint64_t items = (uint64_t)nblocks * g.nch, piece_items = 0;
    if (!is_short) {
        if (carried) {
            fg.ns = median_segment_rows(W, rows);
            sg.L = fg.ns - (W - 1);
            sg.nseg = (uint32_t)((rows + sg.L - 1) / sg.L);
            sg.N = (uint32_t)rows;
            sg.bns = planar ? g.ns : 0u;
            items = (uint64_t)sg.nseg * g.nch;
        }
        piece_items = std::min<uint64_t>(items, std::max<uint64_t>(1, (1ull << 25) / fg.ns));
    }
    if (int rc = median_reserve(ms, halo_bytes, head_bytes, piece_items * fg.ns)) return rc;
    hipError_t e = hipSuccess;
    if (carried) {  // the state is staged and the new one written from d_src before any kernel stores to d_dst
        sg.head = ms.head;
        e = planar ? launch_medp_carry(w.pf, (const int32_t*)d_src, ms.head, d_state, rows, st) : launch_med_carry(w.f, d_src, ms.head, d_state, rows, st);
    }
    if (e != hipSuccess) return finish_window_call(p, ms.last, e, st);
    const uint8_t* head = carried ? (const uint8_t*)ms.head : nullptr;
    if (is_short && planar) {
        e = launch_med_short_planar(w.pf, (const int32_t*)d_src, (int32_t*)d_dst, reinterpret_cast<int32_t*>((uint8_t*)ms.halo), pieces * (uint64_t)(W - 1),
                                    head, st);
    } else if (is_short) {
        const uint8_t* halo = pieces ? (const uint8_t*)ms.halo : nullptr;
        if (pieces) e = launch_halo(w.f, d_src, ms.halo, pieces, st);
        if (e == hipSuccess)
            e = carried ? launch_med_short_w<true>(bps, w.f, d_src, d_dst, halo, aligned, st, head)
                        : launch_med_short_w<false>(bps, w.f, d_src, d_dst, halo, aligned, st, nullptr);
    } else {
        // (with a state from the last segment to the first: a walk writes its segment's new rows, which no segment sorted later reads)
        const uint8_t* src = (const uint8_t*)d_src;
        uint8_t* dst = (uint8_t*)d_dst;
        for (uint64_t item0 = 0; e == hipSuccess && item0 < items; item0 += piece_items) {
            const uint64_t ni = std::min(piece_items, items - item0);
            if (planar && carried) e = launch_med_generic<kMedPlanar, true>(p, fg, src, dst, item0, ni, true, st, sg);
            else
                e = by_bps(planar ? 4u : bps, [&](auto bb) {
                    constexpr int B = decltype(bb)::value;
                    return carried ? launch_med_generic<B, true>(p, fg, src, dst, item0, ni, aligned, st, sg)
                                   : launch_med_generic<B>(p, fg, src, dst, item0, ni, aligned, st);
                });
        }
    }
    return finish_window_call(p, ms.last, e, st);
}

int rspt_hip_median_filter_batch_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, size_t window, void* stream) {
    return median_call(p, d_src, d_dst, nblocks, window, nullptr, stream);
}

int rspt_hip_median_state_bytes(rspt_hip_packer* p, size_t window, size_t* bytes) { return median_state_bytes(p, window, bytes, false); }

int rspt_hip_median_filter_stream_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, size_t window, void* d_state, void* stream) {
    if (!d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    return median_call(p, d_src, d_dst, nblocks, window, d_state, stream);
}

int rspt_hip_median_filter_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, size_t window, void* stream) {
    return median_call(p, d_src, d_dst, nblocks, window, nullptr, stream, true);
}

int rspt_hip_median_planar_state_bytes(rspt_hip_packer* p, size_t window, size_t* bytes) { return median_state_bytes(p, window, bytes, true); }

int rspt_hip_median_filter_planar_stream_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, size_t window, void* d_state,
                                             void* stream) {
    if (!d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    return median_call(p, d_src, d_dst, nblocks, window, d_state, stream, true);
}

// ---- PRDN: the quality figure of the reference's harness (quality.hip) -----------------------------------------------------------
// The decomposition of the two streaming passes for the widest load the buffers' alignment allows.
static QGeom quality_geom(const rspt_hip_packer* p, size_t nblocks, int W) {
    const Geom& g = p->g;
    QGeom q{};
    q.block_bytes = g.block_bytes;
    q.nch = g.nch, q.ns = g.ns, q.be = g.be;
    const uint32_t nw = W == 0 ? 1u : (g.bps == 3 ? 3u : 1u) * (uint32_t)W;
    const uint32_t vs = W == 0 ? 1u : nw * 4u / g.bps;  // samples of a load group
    uint32_t a = g.nch, b = vs;
    while (b) {
        const uint32_t t = a % b;
        a = b, b = t;
    }
    q.rows = vs / a;  // the fewest rows that hold whole groups
    const uint64_t qps = (uint64_t)q.rows * g.nch / vs;
    q.qps = (uint32_t)qps;
    q.nsub = qps < kQThreads ? kQThreads / q.qps : 1u;
    q.ncg = (uint32_t)((qps + kQThreads - 1) / kQThreads);
    q.nsr = g.ns / q.rows;
    const uint64_t sweeps = ((uint64_t)q.nsr + q.nsub - 1) / q.nsub;
    // workgroups: about 4096 in all where the blocks are long enough to give each at least 8 sweeps
    uint64_t nsplit = std::min<uint64_t>(std::max<uint64_t>(1, sweeps / 8), (4096 + nblocks * q.ncg - 1) / (nblocks * q.ncg));
    q.span = (uint32_t)std::max<uint64_t>(1, (sweeps + nsplit - 1) / nsplit) * q.nsub;
    q.nsplit = (uint32_t)std::max<uint64_t>(1, ((uint64_t)q.nsr + q.span - 1) / q.span);
    return q;
}

// The refusals both PRDN entries share, in front of each entry's own.
static int prdn_checks(const rspt_hip_packer* p, const void* d_orig, const void* d_dec, size_t nblocks, const double* d_prdn) {
    if (!p || !d_orig || !d_dec || !d_prdn || !batch_count_ok(p, nblocks)) return RSPT_HIP_ERR_ARG;
    return p->feed ? RSPT_HIP_ERR_ARG : RSPT_HIP_OK;  // (the feed owns the handle's workspace until rspt_hip_feed_end)
}

// Both PRDN entries behind their refusals: the workspace, the zeroed scratch, then launch(s, st, false) -- the entry's streaming
// passes --, k_q_finish, and launch(s, st, true) -- the entry's sequential kernel, which reads the flags k_q_finish wrote.
template <class Launch>
static int prdn_call(rspt_hip_packer* p, size_t nblocks, double* d_prdn, double* d_mse, double* d_ref, uint32_t* d_path, void* stream, Launch&& launch) {
    if (int rc = rspt_hip_reserve(p, nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const uint32_t B = (uint32_t)nblocks;
    const QScratch s(p->ws.quality, B, p->g.nch);
    HIPCHK(p, hipMemsetAsync(s.sums, 0, s.clear_bytes, st));
    launch(s, st, false);
    hipLaunchKernelGGL(k_q_finish, dim3((B + 255) / 256), dim3(256), 0, st, (const unsigned long long*)s.acc, B, s.flag, d_prdn, d_mse, d_ref, d_path);
    launch(s, st, true);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_prdn_batch_dev(rspt_hip_packer* p, const void* d_orig, const void* d_dec, size_t nblocks, double* d_prdn, double* d_mse, double* d_ref,
                            uint32_t* d_path, void* stream) {
    if (int rc = prdn_checks(p, d_orig, d_dec, nblocks, d_prdn)) return rc;
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    const Geom& g = p->g;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_orig), d0 = reinterpret_cast<uintptr_t>(d_dec);
    auto aligned = [&](uintptr_t m) { return o0 % m == 0 && d0 % m == 0 && (nblocks == 1 || g.block_bytes % m == 0); };
    const int W = aligned(16) ? 4 : aligned(4) ? 1 : 0;
    QGeom q = quality_geom(p, nblocks, W);
    q.aligned4 = aligned(4) ? 1u : 0u;
    const uint64_t units = (uint64_t)nblocks * q.ncg * q.nsplit;
    if (units >= (1ull << 31) || (uint64_t)q.rows * g.nch >= (1ull << 32)) return RSPT_HIP_ERR_UNSUPPORTED;
    const uint8_t* o = (const uint8_t*)d_orig;
    const uint8_t* d = (const uint8_t*)d_dec;
    return prdn_call(p, nblocks, d_prdn, d_mse, d_ref, d_path, stream, [&](const QScratch& s, hipStream_t st, bool seq) {
        by_bps(g.bps, [&](auto bb) {
            constexpr int BPS = decltype(bb)::value;
            auto go = [&](auto ww) {
                constexpr int WW = decltype(ww)::value;
                hipLaunchKernelGGL((k_q_sums<BPS, WW>), dim3((uint32_t)units), dim3(kQThreads), 0, st, o, q, s.sums);
                hipLaunchKernelGGL((k_q_accum<BPS, WW>), dim3((uint32_t)units), dim3(kQThreads), 0, st, o, d, q, (const long long*)s.sums, s.acc);
            };
            if (seq)
                hipLaunchKernelGGL(k_q_seq<BPS>, dim3((uint32_t)nblocks), dim3(kQThreads), 0, st, o, d, q, (const long long*)s.sums,
                                   (const unsigned long long*)s.acc, (const uint32_t*)s.flag, d_prdn, d_mse, d_ref);
            else if (W == 4) go(std::integral_constant<int, 4>());
            else if (W == 1) go(std::integral_constant<int, 1>());
            else go(std::integral_constant<int, 0>());
        });
    });
}

// ---- PRDN on the planar int32 matrix (quality_planar.hip) -------------------------------------------------------------------------
// whole_rows: a unit is a whole row (k_qp_rows); else rows longer than a wave's are cut into spans of whole sweeps while the call
// has fewer than kQpUnits units and a span keeps kQpMinSweeps sweeps.
static QPGeom quality_planar_geom(const Geom& g, size_t nblocks, bool whole_rows) {
    QPGeom q{};
    q.rows = (uint64_t)nblocks * g.nch;
    q.nch = g.nch, q.ns = g.ns;
    q.lanes = g.ns <= kQpWaveRow ? (uint32_t)kWave : kQpThreads;
    q.span = g.ns, q.nsplit = 1;
    if (q.lanes == kQpThreads && !whole_rows) {
        const uint64_t sweeps = ((uint64_t)g.ns + kQpSweep - 1) / kQpSweep;
        const uint64_t nsplit = std::min<uint64_t>(std::max<uint64_t>(1, sweeps / kQpMinSweeps), (kQpUnits + q.rows - 1) / q.rows);
        const uint64_t span = (sweeps + nsplit - 1) / nsplit * kQpSweep;  // (at most ns rounded up to a sweep: below 2^32)
        if (span < g.ns) q.span = (uint32_t)span, q.nsplit = (uint32_t)(((uint64_t)g.ns + span - 1) / span);
    }
    return q;
}
static uint64_t quality_planar_units(const QPGeom& q) { return q.lanes == (uint32_t)kWave ? (q.rows + kQpWaves - 1) / kQpWaves : q.rows * q.nsplit; }

int rspt_hip_prdn_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_orig, const int32_t* d_dec, size_t nblocks, double* d_prdn, double* d_mse,
                                   double* d_ref, uint32_t* d_path, void* stream) {
    if (int rc = prdn_checks(p, d_orig, d_dec, nblocks, d_prdn)) return rc;
    if (p->g.kind == RSPT_HIP_KIND_BYTES) return RSPT_HIP_ERR_ARG;  // (a byte buffer has no samples)
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_orig), d0 = reinterpret_cast<uintptr_t>(d_dec);
    if ((o0 | d0) & 3u) return RSPT_HIP_ERR_ARG;
    const Geom& g = p->g;
    QPGeom q = quality_planar_geom(g, nblocks, true);
    bool fused = quality_planar_units(q) >= kQpFusedMinUnits && g.ns <= kQpFusedMaxNs;
    if (p->qp_form) fused = p->qp_form == 2;
    if (!fused) q = quality_planar_geom(g, nblocks, false);
    const uint64_t units = quality_planar_units(q);  // (below 2^31: at most the rows of the call, or about kQpUnits where rows are cut)
    return prdn_call(p, nblocks, d_prdn, d_mse, d_ref, d_path, stream, [&](const QScratch& s, hipStream_t st, bool seq) {
        const dim3 grid((uint32_t)units), wg(kQpThreads);
        if (seq) {
            hipLaunchKernelGGL(k_qp_seq, dim3((uint32_t)nblocks), dim3(kQThreads), 0, st, d_orig, d_dec, g.nch, g.ns, (const long long*)s.sums,
                               (const unsigned long long*)s.acc, (const uint32_t*)s.flag, d_prdn, d_mse, d_ref);
        } else if (fused) {
            if (g.ns <= (q.lanes == (uint32_t)kWave ? kQpWaveRow : kQpRowRegs))
                hipLaunchKernelGGL(k_qp_rows<true>, grid, wg, 0, st, d_orig, d_dec, q, (long long*)s.sums, s.acc);
            else hipLaunchKernelGGL(k_qp_rows<false>, grid, wg, 0, st, d_orig, d_dec, q, (long long*)s.sums, s.acc);
        } else {
            hipLaunchKernelGGL(k_qp_sums, grid, wg, 0, st, d_orig, q, s.sums);
            hipLaunchKernelGGL(k_qp_accum, grid, wg, 0, st, d_orig, d_dec, q, (const long long*)s.sums, s.acc);
        }
    });
}

// ---- native <-> planar int32 (the reference's convert_native_to_i32 / convert_i32_to_native, utils.cpp:51-191) -------------------
// The checks of both entries.  Nothing of the handle but its shape and byte order is used: no workspace, no allocation.
static int convert_checks(const rspt_hip_packer* p, const void* d_native, const void* d_planar, size_t nblocks) {
    if (!p || !d_native || !d_planar || nblocks > 65535 || !batch_count_ok(p, nblocks)) return RSPT_HIP_ERR_ARG;  // (65535: grid.z, as rspt_hip_reserve)
    const Geom& g = p->g;
    const uintptr_t n0 = reinterpret_cast<uintptr_t>(d_native), p0 = reinterpret_cast<uintptr_t>(d_planar);
    if (p0 & 3u) return RSPT_HIP_ERR_ARG;
    const uint64_t nbytes = (uint64_t)nblocks * g.block_bytes, pbytes = (uint64_t)nblocks * g.N * sizeof(int32_t);
    if (n0 < p0 + pbytes && p0 < n0 + nbytes) return RSPT_HIP_ERR_ARG;  // the two buffers overlap
    return RSPT_HIP_OK;
}

// Narrow handles with a 16-byte aligned native buffer take the tile kernels of the packers' own front end and inverse; wide ones,
// and native buffers at any other address, the 64 x 64 transposes k_wide_planar / k_wide_native.
static bool convert_i32x4_ok(const Geom& g, const void* d_planar) {
    return g.bps == 4 && (g.nch & 3) == 0 && (g.ns & 3) == 0 && g.nch <= 1024 && (reinterpret_cast<uintptr_t>(d_planar) & 15) == 0;
}

int rspt_hip_native_to_i32_batch_dev(rspt_hip_packer* p, const void* d_native, int32_t* d_planar, size_t nblocks, void* stream) {
    if (int rc = convert_checks(p, d_native, d_planar, nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    const Geom& g = p->g;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* src = (const uint8_t*)d_native;
    const unsigned B = (unsigned)nblocks;
    if (!p->wide && (reinterpret_cast<uintptr_t>(d_native) & 15) == 0) {
        if (convert_i32x4_ok(g, d_planar)) {
            const uint32_t T4 = tile_i32x4(g);
            hipLaunchKernelGGL(k_tile_planar_i32x4, dim3((g.ns + T4 - 1) / T4, B), dim3(256), g.nch * (T4 + 1) * 4, st, src, g, T4, d_planar,
                               (long long*)nullptr);
        } else {
            by_bps(g.bps, [&](auto bps) {
                constexpr int BPS = decltype(bps)::value;
                if (!p->conv_lds_raised) {  // (once per handle: a handle has one sample width)
                    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tile_planar<BPS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->in_lds) != hipSuccess) return;
                    p->conv_lds_raised = true;
                }
                hipLaunchKernelGGL((k_tile_planar<BPS>), dim3((g.ns + p->T - 1) / p->T, B), dim3(256), p->in_lds, st, src, g, p->T, d_planar);
            });
        }
    } else {
        by_bps(g.bps, [&](auto bps) {
            hipLaunchKernelGGL(k_wide_planar<decltype(bps)::value>, dim3((g.ns + 63) / 64, (g.nch + 63) / 64, B), dim3(256), 0, st, src, g, d_planar);
        });
    }
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_i32_to_native_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, void* d_native, size_t nblocks, void* stream) {
    if (int rc = convert_checks(p, d_native, d_planar, nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    const Geom& g = p->g;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* dst = (uint8_t*)d_native;
    const unsigned B = (unsigned)nblocks;
    // k_planar_native divides per element and stores int8 / int16 / int24 byte by byte: it keeps only the handles of fewer than 32
    // channels, where more than half of k_wide_native's 64-channel tile would be empty.
    const bool narrow = !p->wide && p->Tn_native && (reinterpret_cast<uintptr_t>(d_native) & 15) == 0;
    if (narrow && (convert_i32x4_ok(g, d_planar) || g.nch < 32)) {
        if (convert_i32x4_ok(g, d_planar)) {
            const uint32_t T4 = tile_i32x4(g);
            hipLaunchKernelGGL(k_planar_native_i32x4, dim3((g.ns + T4 - 1) / T4, B), dim3(256), g.nch * (T4 + 1) * 4, st, d_planar, g, T4, dst);
        } else {
            const uint32_t T = min(p->Tn_native, g.ns);
            by_bps(g.bps, [&](auto bps) {
                hipLaunchKernelGGL((k_planar_native<decltype(bps)::value>), dim3((g.ns + T - 1) / T, B), dim3(256), g.nch * (T + 1) * 4, st, d_planar, g, T,
                                   dst);
            });
        }
    } else {
        by_bps(g.bps, [&](auto bps) { launch_wide_native<decltype(bps)::value>(g, d_planar, dst, B, st); });
    }
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_design_iir(int type, int order, double sampling_rate, double cutoff_low, double cutoff_high, double* num, double* den,
                        size_t* nr_coefficients) {
    if (!num || !den || !nr_coefficients) return RSPT_HIP_ERR_ARG;
    double n[5], d[5];
    const int nc = design_iir(type, order, sampling_rate, cutoff_low, cutoff_high, n, d);
    if (nc == 0) return RSPT_HIP_ERR_ARG;
    for (int i = 0; i < nc; ++i) {
        num[i] = n[i];
        den[i] = d[i];
    }
    *nr_coefficients = (size_t)nc;
    return RSPT_HIP_OK;
}

// ---- R-peak detectors (peak.hip) ----
// The checks all four peak entries make, and the kernel arguments from them (all of PeakOffArgs but its workspace): false where
// an entry refuses the call.  planar: d_src is the int32 matrix [nblocks][nch][ns] (and the traces are matrices of that shape).
static bool peak_args(rspt_hip_packer* p, const void* d_src, size_t nblocks, double sampling_rate, void* d_state, uint32_t* d_count,
                      int32_t* d_index, double* d_value, size_t max_peaks, double* d_sig, double* d_threshold, PeakArgs& a, bool planar) {
    if (!p || !d_src || !d_count || !batch_count_ok(p, nblocks)) return false;
    if (planar && reinterpret_cast<uintptr_t>(d_src) % 4) return false;
    if (!std::isfinite(sampling_rate) || sampling_rate <= 0 || sampling_rate > (double)(1 << 20)) return false;
    if (max_peaks > 0 && (!d_index || !d_value)) return false;
    if ((uint64_t)max_peaks > (1ull << 32) || (!d_sig) != (!d_threshold)) return false;
    const Geom& g = p->g;
    a.src = (const uint8_t*)d_src;
    a.block_bytes = planar ? (uint64_t)g.N * sizeof(int32_t) : g.block_bytes;
    a.stride = planar ? (uint32_t)sizeof(int32_t) : g.nch * g.bps;
    a.nch = g.nch;
    a.ns = g.ns;
    a.nblocks = (uint32_t)nblocks;
    a.lanes = d_state ? g.nch : (uint32_t)(nblocks * g.nch);
    a.state = (uint8_t*)d_state;
    a.count = d_count;
    a.index = d_index;
    a.value = d_value;
    a.max_peaks = max_peaks;
    a.sig = d_sig;
    a.thr = d_threshold;
    return true;
}

// A variant's three filters as the detector's constructor designs them (create_filter_iir(f.d, f.n, ...): numerator -> d), and
// its constants.  (Every design is valid for fs > 0.)
static bool peak_coef(int variant, double sampling_rate, double marker_val, PeakCoef& c) {
    static const struct { int bp_order; double bp_lo, bp_hi; int ig_order; double A; } kVar[3] = {
        {2, 10.0, 20.0, 2, 25.0}, {1, 10.0, 20.0, 1, 25.0}, {1, 15.0, 25.0, 1, 70.0}};
    const auto& v = kVar[variant];
    if (!design_iir(kFiltBandPass, v.bp_order, sampling_rate, v.bp_lo, v.bp_hi, c.bf, c.bb) ||
        !design_iir(kFiltLowPass, v.ig_order, sampling_rate, 3.0, 0.0, c.gf, c.gb) ||
        !design_iir(kFiltLowPass, 2, sampling_rate, 0.15, 0.0, c.tf, c.tb))
        return false;
    c.atten = 1.0 / (1.0 + v.A / sampling_rate);
    c.marker = marker_val;
    c.nslope = (int32_t)((100.0 * sampling_rate) / 1000.0);
    c.hist = 4 * (int32_t)sampling_rate;
    return true;
}

// One lane per detector, 64 to a workgroup, on the caller's stream.
template <class Args, class Coef>
static int peak_launch(rspt_hip_packer* p, void (*kern)(Args, Coef), const Args& a, const Coef& c, void* stream) {
    HIPCHK(p, hipSetDevice(p->device));
    hipLaunchKernelGGL(kern, dim3((a.lanes + 63) / 64), dim3(64), 0, (hipStream_t)stream, a, c);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_peak_state_bytes(rspt_hip_packer* p, size_t* bytes) {
    if (!p || !bytes) return RSPT_HIP_ERR_ARG;
    *bytes = (size_t)p->g.nch * kPeakStateBytesPerChannel;
    return RSPT_HIP_OK;
}

// Both online entries: d_src is the native batch, or (planar) the int32 matrix.
static int peak_call(rspt_hip_packer* p, const void* d_src, size_t nblocks, int variant, double sampling_rate, double marker_val, void* d_state,
                     uint32_t* d_count, int32_t* d_index, double* d_value, size_t max_peaks, double* d_sig, double* d_threshold, void* stream,
                     bool planar) {
    PeakArgs a{};
    PeakCoef c{};
    if (variant < kPeakOnline || variant > kPeakOfflineFw ||
        !peak_args(p, d_src, nblocks, sampling_rate, d_state, d_count, d_index, d_value, max_peaks, d_sig, d_threshold, a, planar) ||
        !peak_coef(variant, sampling_rate, marker_val, c))
        return RSPT_HIP_ERR_ARG;
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    auto by_variant = [&](auto go) {
        if (variant == kPeakOnline) return go(std::integral_constant<int, kPeakOnline>());
        if (variant == kPeakOnline1st) return go(std::integral_constant<int, kPeakOnline1st>());
        return go(std::integral_constant<int, kPeakOfflineFw>());
    };
    if (planar)
        return by_variant([&](auto vv) {
            constexpr int V = decltype(vv)::value;
            return peak_launch(p, d_sig ? &k_peak_planar<V, true> : &k_peak_planar<V, false>, a, c, stream);
        });
    return by_bps(p->g.bps, [&](auto bb) {
        constexpr int B = decltype(bb)::value;
        return by_variant([&](auto vv) {
            constexpr int V = decltype(vv)::value;
            return peak_launch(p, d_sig ? &k_peak<B, V, true> : &k_peak<B, V, false>, a, c, stream);
        });
    });
}

int rspt_hip_peak_detect_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, int variant, double sampling_rate, double marker_val,
                                   void* d_state, uint32_t* d_count, int32_t* d_index, double* d_value, size_t max_peaks, double* d_sig,
                                   double* d_threshold, void* stream) {
    return peak_call(p, d_src, nblocks, variant, sampling_rate, marker_val, d_state, d_count, d_index, d_value, max_peaks, d_sig, d_threshold, stream,
                     false);
}

int rspt_hip_peak_detect_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, int variant, double sampling_rate,
                                          double marker_val, void* d_state, uint32_t* d_count, int32_t* d_index, double* d_value, size_t max_peaks,
                                          double* d_sig, double* d_threshold, void* stream) {
    return peak_call(p, d_planar, nblocks, variant, sampling_rate, marker_val, d_state, d_count, d_index, d_value, max_peaks, d_sig, d_threshold,
                     stream, true);
}

int rspt_hip_peak_offline_work_bytes(rspt_hip_packer* p, size_t nblocks, int stateful, size_t* bytes) {
    if (!p || !bytes || !batch_count_ok(p, nblocks)) return RSPT_HIP_ERR_ARG;
    const Geom& g = p->g;
    const uint64_t lanes = stateful ? g.nch : (uint64_t)nblocks * g.nch;
    *bytes = (size_t)(((lanes + 63) / 64) * kPeakOffSlabBytesPerSample * g.ns);
    return RSPT_HIP_OK;
}

// Both offline entries, as peak_call.
static int peak_offline_call(rspt_hip_packer* p, const void* d_src, size_t nblocks, double sampling_rate, double marker_val, void* d_state,
                             void* d_work, uint32_t* d_count, int32_t* d_index, double* d_value, size_t max_peaks, double* d_sig,
                             double* d_threshold, void* stream, bool planar) {
    PeakOffArgs a{};
    PeakOffCoef k{};
    if (!d_work || ((uintptr_t)d_work % 8) != 0 ||
        !peak_args(p, d_src, nblocks, sampling_rate, d_state, d_count, d_index, d_value, max_peaks, d_sig, d_threshold, a, planar) ||
        !peak_coef(kPeakOfflineFw, sampling_rate, marker_val, k.c))
        return RSPT_HIP_ERR_ARG;
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    // the reference's undefined cases: nr_slope_samples 0 (the shift runs every event off the end of the array) and a block
    // shorter than the relocation radius (the unsigned bound len - radius wraps)
    k.radius = (int32_t)((10.0 * sampling_rate) / 1000.0);
    if (k.c.nslope == 0 || (uint64_t)a.ns < (uint64_t)k.radius) return RSPT_HIP_ERR_ARG;
    // peak_detector_offline's constructor adds the baseline: a 0.5 Hz first-order low-pass
    if (!design_iir(kFiltLowPass, 1, sampling_rate, 0.5, 0.0, k.lf, k.lb)) return RSPT_HIP_ERR_ARG;
    a.work = (uint8_t*)d_work;
    if (planar) return peak_launch(p, d_sig ? &k_peak_offline_planar<true> : &k_peak_offline_planar<false>, a, k, stream);
    return by_bps(p->g.bps, [&](auto bb) {
        constexpr int B = decltype(bb)::value;
        return peak_launch(p, d_sig ? &k_peak_offline<B, true> : &k_peak_offline<B, false>, a, k, stream);
    });
}

int rspt_hip_peak_detect_offline_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, double sampling_rate, double marker_val,
                                           void* d_state, void* d_work, uint32_t* d_count, int32_t* d_index, double* d_value,
                                           size_t max_peaks, double* d_sig, double* d_threshold, void* stream) {
    return peak_offline_call(p, d_src, nblocks, sampling_rate, marker_val, d_state, d_work, d_count, d_index, d_value, max_peaks, d_sig, d_threshold,
                             stream, false);
}

int rspt_hip_peak_detect_offline_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, double sampling_rate,
                                                  double marker_val, void* d_state, void* d_work, uint32_t* d_count, int32_t* d_index,
                                                  double* d_value, size_t max_peaks, double* d_sig, double* d_threshold, void* stream) {
    return peak_offline_call(p, d_planar, nblocks, sampling_rate, marker_val, d_state, d_work, d_count, d_index, d_value, max_peaks, d_sig,
                             d_threshold, stream, true);
}
