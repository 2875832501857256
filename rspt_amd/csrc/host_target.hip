// host_target.hip -- compress to a PRDN target (rspt_hip.h: rspt_hip_compress_target_batch_dev and its planar form,
// rspt_hip_compress_target_planar_batch_dev), included by rspt_hip.hip.
//
// The probes find, per block and ladder entry, the PRDN the entry's stream would decode to -- without the hzr stage, which changes
// no value -- k_target_select applies the rule, and rspt_hip_compress_batch_ladder_dev's path writes the streams.
//
// The caller's d_work, every part on a 256-byte boundary:
//   orig   [nblocks][nch][ns] int32   the native blocks as the front end sees them (rspt_hip_native_to_i32_batch_dev)
//   dec    [nblocks][nch][ns] int32   one candidate's decoded samples
//   nz     [nblocks][4][nblk] uint32  where the candidates' plane kernels mark their non-zero segments (never read)
//   prdn, mse [nladder][nblocks] double, path [nladder][nblocks] uint32: what rspt_hip_prdn_planar_batch_dev says of each candidate
//   acc    [nladder][nblocks][4] uint64, flag [nladder][nblocks] uint32: the fused probe's exact sums and k_q_finish's flags
// Two routes, picked from the handle's shape alone (rspt_hip_debug_set_target_route overrides it for the tests):
//   general  every supported shape: per ladder entry the kernels of a compress and a decompress call, then the planar PRDN entry
//   fused    hadamard rows of up to kTpMaxNs points with nch * ns < 2^22: k_target_probe (target.hip) -- one pass over the block
//            for all entries -- and k_q_finish on its table
// The planar form reads the caller's matrix where the native one reads orig, and keeps the five tables in the handle's workspace
// (Workspace::target_tab), so that its d_work holds block-sized scratch alone:
//   general  orig only on a handle of bps < 4 (the matrix cut to the sample width, for the PRDN step; at bps 4 the matrix is
//            the original), dec, nz
//   fused    nothing: k_planar_target_probe reads each row from the matrix
struct TargetWork {
    enum Form { NATIVE, PLANAR_GENERAL, PLANAR_FUSED };
    int32_t *orig = nullptr, *dec = nullptr;
    uint32_t *nz = nullptr, *path, *flag;
    double *prdn, *mse;
    unsigned long long* acc;
    size_t bytes;  // of d_work
    // tab: where the tables of a planar form lie (Workspace::target_tab)
    TargetWork(const rspt_hip_packer* p, void* base, size_t nblocks, size_t nladder, Form form = NATIVE, void* tab = nullptr) {
        size_t at = 0;
        auto take = [&](size_t n) {
            uint8_t* q = (uint8_t*)base + at;
            at += (n + 255) & ~(size_t)255;
            return q;
        };
        const size_t planar = nblocks * (size_t)p->g.N * sizeof(int32_t), cells = nladder * nblocks;
        if (form == NATIVE || (form == PLANAR_GENERAL && p->g.bps < 4)) orig = (int32_t*)take(planar);
        if (form != PLANAR_FUSED) {
            dec = (int32_t*)take(planar);
            nz = (uint32_t*)take(nblocks * kMaxPlanes * p->g.nblk * sizeof(uint32_t));
        }
        if (form != NATIVE) {  // (a d_work of no bytes would be no pointer: 16 at the least)
            bytes = at < 16 ? 16 : at;
            base = tab, at = 0;
        }
        prdn = (double*)take(cells * sizeof(double));
        mse = (double*)take(cells * sizeof(double));
        path = (uint32_t*)take(cells * sizeof(uint32_t));
        acc = (unsigned long long*)take(cells * 4 * sizeof(unsigned long long));
        flag = (uint32_t*)take(cells * sizeof(uint32_t));
        if (form == NATIVE) bytes = at;  // (a planar form's tables: at most target_tab_bytes(nblocks), host_handle.hpp)
    }
};

// the refusals of both entries that come from the handle and the batch alone
static int target_checks(const rspt_hip_packer* p, size_t nblocks, size_t nladder) {
    if (!p || nblocks == 0 || nblocks > 65535) return RSPT_HIP_ERR_ARG;  // (65535: rspt_hip_reserve)
    const Geom& g = p->g;
    if (g.kind != RSPT_HIP_KIND_HADAMARD && !(g.kind == RSPT_HIP_KIND_DCT && !p->dct_fft)) return RSPT_HIP_ERR_UNSUPPORTED;
    if (nladder < 1 || nladder > kMaxLadder) return RSPT_HIP_ERR_ARG;
    return RSPT_HIP_OK;
}

int rspt_hip_compress_target_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    if (!bytes) return RSPT_HIP_ERR_ARG;
    if (int rc = target_checks(p, nblocks, nladder)) return rc;
    *bytes = TargetWork(p, nullptr, nblocks, nladder).bytes;
    return RSPT_HIP_OK;
}

// One candidate on the general route: the kernels of a compress and a decompress call at the handle's current quantiser, the hzr
// stage left out -- orig -> forward transform -> planes of nb bytes -> planar -> inverse transform -> the cut to the sample width
// -> its PRDN against orig, into row k of the table.  d_planar: the planar form -- the caller's matrix goes into ws.planar through
// the planar front end's own k_planar_ingest, which cuts it, and is the original itself where w has none.
static int target_probe_general(rspt_hip_packer* p, const TargetWork& w, size_t nblocks, size_t k, hipStream_t st, const int32_t* d_planar) {
    const Geom& g = p->g;
    const uint32_t B = (uint32_t)nblocks;
    if (d_planar)
        hipLaunchKernelGGL(k_planar_ingest, dim3((g.ns + 4095u) / 4096u, g.nch, B), dim3(256), 0, st, d_planar, g, (int32_t*)p->ws.planar, (long long*)nullptr);
    else
        HIPCHK(p, hipMemcpyAsync(p->ws.planar, w.orig, nblocks * (size_t)g.N * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    launch_forward_transform(p, B, st, w.nz, nullptr);
    HIPCHK(p, hipMemsetD32Async((hipDeviceptr_t)(uint32_t*)p->ws.dec_nb, (int)p->nb_host, nblocks, st));  // every candidate has the handle's nb planes
    const int32_t* back = launch_inverse(p, B, st, p->ws.planar, 0u, nullptr);
    const uint64_t wgs = ((uint64_t)B * g.N + 255) / 256, want = 16ull * (uint64_t)p->num_cu;
    hipLaunchKernelGGL(k_planar_emit, dim3((uint32_t)(wgs < want ? wgs : want)), dim3(256), 0, st, back, g, B, w.dec);
    HIPCHK(p, hipGetLastError());
    return rspt_hip_prdn_planar_batch_dev(p, w.orig ? w.orig : d_planar, w.dec, nblocks, w.prdn + k * nblocks, w.mse + k * nblocks, nullptr,
                                          w.path + k * nblocks, (void*)st);
}

static int target_probes_general(rspt_hip_packer* p, const TargetWork& w, const double* ladder, size_t nladder, size_t nblocks, hipStream_t st,
                                 const int32_t* d_planar = nullptr);

// where the fused probe runs: its row length, and the bound under which every reference sum is exact
static bool target_fused_ok(const rspt_hip_packer* p) {
    const Geom& g = p->g;
    return g.kind == RSPT_HIP_KIND_HADAMARD && g.ns <= kTpMaxNs && g.N < (1u << 22);
}

int rspt_hip_debug_set_target_route(rspt_hip_packer* p, int route) {
    if (!p || route < 0 || route > 2) return RSPT_HIP_ERR_ARG;
    if (route == 2 && !target_fused_ok(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    p->target_route = (uint32_t)route;
    return RSPT_HIP_OK;
}

// Every candidate of every block on the fused route: the table's exact sums in one kernel, finished by the PRDN stage's own k_q_finish.
// d_planar: the planar form -- k_planar_target_probe on the caller's matrix
static int target_probe_fused(rspt_hip_packer* p, const TargetWork& w, const LadderSel& ls, size_t nblocks, hipStream_t st, const int32_t* d_planar = nullptr) {
    const Geom& g = p->g;
    const uint32_t B = (uint32_t)nblocks, cells = ls.fwd.n * B;
    HIPCHK(p, hipMemsetAsync(w.acc, 0, (size_t)cells * 4 * sizeof(unsigned long long), st));
    const uint32_t nt = std::max(64u, std::min(1024u, g.ns / kTpPer));
    const uint32_t lds = 2u * tp_pad(g.ns) * (uint32_t)sizeof(uint32_t);
    if (d_planar) {
        HIPCHK(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_planar_target_probe), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_planar_target_probe, dim3(g.nch, B), dim3(nt), lds, st, d_planar, g, ls.fwd, ls.inv, (uint32_t)p->nb_host, B, w.acc);
    } else {
        HIPCHK(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_target_probe), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_target_probe, dim3(g.nch, B), dim3(nt), lds, st, (const int32_t*)w.orig, g, ls.fwd, ls.inv, (uint32_t)p->nb_host, B, w.acc);
    }
    hipLaunchKernelGGL(k_q_finish, dim3((cells + 255) / 256), dim3(256), 0, st, (const unsigned long long*)w.acc, cells, w.flag, w.prdn, w.mse,
                       (double*)nullptr, w.path);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_compress_target_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder, double target_prdn,
                                       void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice, double* d_prdn, void* d_work,
                                       void* stream) {
    if (!p || !d_src || !d_dst || !d_sizes || !d_choice || !d_work || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_src) & 15) || (reinterpret_cast<uintptr_t>(d_choice) & 3) || (reinterpret_cast<uintptr_t>(d_prdn) & 7) ||
        (reinterpret_cast<uintptr_t>(d_work) & 15))
        return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    if (int rc = target_checks(p, nblocks, nladder)) return rc;
    LadderSel ls;
    if (int rc = make_ladder(p, ladder, nladder, d_choice, &ls)) return rc;
    if (!std::isfinite(target_prdn) || !(target_prdn > 0.0)) return RSPT_HIP_ERR_ARG;
    if ((unsigned long long)dst_stride >> 32 >= p->g.nblk) return RSPT_HIP_ERR_ARG;  // (as rspt_hip_compress_batch_ladder_dev)
    if (int rc = rspt_hip_reserve(p, nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const TargetWork w(p, d_work, nblocks, nladder);
    if (int rc = rspt_hip_native_to_i32_batch_dev(p, d_src, w.orig, nblocks, stream)) return rc;
    const bool fused = p->target_route ? p->target_route == 2 : target_fused_ok(p);
    if (fused) {
        if (int rc = target_probe_fused(p, w, ls, nblocks, st)) return rc;
    } else {
        if (int rc = target_probes_general(p, w, ladder, nladder, nblocks, st)) return rc;
    }
    hipLaunchKernelGGL(k_target_select, dim3(((uint32_t)nblocks + 255) / 256), dim3(256), 0, st, (const double*)w.prdn, (const double*)w.mse,
                       (const uint32_t*)w.path, (uint32_t)nladder, (uint32_t)nblocks, target_prdn, d_choice, d_prdn);
    HIPCHK(p, hipGetLastError());
    return compress_batch_serial(p, d_src, nblocks, d_dst, dst_stride, d_sizes, st, nullptr, &ls);
}

// ---- the planar form -------------------------------------------------------------------------------------------------------------
static TargetWork::Form target_planar_form(const rspt_hip_packer* p) {
    const bool fused = p->target_route ? p->target_route == 2 : target_fused_ok(p);
    return fused ? TargetWork::PLANAR_FUSED : TargetWork::PLANAR_GENERAL;
}

int rspt_hip_compress_target_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    if (!bytes) return RSPT_HIP_ERR_ARG;
    if (int rc = target_checks(p, nblocks, nladder)) return rc;
    *bytes = TargetWork(p, nullptr, nblocks, nladder, target_planar_form(p)).bytes;
    return RSPT_HIP_OK;
}

int rspt_hip_compress_target_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                                              double target_prdn, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice,
                                              double* d_prdn, void* d_work, void* stream) {
    if (!p || !d_planar || !d_dst || !d_sizes || !d_choice || !d_work || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_planar) & 3) || (reinterpret_cast<uintptr_t>(d_choice) & 3) || (reinterpret_cast<uintptr_t>(d_prdn) & 7) ||
        (reinterpret_cast<uintptr_t>(d_work) & 15))
        return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    if (int rc = target_checks(p, nblocks, nladder)) return rc;
    LadderSel ls;
    if (int rc = make_ladder(p, ladder, nladder, d_choice, &ls)) return rc;
    if (!std::isfinite(target_prdn) || !(target_prdn > 0.0)) return RSPT_HIP_ERR_ARG;
    if ((unsigned long long)dst_stride >> 32 >= p->g.nblk) return RSPT_HIP_ERR_ARG;  // (as rspt_hip_compress_batch_ladder_dev)
    if (int rc = rspt_hip_reserve(p, nblocks)) return rc;  // (the tables lie in the workspace)
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const Geom& g = p->g;
    const TargetWork::Form form = target_planar_form(p);
    const TargetWork w(p, d_work, nblocks, nladder, form, p->ws.target_tab);
    if (form == TargetWork::PLANAR_FUSED) {
        if (int rc = target_probe_fused(p, w, ls, nblocks, st, d_planar)) return rc;
    } else {
        if (w.orig)  // bps < 4: the original of the rule is the matrix cut to the sample width
            hipLaunchKernelGGL(k_planar_ingest, dim3((g.ns + 4095u) / 4096u, g.nch, (unsigned)nblocks), dim3(256), 0, st, d_planar, g, w.orig, (long long*)nullptr);
        if (int rc = target_probes_general(p, w, ladder, nladder, nblocks, st, d_planar)) return rc;
    }
    hipLaunchKernelGGL(k_target_select, dim3(((uint32_t)nblocks + 255) / 256), dim3(256), 0, st, (const double*)w.prdn, (const double*)w.mse,
                       (const uint32_t*)w.path, (uint32_t)nladder, (uint32_t)nblocks, target_prdn, d_choice, d_prdn);
    HIPCHK(p, hipGetLastError());
    return compress_batch_serial(p, nullptr, nblocks, d_dst, dst_stride, d_sizes, st, d_planar, &ls);
}

// all candidates on the general route
static int target_probes_general(rspt_hip_packer* p, const TargetWork& w, const double* ladder, size_t nladder, size_t nblocks, hipStream_t st,
                                 const int32_t* d_planar) {
    p->ws.planes_unknown = true;  // the candidates' planes land in the compressor's plane workspace
    // every candidate runs under its own quantiser: the handle's fields are what the launches read, so they take the entry's
    // values for the length of its launches (kernel arguments: nothing of it outlives them) and then their own again
    const Quantizer own{p->dct_scale0, p->dct_scale1, p->idct_scale, p->dct_cs0, p->had_div_fwd, p->had_div_inv};
    const double own_quality = p->quality;
    const bool own_quant = p->had_quant;
    int rc = RSPT_HIP_OK;
    for (size_t k = 0; k < nladder && rc == RSPT_HIP_OK; ++k) {
        set_quality(p, ladder[k]);
        rc = target_probe_general(p, w, nblocks, k, st, d_planar);
    }
    p->dct_scale0 = own.dct_scale0, p->dct_scale1 = own.dct_scale1, p->idct_scale = own.idct_scale, p->dct_cs0 = own.dct_cs0;
    p->had_div_fwd = own.had_div_fwd, p->had_div_inv = own.had_div_inv, p->had_quant = own_quant, p->quality = own_quality;
    return rc;
}
