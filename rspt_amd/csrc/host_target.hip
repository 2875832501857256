// host_target.hip -- compress to a PRDN target (rspt_hip.h: rspt_hip_compress_target_batch_dev and its planar form,
// rspt_hip_compress_target_planar_batch_dev), included by rspt_hip.hip behind host_rate.hip, whose frame both go through.
//
// The probes find, per block and ladder entry, the PRDN the entry's stream would decode to -- without the hzr stage, which changes
// no value -- and k_target_select applies the rule.  The work area is rate_work::Target (rate_work.hpp).
// Two routes, picked from the handle's shape alone (rspt_hip_debug_set_target_route overrides it for the tests):
//   general  every supported shape: per ladder entry the kernels of a compress and a decompress call, then the planar PRDN entry
//   fused    hadamard rows of up to kTpMaxNs points with nch * ns < 2^22: k_target_probe (target.hip) -- one pass over the block
//            for all entries -- and k_q_finish on its table
// The native form converts its blocks into orig (rspt_hip_native_to_i32_batch_dev).  The planar form reads the caller's matrix
// where the native one reads orig:
//   general  orig only on a handle of bps < 4 (the matrix cut to the sample width, for the PRDN step; at bps 4 the matrix is
//            the original)
//   fused    nothing: k_planar_target_probe reads each row from the matrix
struct TargetWork {
    int32_t *orig, *dec;
    uint32_t *nz, *path, *flag;
    double *prdn, *mse;
    unsigned long long* acc;
    // work: the layout's d_work; tab: where its tables lie
    TargetWork(const rate_work::Target& l, void* work, void* tab)
        : orig(rate_work::part<int32_t>(work, l.orig)),
          dec(rate_work::part<int32_t>(work, l.dec)),
          nz(rate_work::part<uint32_t>(work, l.nz)),
          path(rate_work::part<uint32_t>(tab, l.tab.path)),
          flag(rate_work::part<uint32_t>(tab, l.tab.flag)),
          prdn(rate_work::part<double>(tab, l.tab.prdn)),
          mse(rate_work::part<double>(tab, l.tab.mse)),
          acc(rate_work::part<unsigned long long>(tab, l.tab.acc)) {}
};

// where the fused probe runs: its row length, and the bound under which every reference sum is exact
static bool target_fused_ok(const rspt_hip_packer* p, size_t = 1, size_t = 1) {
    const Geom& g = p->g;
    return g.kind == RSPT_HIP_KIND_HADAMARD && g.ns <= kTpMaxNs && g.N < (1u << 22);
}

int rspt_hip_debug_set_target_route(rspt_hip_packer* p, int route) { return rate_set_route(p, RATE_TARGET, route, target_fused_ok); }

static int target_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes, bool planar) {
    const int route = rate_sizing(p, nblocks, nladder, bytes, RATE_TARGET, target_fused_ok);
    if (route < 0) return route;
    const Geom& g = p->g;
    *bytes = rate_work::Target(g.N, g.nblk, g.bps, nblocks, nladder, planar ? rate_work::Total::form(route, true) : rate_work::NATIVE).bytes;
    return RSPT_HIP_OK;
}

int rspt_hip_compress_target_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    return target_work_bytes(p, nblocks, nladder, bytes, false);
}

int rspt_hip_compress_target_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    return target_work_bytes(p, nblocks, nladder, bytes, true);
}

// One candidate on the general route: the kernels of a compress and a decompress call at the handle's current quantiser, the hzr
// stage left out -- orig -> forward transform -> planes of nb bytes -> planar -> inverse transform -> the cut to the sample width
// -> its PRDN against orig, into row k of the table.  d_planar: the planar form -- the caller's matrix goes into ws.planar through
// the planar front end's own k_planar_ingest, which cuts it, and is the original itself where w has none.
static int target_probe_general(rspt_hip_packer* p, const TargetWork& w, size_t nblocks, size_t k, hipStream_t st, const int32_t* d_planar) {
    const Geom& g = p->g;
    const uint32_t B = (uint32_t)nblocks;
    if (d_planar)
        ingest_cut(p, d_planar, nblocks, (int32_t*)p->ws.planar, st);
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

// All candidates on the general route, from w.orig (or the matrix): the planar form first cuts the matrix into an orig it has
static int target_probes_general(rspt_hip_packer* p, const TargetWork& w, const double* ladder, size_t nladder, size_t nblocks, hipStream_t st,
                                 const int32_t* d_planar) {
    if (d_planar && w.orig) ingest_cut(p, d_planar, nblocks, w.orig, st);
    p->ws.planes_unknown = true;  // the candidates' planes land in the compressor's plane workspace
    const QuantizerScope own(p);
    for (size_t k = 0; k < nladder; ++k) {
        set_quality(p, ladder[k]);
        if (int rc = target_probe_general(p, w, nblocks, k, st, d_planar)) return rc;
    }
    return RSPT_HIP_OK;
}

// Every candidate of every block on the fused route: the table's exact sums in one kernel, finished by the PRDN stage's own k_q_finish
static int target_probe_fused(rspt_hip_packer* p, const TargetWork& w, const LadderSel& ls, size_t nblocks, hipStream_t st, const int32_t* d_planar) {
    const uint32_t B = (uint32_t)nblocks, cells = ls.fwd.n * B;
    HIPCHK(p, hipMemsetAsync(w.acc, 0, (size_t)cells * 4 * sizeof(unsigned long long), st));
    if (int rc = probe_launch(p, k_target_probe, k_planar_target_probe, w.orig, d_planar, 2, B, st, ls.fwd, ls.inv, (uint32_t)p->nb_host, B, w.acc)) return rc;
    hipLaunchKernelGGL(k_q_finish, dim3((cells + 255) / 256), dim3(256), 0, st, (const unsigned long long*)w.acc, cells, w.flag, w.prdn, w.mse,
                       (double*)nullptr, w.path);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

// Both entries.  d_prdn is the entry's own optional pointer; a planar form's tables lie in the workspace (rspt_hip_reserve).
static int compress_target(RateCall c, double target_prdn, double* d_prdn) {
    if (misaligned(d_prdn, 8)) return RSPT_HIP_ERR_ARG;
    if (int rc = rate_begin(c, RATE_TARGET, target_fused_ok, std::isfinite(target_prdn) && target_prdn > 0.0)) return rc;
    rspt_hip_packer* p = c.p;
    const Geom& g = p->g;
    const rate_work::Target l(g.N, g.nblk, g.bps, c.nblocks, c.nladder, c.d_planar ? rate_work::Total::form(c.route, true) : rate_work::NATIVE);
    const TargetWork w(l, c.d_work, c.d_planar ? (uint8_t*)p->ws.target_tab : (uint8_t*)c.d_work + l.scratch);
    if (!c.d_planar)
        if (int rc = rspt_hip_native_to_i32_batch_dev(p, c.d_src, w.orig, c.nblocks, (void*)c.st)) return rc;
    if (int rc = c.route ? target_probe_fused(p, w, c.ls, c.nblocks, c.st, c.d_planar)
                         : target_probes_general(p, w, c.ladder, c.nladder, c.nblocks, c.st, c.d_planar))
        return rc;
    hipLaunchKernelGGL(k_target_select, dim3(((uint32_t)c.nblocks + 255) / 256), dim3(256), 0, c.st, (const double*)w.prdn, (const double*)w.mse,
                       (const uint32_t*)w.path, (uint32_t)c.nladder, (uint32_t)c.nblocks, target_prdn, c.d_choice, d_prdn);
    return rate_finish(c);
}

int rspt_hip_compress_target_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder, double target_prdn,
                                       void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice, double* d_prdn, void* d_work,
                                       void* stream) {
    return compress_target({p, d_src, nullptr, nblocks, ladder, nladder, d_dst, dst_stride, d_sizes, d_choice, d_work, (hipStream_t)stream}, target_prdn,
                           d_prdn);
}

int rspt_hip_compress_target_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                                              double target_prdn, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice,
                                              double* d_prdn, void* d_work, void* stream) {
    return compress_target({p, nullptr, d_planar, nblocks, ladder, nladder, d_dst, dst_stride, d_sizes, d_choice, d_work, (hipStream_t)stream}, target_prdn,
                           d_prdn);
}
