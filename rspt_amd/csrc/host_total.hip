// host_total.hip -- compress a batch to one byte total (rspt_hip.h: rspt_hip_compress_total_batch_dev and its planar form,
// rspt_hip_compress_total_planar_batch_dev), included by rspt_hip.hip.
//
// The two tables of the siblings -- every candidate's stream size (host_budget.hip) and every candidate's PRDN figure
// (host_target.hip) -- are filled for one batch, k_total_figs / k_total_level / k_total_pick (total.hip) apply the rule on the
// device, and rspt_hip_compress_batch_ladder_dev's path writes the chosen streams.
//
// The caller's d_work, every part on a 256-byte boundary:
//   sizes  [nladder][nblocks] uint64   the budget entry's table
//   figs   [nladder][nblocks] uint64   the figures as bit patterns (k_total_figs)
//   res    [3] uint64, and kTotalRounds slots behind them: T*, cost(T*) and the lower bound between the level kernels and
//          k_total_pick; a round's sums (k_total_round)
//   then   general: the target entry's whole work area (TargetWork: orig, dec, nz and its five tables)
//          fused:   the five tables alone -- the converted blocks lie in the last entry's slots of ws.planar
// Two routes (rspt_hip_debug_set_total_route overrides the host's pick for the tests):
//   general  every shape the ladder takes: the target entry's probes per ladder entry (target_probes_general), then the budget
//            entry's passes per ladder entry (budget_sizes_general) -- two forward transforms per entry, each inside its own
//            sequence, so that neither sequence's bookkeeping changes
//   fused    hadamard rows of up to kTpMaxNs points with nch * ns < 2^22 and nladder * nblocks <= 65535 block slots: k_total_probe
//            reads each row once for both tables, k_q_finish finishes its sums, and ONE pass of k_planar_planes / k_nb_scan /
//            k_histlist / k_hist / k_tree runs over all slots, as on the budget entry's batched route
// The planar form is the same body (compress_total) with the caller's matrix as the source, on the same route:
//   general  the matrix is the original of the figures at bps 4 -- d_work has no orig, one 256-padded nblocks * N * 4 block less
//            -- and k_planar_ingest of it into orig at bps < 4; the planar front end ingests the matrix per entry in both
//            sequences, cutting it to the sample width, and again in the final pass
//   fused    k_planar_total_probe reads each row from the matrix, cutting it on load: no converter pass, no original inside
//            ws.planar -- nothing but the probe reads the matrix and every slot is only written.  The work area is the native one.
struct TotalWork {
    unsigned long long *sizes, *figs, *res;
    size_t scratch;  // the planar general route: the block-sized parts of the target entry's area, its tables behind them
    TargetWork t;
    size_t bytes;
    static size_t pad(size_t n) { return (n + 255) & ~(size_t)255; }
    static constexpr size_t kResBytes = 256 + kTotalRounds * sizeof(TotalSlot);
    static size_t head(size_t cells) { return 2 * pad(cells * sizeof(unsigned long long)) + pad(kResBytes); }
    TotalSlot* slots() const { return (TotalSlot*)((uint8_t*)res + 256); }
    static TargetWork::Form form(bool fused, bool planar) {
        return fused ? TargetWork::PLANAR_FUSED : planar ? TargetWork::PLANAR_GENERAL : TargetWork::NATIVE;
    }
    // planar: the source is the caller's matrix (the fused area does not depend on it)
    TotalWork(const rspt_hip_packer* p, void* base, size_t nblocks, size_t nladder, bool fused, bool planar = false)
        : sizes((unsigned long long*)base),
          figs((unsigned long long*)((uint8_t*)base + pad(nladder * nblocks * sizeof(unsigned long long)))),
          res((unsigned long long*)((uint8_t*)base + 2 * pad(nladder * nblocks * sizeof(unsigned long long)))),
          scratch(!fused && planar ? TargetWork(p, nullptr, nblocks, nladder, TargetWork::PLANAR_GENERAL).bytes : 0),
          t(p, (uint8_t*)base + head(nladder * nblocks), nblocks, nladder, form(fused, planar), (uint8_t*)base + head(nladder * nblocks) + scratch) {
        // (a TargetWork of a planar form names no bytes of its tables: they end behind flag, its last one)
        const size_t tables = (size_t)((uint8_t*)t.flag - ((uint8_t*)base + head(nladder * nblocks) + scratch)) + pad(nladder * nblocks * sizeof(uint32_t));
        bytes = head(nladder * nblocks) + (fused || planar ? scratch + tables : t.bytes);
    }
};

// where the fused route runs: the fused probe of the target entry and the batched route of the budget entry both take the call
static bool total_fused_ok(const rspt_hip_packer* p, size_t nblocks, size_t nladder) {
    return target_fused_ok(p) && budget_batched_ok(p, nblocks, nladder);
}

// 1: the fused route, 0: the general one, < 0: a forced fused route on a call it does not take
static int total_route(const rspt_hip_packer* p, size_t nblocks, size_t nladder) {
    const bool ok = total_fused_ok(p, nblocks, nladder);
    if (p->total_route == 2) return ok ? 1 : RSPT_HIP_ERR_UNSUPPORTED;
    return p->total_route == 0 && ok ? 1 : 0;
}

int rspt_hip_debug_set_total_route(rspt_hip_packer* p, int route) {
    if (!p || route < 0 || route > 2) return RSPT_HIP_ERR_ARG;
    if (route == 2 && !total_fused_ok(p, 1, 1)) return RSPT_HIP_ERR_UNSUPPORTED;  // (the shape; the slot bound is each call's)
    p->total_route = (uint32_t)route;
    return RSPT_HIP_OK;
}

static int total_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes, bool planar) {
    if (!bytes) return RSPT_HIP_ERR_ARG;
    if (int rc = target_checks(p, nblocks, nladder)) return rc;
    const int route = total_route(p, nblocks, nladder);
    if (route < 0) return route;
    *bytes = TotalWork(p, nullptr, nblocks, nladder, route == 1, planar).bytes;
    return RSPT_HIP_OK;
}

int rspt_hip_compress_total_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    return total_work_bytes(p, nblocks, nladder, bytes, false);
}

// both tables on the fused route.  d_planar: the planar form -- k_planar_total_probe on the caller's matrix: no converter pass,
// and no row of ws.planar is read
static int total_tables_fused(rspt_hip_packer* p, const void* d_src, const int32_t* d_planar, size_t nblocks, const LadderSel& ls, const TotalWork& w,
                              hipStream_t st) {
    const Geom& g = p->g;
    const uint32_t B = (uint32_t)nblocks, S = ls.fwd.n * B;  // block slots: entry k of block b is slot k * B + b
    if (int rc = rspt_hip_reserve(p, S)) return rc;
    if (int rc = front_begin(p, S, st)) return rc;
    int32_t* orig = p->ws.planar + (size_t)(S - B) * g.N;  // the last entry's slots: each row is read before it is written
    if (!d_planar)
        if (int rc = rspt_hip_native_to_i32_batch_dev(p, d_src, orig, nblocks, (void*)st)) return rc;
    HIPCHK(p, hipMemsetAsync(w.t.acc, 0, (size_t)S * 4 * sizeof(unsigned long long), st));
    const uint32_t nt = std::max(64u, std::min(1024u, g.ns / kTpPer));
    const uint32_t lds = 2u * tp_pad(g.ns) * (uint32_t)sizeof(uint32_t);
    if (d_planar) {
        HIPCHK(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_planar_total_probe), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_planar_total_probe, dim3(g.nch, B), dim3(nt), lds, st, d_planar, g, ls.fwd, ls.inv, (uint32_t)p->nb_host, B,
                           (int32_t*)p->ws.planar, w.t.acc);
    } else {
        HIPCHK(p, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_total_probe), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(k_total_probe, dim3(g.nch, B), dim3(nt), lds, st, (const int32_t*)orig, g, ls.fwd, ls.inv, (uint32_t)p->nb_host, B,
                           (int32_t*)p->ws.planar, w.t.acc);
    }
    hipLaunchKernelGGL(k_q_finish, dim3((S + 255) / 256), dim3(256), 0, st, (const unsigned long long*)w.t.acc, S, w.t.flag, w.t.prdn, w.t.mse,
                       (double*)nullptr, w.t.path);
    // from here on what phase_front runs behind a lossy packer's transform, over all slots (budget_sizes_batched)
    hipLaunchKernelGGL((k_planar_planes<false>), dim3((g.N + 4095) / 4096, S), dim3(256), 0, st, p->ws.planar, g, (uint32_t)p->nb_host, p->ws.planes,
                       p->nzflag, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_nb_scan, dim3(1), dim3(1024), 0, st, p->needmask, S, p->nb_state, p->ws.nbuse, 0);
    const uint32_t nhb = S * kMaxPlanes * g.nblk;
    hipLaunchKernelGGL(k_histlist, dim3((nhb + 255) / 256), dim3(256), 0, st, p->nzflag, p->ws.nbuse, g, nhb, p->ws.big_list, p->work_ctr + 2, p->psel);
    HIPCHK(p, hipGetLastError());
    if (int rc = phase_hist(p, S, st)) return rc;
    if (int rc = phase_tree(p, S, st)) return rc;
    return budget_pass_end(p, S, w.sizes, st);
}

// both tables on the general route: the two siblings' own sequences, one behind the other.  d_planar: the planar form -- the
// original of the figures is the matrix itself, and where w has an orig (bps < 4) the matrix cut to the sample width
static int total_tables_general(rspt_hip_packer* p, const void* d_src, const int32_t* d_planar, size_t nblocks, const double* ladder,
                                const LadderSel& ls, uint32_t* d_choice, const TotalWork& w, hipStream_t st) {
    const Geom& g = p->g;
    if (!d_planar) {
        if (int rc = rspt_hip_native_to_i32_batch_dev(p, d_src, w.t.orig, nblocks, (void*)st)) return rc;
    } else if (w.t.orig) {
        hipLaunchKernelGGL(k_planar_ingest, dim3((g.ns + 4095u) / 4096u, g.nch, (unsigned)nblocks), dim3(256), 0, st, d_planar, g, w.t.orig, (long long*)nullptr);
    }
    if (int rc = target_probes_general(p, w.t, ladder, ls.fwd.n, nblocks, st, d_planar)) return rc;
    return budget_sizes_general(p, d_src, nblocks, ls, d_choice, w.sizes, st, d_planar);
}

// Both entries.  Exactly one of d_src (native blocks, 16-byte aligned) and d_planar (the matrix, 4-byte aligned) is given.
static int compress_total(rspt_hip_packer* p, const void* d_src, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                          size_t total_bytes, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice, double* d_level, uint64_t* d_total,
                          double* d_prdn, uint64_t* d_cand_sizes, double* d_cand_figs, void* d_work, void* stream) {
    static_assert(sizeof(size_t) == sizeof(uint64_t), "total_bytes carries any uint64");
    if (!p || !(d_src || d_planar) || !d_dst || !d_sizes || !d_choice || !d_work || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_src) & 15) || (reinterpret_cast<uintptr_t>(d_planar) & 3) || (reinterpret_cast<uintptr_t>(d_choice) & 3) ||
        (reinterpret_cast<uintptr_t>(d_work) & 15) || (reinterpret_cast<uintptr_t>(d_level) & 7) || (reinterpret_cast<uintptr_t>(d_total) & 7) ||
        (reinterpret_cast<uintptr_t>(d_prdn) & 7) || (reinterpret_cast<uintptr_t>(d_cand_sizes) & 7) || (reinterpret_cast<uintptr_t>(d_cand_figs) & 7))
        return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    if (int rc = target_checks(p, nblocks, nladder)) return rc;
    LadderSel ls;
    if (int rc = make_ladder(p, ladder, nladder, d_choice, &ls)) return rc;
    if ((unsigned long long)dst_stride >> 32 >= p->g.nblk) return RSPT_HIP_ERR_ARG;  // (as rspt_hip_compress_batch_ladder_dev)
    const int route = total_route(p, nblocks, nladder);
    if (route < 0) return route;
    if (int rc = rspt_hip_reserve(p, nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const TotalWork w(p, d_work, nblocks, nladder, route == 1, d_planar != nullptr);
    if (int rc = route ? total_tables_fused(p, d_src, d_planar, nblocks, ls, w, st)
                       : total_tables_general(p, d_src, d_planar, nblocks, ladder, ls, d_choice, w, st))
        return rc;
    const uint32_t K = (uint32_t)nladder, B = (uint32_t)nblocks, cells = K * B;
    hipLaunchKernelGGL(k_total_figs, dim3((cells + 255) / 256), dim3(256), 0, st, (const double*)w.t.prdn, (const double*)w.t.mse, (const uint32_t*)w.t.path,
                       cells, w.figs);
    if (B <= kTotalWide) {
        const uint32_t nt = std::min(1024u, (B + 63u) & ~63u);  // block b < nt stays in the registers of thread b
        hipLaunchKernelGGL(k_total_level, dim3(1), dim3(nt), 0, st, (const unsigned long long*)w.sizes, (const unsigned long long*)w.figs, K, B,
                           (unsigned long long)total_bytes, w.res);
    } else {  // one workgroup would walk the table 64 times: a launch per round, the whole chip on each
        HIPCHK(p, hipMemsetAsync(w.slots(), 0, kTotalRounds * sizeof(TotalSlot), st));
        const uint32_t grid = std::min((B + 255u) / 256u, 2u * (uint32_t)p->num_cu);
        for (uint32_t r = 0; r < kTotalRounds; ++r)
            hipLaunchKernelGGL(k_total_round, dim3(grid), dim3(256), 0, st, (const unsigned long long*)w.sizes, (const unsigned long long*)w.figs, K, B,
                               (unsigned long long)total_bytes, r, w.res, w.slots() + r);
    }
    hipLaunchKernelGGL(k_total_pick, dim3((B + 255) / 256), dim3(256), 0, st, (const unsigned long long*)w.sizes, (const unsigned long long*)w.figs,
                       (const uint32_t*)w.t.path, K, B, (const unsigned long long*)w.res, d_choice, d_prdn, d_level, (unsigned long long*)d_total,
                       (unsigned long long*)d_cand_sizes, d_cand_figs);
    HIPCHK(p, hipGetLastError());
    return compress_batch_serial(p, d_src, nblocks, d_dst, dst_stride, d_sizes, st, d_planar, &ls);
}

int rspt_hip_compress_total_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder, size_t total_bytes,
                                      void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice, double* d_level, uint64_t* d_total,
                                      double* d_prdn, uint64_t* d_cand_sizes, double* d_cand_figs, void* d_work, void* stream) {
    return compress_total(p, d_src, nullptr, nblocks, ladder, nladder, total_bytes, d_dst, dst_stride, d_sizes, d_choice, d_level, d_total, d_prdn,
                          d_cand_sizes, d_cand_figs, d_work, stream);
}

// ---- the planar form -------------------------------------------------------------------------------------------------------------
int rspt_hip_compress_total_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    return total_work_bytes(p, nblocks, nladder, bytes, true);
}

int rspt_hip_compress_total_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                                             size_t total_bytes, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice, double* d_level,
                                             uint64_t* d_total, double* d_prdn, uint64_t* d_cand_sizes, double* d_cand_figs, void* d_work,
                                             void* stream) {
    return compress_total(p, nullptr, d_planar, nblocks, ladder, nladder, total_bytes, d_dst, dst_stride, d_sizes, d_choice, d_level, d_total, d_prdn,
                          d_cand_sizes, d_cand_figs, d_work, stream);
}
