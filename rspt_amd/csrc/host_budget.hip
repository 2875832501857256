// host_budget.hip -- compress to a byte budget (rspt_hip.h: rspt_hip_compress_budget_batch_dev and its planar form,
// rspt_hip_compress_budget_planar_batch_dev), included by rspt_hip.hip.
//
// A candidate's stream size is known behind k_tree -- k_layout only adds up what k_tree left in BlockMeta -- so the candidates run
// a compress call up to k_tree and k_budget_sizes (budget.hip) adds up in k_layout's place: no k_layout, no k_encode, no byte of
// a candidate's stream.  k_budget_select applies the rule and rspt_hip_compress_batch_ladder_dev's path writes the chosen streams.
//
// The caller's d_work: the table of sizes, [nladder][nblocks] uint64, and nothing else on either route.
// Two routes (rspt_hip_debug_set_budget_route overrides the host's pick for the tests):
//   general  every shape the ladder takes: per entry k one pass of phase_front / phase_hist / phase_tree as a ladder call whose
//            every choice is k -- d_choice, which the call owns until k_budget_select writes it, is filled with k
//   batched  hadamard rows of up to kTpMaxNs points with nladder * nblocks <= 65535 block slots (rspt_hip_reserve's bound): the
//            workspace is reserved for that many slots, k_budget_probe reads each row once and writes entry k's coefficients of
//            block b into slot k * nblocks + b of ws.planar, and ONE pass of k_planar_planes / k_nb_scan / k_histlist / k_hist /
//            k_tree runs over all slots.  The converted blocks lie in the last entry's slots until the probe has read them.
// The planar form is the same body (compress_budget) with the caller's matrix as the source, and the same d_work:
//   general  the planar front end ingests the matrix per entry, cutting it to the sample width, and again in the final pass
//   batched  k_planar_budget_probe reads each row from the matrix, cutting it on load: no converter pass, no original inside
//            ws.planar -- nothing but the probe reads the matrix and every slot is only written
// A pass that stops behind k_tree leaves the handle as compress_batch_serial's `psel & 512` branch does: the other copy of the zero
// region is ready (k_tree zeroed it) and becomes the next call's; and since neither k_layout has flagged nor k_encode wiped the
// planes the pass wrote, they count as unknown and the next front end flags them all.
static size_t budget_tab_bytes(size_t nblocks, size_t nladder) { return (nladder * nblocks * sizeof(uint64_t) + 255) & ~(size_t)255; }

// where the batched route runs
static bool budget_batched_ok(const rspt_hip_packer* p, size_t nblocks, size_t nladder) {
    const Geom& g = p->g;
    return g.kind == RSPT_HIP_KIND_HADAMARD && g.ns <= kTpMaxNs && nladder * nblocks <= 65535;
}

// 1: the batched route, 0: the general one, < 0: a forced batched route on a call it does not take
static int budget_route(const rspt_hip_packer* p, size_t nblocks, size_t nladder) {
    const bool ok = budget_batched_ok(p, nblocks, nladder);
    if (p->budget_route == 2) return ok ? 1 : RSPT_HIP_ERR_UNSUPPORTED;
    return p->budget_route == 0 && ok ? 1 : 0;
}

int rspt_hip_debug_set_budget_route(rspt_hip_packer* p, int route) {
    if (!p || route < 0 || route > 2) return RSPT_HIP_ERR_ARG;
    if (route == 2 && !budget_batched_ok(p, 1, 1)) return RSPT_HIP_ERR_UNSUPPORTED;  // (the shape; the slot bound is each call's)
    p->budget_route = (uint32_t)route;
    return RSPT_HIP_OK;
}

int rspt_hip_compress_budget_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    if (!bytes) return RSPT_HIP_ERR_ARG;
    if (int rc = target_checks(p, nblocks, nladder)) return rc;
    if (int r = budget_route(p, nblocks, nladder); r < 0) return r;
    *bytes = budget_tab_bytes(nblocks, nladder);
    return RSPT_HIP_OK;
}

// the handle's bookkeeping behind a pass that ends with k_tree, and the sizes of its B slots
static int budget_pass_end(rspt_hip_packer* p, uint32_t B, unsigned long long* sizes, hipStream_t st) {
    const int zset_next = p->ws.zset ^ 1;
    p->ws.zero_ready[zset_next] = true;
    p->ws.zset = zset_next;
    p->ws.planes_unknown = true;
    hipLaunchKernelGGL(k_budget_sizes, dim3(B), dim3(64), 0, st, p->g, (const uint32_t*)p->ws.nbuse, (const BlockMeta*)p->ws.meta, sizes);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

// d_planar: the planar form -- the planar front end ingests the caller's matrix, cutting it, where the native one reads d_src
static int budget_sizes_general(rspt_hip_packer* p, const void* d_src, size_t nblocks, const LadderSel& ls, uint32_t* d_choice,
                                unsigned long long* tab, hipStream_t st, const int32_t* d_planar) {
    const uint32_t B = (uint32_t)nblocks;
    for (uint32_t k = 0; k < ls.fwd.n; ++k) {
        HIPCHK(p, hipMemsetD32Async((hipDeviceptr_t)d_choice, (int)k, nblocks, st));
        if (int rc = phase_front(p, (const uint8_t*)d_src, nblocks, st, d_planar, &ls)) return rc;
        if (int rc = phase_hist(p, B, st)) return rc;
        if (int rc = phase_tree(p, B, st)) return rc;
        if (int rc = budget_pass_end(p, B, tab + (size_t)k * nblocks, st)) return rc;
    }
    return RSPT_HIP_OK;
}

// d_planar: the planar form -- k_planar_budget_probe on the caller's matrix: no converter pass, and no row of ws.planar is read
static int budget_sizes_batched(rspt_hip_packer* p, const void* d_src, size_t nblocks, const LadderSel& ls, unsigned long long* tab,
                                hipStream_t st, const int32_t* d_planar) {
    const Geom& g = p->g;
    const uint32_t B = (uint32_t)nblocks, S = ls.fwd.n * B;  // block slots: entry k of block b is slot k * B + b
    if (int rc = rspt_hip_reserve(p, S)) return rc;
    if (int rc = front_begin(p, S, st)) return rc;
    const uint32_t nt = std::max(64u, std::min(1024u, g.ns / kTpPer));
    const uint32_t lds = tp_pad(g.ns) * (uint32_t)sizeof(uint32_t);
    if (d_planar) {
        hipLaunchKernelGGL(k_planar_budget_probe, dim3(g.nch, B), dim3(nt), lds, st, d_planar, g, ls.fwd, B, (int32_t*)p->ws.planar);
    } else {
        int32_t* orig = p->ws.planar + (size_t)(S - B) * g.N;  // the last entry's slots: each row is read before it is written
        if (int rc = rspt_hip_native_to_i32_batch_dev(p, d_src, orig, nblocks, (void*)st)) return rc;
        hipLaunchKernelGGL(k_budget_probe, dim3(g.nch, B), dim3(nt), lds, st, (const int32_t*)orig, g, ls.fwd, B, (int32_t*)p->ws.planar);
    }
    // from here on what phase_front runs behind a lossy packer's transform, over all slots
    hipLaunchKernelGGL((k_planar_planes<false>), dim3((g.N + 4095) / 4096, S), dim3(256), 0, st, p->ws.planar, g, (uint32_t)p->nb_host, p->ws.planes,
                       p->nzflag, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_nb_scan, dim3(1), dim3(1024), 0, st, p->needmask, S, p->nb_state, p->ws.nbuse, 0);
    const uint32_t nhb = S * kMaxPlanes * g.nblk;
    hipLaunchKernelGGL(k_histlist, dim3((nhb + 255) / 256), dim3(256), 0, st, p->nzflag, p->ws.nbuse, g, nhb, p->ws.big_list, p->work_ctr + 2, p->psel);
    HIPCHK(p, hipGetLastError());
    if (int rc = phase_hist(p, S, st)) return rc;
    if (int rc = phase_tree(p, S, st)) return rc;
    return budget_pass_end(p, S, tab, st);
}

// Both entries.  Exactly one of d_src (native blocks, 16-byte aligned) and d_planar (the matrix, 4-byte aligned) is given.
static int compress_budget(rspt_hip_packer* p, const void* d_src, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                           size_t budget_bytes, const uint64_t* d_budget, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice,
                           uint64_t* d_cand_sizes, void* d_work, void* stream) {
    static_assert(sizeof(size_t) == sizeof(uint64_t), "budget_bytes carries any uint64");
    if (!p || !(d_src || d_planar) || !d_dst || !d_sizes || !d_choice || !d_work || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_src) & 15) || (reinterpret_cast<uintptr_t>(d_planar) & 3) || (reinterpret_cast<uintptr_t>(d_choice) & 3) ||
        (reinterpret_cast<uintptr_t>(d_budget) & 7) || (reinterpret_cast<uintptr_t>(d_cand_sizes) & 7) || (reinterpret_cast<uintptr_t>(d_work) & 15))
        return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    if (int rc = target_checks(p, nblocks, nladder)) return rc;
    LadderSel ls;
    if (int rc = make_ladder(p, ladder, nladder, d_choice, &ls)) return rc;
    if ((unsigned long long)dst_stride >> 32 >= p->g.nblk) return RSPT_HIP_ERR_ARG;  // (as rspt_hip_compress_batch_ladder_dev)
    const int route = budget_route(p, nblocks, nladder);
    if (route < 0) return route;
    if (int rc = rspt_hip_reserve(p, nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* tab = (unsigned long long*)d_work;
    if (int rc = route ? budget_sizes_batched(p, d_src, nblocks, ls, tab, st, d_planar)
                       : budget_sizes_general(p, d_src, nblocks, ls, d_choice, tab, st, d_planar))
        return rc;
    hipLaunchKernelGGL(k_budget_select, dim3(((uint32_t)nblocks + 255) / 256), dim3(256), 0, st, (const unsigned long long*)tab, (uint32_t)nladder,
                       (uint32_t)nblocks, (unsigned long long)budget_bytes, (const unsigned long long*)d_budget, d_choice,
                       (unsigned long long*)d_cand_sizes);
    HIPCHK(p, hipGetLastError());
    return compress_batch_serial(p, d_src, nblocks, d_dst, dst_stride, d_sizes, st, d_planar, &ls);
}

int rspt_hip_compress_budget_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder,
                                       size_t budget_bytes, const uint64_t* d_budget, void* d_dst, size_t dst_stride, uint64_t* d_sizes,
                                       uint32_t* d_choice, uint64_t* d_cand_sizes, void* d_work, void* stream) {
    return compress_budget(p, d_src, nullptr, nblocks, ladder, nladder, budget_bytes, d_budget, d_dst, dst_stride, d_sizes, d_choice, d_cand_sizes,
                           d_work, stream);
}

// ---- the planar form -------------------------------------------------------------------------------------------------------------
// (the size table is the whole work area on either route, whatever the source layout)
int rspt_hip_compress_budget_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    return rspt_hip_compress_budget_work_bytes(p, nblocks, nladder, bytes);
}

int rspt_hip_compress_budget_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                                              size_t budget_bytes, const uint64_t* d_budget, void* d_dst, size_t dst_stride, uint64_t* d_sizes,
                                              uint32_t* d_choice, uint64_t* d_cand_sizes, void* d_work, void* stream) {
    return compress_budget(p, nullptr, d_planar, nblocks, ladder, nladder, budget_bytes, d_budget, d_dst, dst_stride, d_sizes, d_choice,
                           d_cand_sizes, d_work, stream);
}
