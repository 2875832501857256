// host_budget.hip -- compress to a byte budget (rspt_hip.h: rspt_hip_compress_budget_batch_dev and its planar form,
// rspt_hip_compress_budget_planar_batch_dev), included by rspt_hip.hip behind host_rate.hip, whose frame both go through.
//
// The candidates run a compress call up to k_tree and k_budget_sizes (budget.hip) adds up in k_layout's place (host_rate.hip:
// pass_end): no k_layout, no k_encode, no byte of a candidate's stream.  k_budget_select applies the rule.
//
// The caller's d_work: the table of sizes (rate_work::budget_bytes), and nothing else on either route or from either source.
// Two routes (rspt_hip_debug_set_budget_route overrides the host's pick for the tests):
//   general  every shape the ladder takes: per entry k one pass of phase_front / phase_hist / phase_tree as a ladder call whose
//            every choice is k -- d_choice, which the call owns until k_budget_select writes it, is filled with k.  The planar
//            front end ingests the matrix per entry, cutting it to the sample width, and again in the final pass
//   batched  hadamard rows of up to kTpMaxNs points with nladder * nblocks <= 65535 block slots (rspt_hip_reserve's bound):
//            k_budget_probe -- k_planar_budget_probe on the matrix -- reads each row once and writes entry k's coefficients of
//            block b into its slot, and one slots_pass follows

// where the batched route runs
static bool budget_batched_ok(const rspt_hip_packer* p, size_t nblocks, size_t nladder) {
    const Geom& g = p->g;
    return g.kind == RSPT_HIP_KIND_HADAMARD && g.ns <= kTpMaxNs && nladder * nblocks <= 65535;
}

int rspt_hip_debug_set_budget_route(rspt_hip_packer* p, int route) { return rate_set_route(p, RATE_BUDGET, route, budget_batched_ok); }

int rspt_hip_compress_budget_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    if (int r = rate_sizing(p, nblocks, nladder, bytes, RATE_BUDGET, budget_batched_ok); r < 0) return r;
    *bytes = rate_work::budget_bytes(nblocks, nladder);
    return RSPT_HIP_OK;
}

int rspt_hip_compress_budget_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    return rspt_hip_compress_budget_work_bytes(p, nblocks, nladder, bytes);
}

static int budget_sizes_general(const RateCall& c, unsigned long long* tab) {
    rspt_hip_packer* p = c.p;
    const uint32_t B = (uint32_t)c.nblocks;
    for (uint32_t k = 0; k < c.ls.fwd.n; ++k) {
        HIPCHK(p, hipMemsetD32Async((hipDeviceptr_t)c.d_choice, (int)k, c.nblocks, c.st));
        if (int rc = phase_front(p, (const uint8_t*)c.d_src, c.nblocks, c.st, c.d_planar, &c.ls)) return rc;
        if (int rc = phase_hist(p, B, c.st)) return rc;
        if (int rc = phase_tree(p, B, c.st)) return rc;
        if (int rc = pass_end(p, B, tab + (size_t)k * c.nblocks, c.st)) return rc;
    }
    return RSPT_HIP_OK;
}

static int budget_sizes_batched(const RateCall& c, unsigned long long* tab) {
    rspt_hip_packer* p = c.p;
    uint32_t S;
    const int32_t* orig;
    if (int rc = slots_begin(c, &S, &orig)) return rc;
    if (int rc = probe_launch(p, k_budget_probe, k_planar_budget_probe, orig, c.d_planar, 1, (uint32_t)c.nblocks, c.st, c.ls.fwd, (uint32_t)c.nblocks,
                              (int32_t*)p->ws.planar))
        return rc;
    return slots_pass(p, S, tab, c.st);
}

// Both entries.  d_budget and d_cand_sizes are the entry's own optional pointers.
static int compress_budget(RateCall c, size_t budget_bytes, const uint64_t* d_budget, uint64_t* d_cand_sizes) {
    static_assert(sizeof(size_t) == sizeof(uint64_t), "budget_bytes carries any uint64");
    if (misaligned(d_budget, 8) || misaligned(d_cand_sizes, 8)) return RSPT_HIP_ERR_ARG;
    if (int rc = rate_begin(c, RATE_BUDGET, budget_batched_ok)) return rc;
    unsigned long long* tab = (unsigned long long*)c.d_work;
    if (int rc = c.route ? budget_sizes_batched(c, tab) : budget_sizes_general(c, tab)) return rc;
    hipLaunchKernelGGL(k_budget_select, dim3(((uint32_t)c.nblocks + 255) / 256), dim3(256), 0, c.st, (const unsigned long long*)tab, (uint32_t)c.nladder,
                       (uint32_t)c.nblocks, (unsigned long long)budget_bytes, (const unsigned long long*)d_budget, c.d_choice,
                       (unsigned long long*)d_cand_sizes);
    return rate_finish(c);
}

int rspt_hip_compress_budget_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder,
                                       size_t budget_bytes, const uint64_t* d_budget, void* d_dst, size_t dst_stride, uint64_t* d_sizes,
                                       uint32_t* d_choice, uint64_t* d_cand_sizes, void* d_work, void* stream) {
    return compress_budget({p, d_src, nullptr, nblocks, ladder, nladder, d_dst, dst_stride, d_sizes, d_choice, d_work, (hipStream_t)stream}, budget_bytes,
                           d_budget, d_cand_sizes);
}

int rspt_hip_compress_budget_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                                              size_t budget_bytes, const uint64_t* d_budget, void* d_dst, size_t dst_stride, uint64_t* d_sizes,
                                              uint32_t* d_choice, uint64_t* d_cand_sizes, void* d_work, void* stream) {
    return compress_budget({p, nullptr, d_planar, nblocks, ladder, nladder, d_dst, dst_stride, d_sizes, d_choice, d_work, (hipStream_t)stream}, budget_bytes,
                           d_budget, d_cand_sizes);
}
