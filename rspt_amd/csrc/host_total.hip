// host_total.hip -- compress a batch to one byte total (rspt_hip.h: rspt_hip_compress_total_batch_dev and its planar form,
// rspt_hip_compress_total_planar_batch_dev), included by rspt_hip.hip behind host_rate.hip, whose frame both go through.
//
// The two tables of the siblings -- every candidate's stream size (host_budget.hip) and every candidate's PRDN figure
// (host_target.hip) -- are filled for one batch, and k_total_figs / k_total_level / k_total_pick (total.hip) apply the rule on
// the device.  The work area is rate_work::Total (rate_work.hpp): figs holds the figures as bit patterns (k_total_figs), res T*,
// cost(T*) and the lower bound between the level kernels and k_total_pick, its slots a round's sums (k_total_round).
// Two routes (rspt_hip_debug_set_total_route overrides the host's pick for the tests):
//   general  every shape the ladder takes: the target entry's probes per ladder entry (target_probes_general), then the budget
//            entry's passes per ladder entry (budget_sizes_general) -- two forward transforms per entry, each inside its own
//            sequence, so that neither sequence's bookkeeping changes.  The area holds the target entry's whole scratch; from the
//            matrix at bps 4, where the matrix is the original of the figures, one copy of the batch less
//   fused    where the target entry's fused probe and the budget entry's batched route both take the call: k_total_probe --
//            k_planar_total_probe on the matrix -- reads each row once for both tables, k_q_finish finishes its sums, and one
//            slots_pass follows.  The area holds no scratch, from either source
struct TotalWork {
    unsigned long long *sizes, *figs, *res;
    TotalSlot* slots;
    TargetWork t;
    TotalWork(const rate_work::Total& l, uint8_t* base)
        : sizes((unsigned long long*)(base + l.sizes)),
          figs((unsigned long long*)(base + l.figs)),
          res((unsigned long long*)(base + l.res)),
          slots((TotalSlot*)(base + l.res + rate_work::kTotalSlots)),
          t(l.t, base + l.head, base + l.tab) {}
};
static_assert(rate_work::kTotalSlots + kTotalRounds * sizeof(TotalSlot) == rate_work::kTotalResBytes, "res and the rounds' slots");

static bool total_fused_ok(const rspt_hip_packer* p, size_t nblocks, size_t nladder) {
    return target_fused_ok(p) && budget_batched_ok(p, nblocks, nladder);
}

int rspt_hip_debug_set_total_route(rspt_hip_packer* p, int route) { return rate_set_route(p, RATE_TOTAL, route, total_fused_ok); }

static int total_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes, bool planar) {
    const int route = rate_sizing(p, nblocks, nladder, bytes, RATE_TOTAL, total_fused_ok);
    if (route < 0) return route;
    const Geom& g = p->g;
    *bytes = rate_work::Total(g.N, g.nblk, g.bps, nblocks, nladder, route == 1, planar).bytes;
    return RSPT_HIP_OK;
}

int rspt_hip_compress_total_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    return total_work_bytes(p, nblocks, nladder, bytes, false);
}

int rspt_hip_compress_total_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes) {
    return total_work_bytes(p, nblocks, nladder, bytes, true);
}

// both tables on the fused route
static int total_tables_fused(const RateCall& c, const TotalWork& w) {
    rspt_hip_packer* p = c.p;
    const uint32_t B = (uint32_t)c.nblocks;
    uint32_t S;
    const int32_t* orig;
    if (int rc = slots_begin(c, &S, &orig)) return rc;
    HIPCHK(p, hipMemsetAsync(w.t.acc, 0, (size_t)S * 4 * sizeof(unsigned long long), c.st));
    if (int rc = probe_launch(p, k_total_probe, k_planar_total_probe, orig, c.d_planar, 2, B, c.st, c.ls.fwd, c.ls.inv, (uint32_t)p->nb_host, B,
                              (int32_t*)p->ws.planar, w.t.acc))
        return rc;
    hipLaunchKernelGGL(k_q_finish, dim3((S + 255) / 256), dim3(256), 0, c.st, (const unsigned long long*)w.t.acc, S, w.t.flag, w.t.prdn, w.t.mse,
                       (double*)nullptr, w.t.path);
    return slots_pass(p, S, w.sizes, c.st);
}

// both tables on the general route: the two siblings' own sequences, one behind the other
static int total_tables_general(const RateCall& c, const TotalWork& w) {
    if (!c.d_planar)
        if (int rc = rspt_hip_native_to_i32_batch_dev(c.p, c.d_src, w.t.orig, c.nblocks, (void*)c.st)) return rc;
    if (int rc = target_probes_general(c.p, w.t, c.ladder, c.ls.fwd.n, c.nblocks, c.st, c.d_planar)) return rc;
    return budget_sizes_general(c, w.sizes);
}

// Both entries.  d_level, d_total, d_prdn, d_cand_sizes and d_cand_figs are the entry's own optional pointers.
static int compress_total(RateCall c, size_t total_bytes, double* d_level, uint64_t* d_total, double* d_prdn, uint64_t* d_cand_sizes, double* d_cand_figs) {
    static_assert(sizeof(size_t) == sizeof(uint64_t), "total_bytes carries any uint64");
    if (misaligned(d_level, 8) || misaligned(d_total, 8) || misaligned(d_prdn, 8) || misaligned(d_cand_sizes, 8) || misaligned(d_cand_figs, 8))
        return RSPT_HIP_ERR_ARG;
    if (int rc = rate_begin(c, RATE_TOTAL, total_fused_ok)) return rc;
    rspt_hip_packer* p = c.p;
    const Geom& g = p->g;
    hipStream_t st = c.st;
    const TotalWork w(rate_work::Total(g.N, g.nblk, g.bps, c.nblocks, c.nladder, c.route == 1, c.d_planar != nullptr), (uint8_t*)c.d_work);
    if (int rc = c.route ? total_tables_fused(c, w) : total_tables_general(c, w)) return rc;
    const uint32_t K = (uint32_t)c.nladder, B = (uint32_t)c.nblocks, cells = K * B;
    hipLaunchKernelGGL(k_total_figs, dim3((cells + 255) / 256), dim3(256), 0, st, (const double*)w.t.prdn, (const double*)w.t.mse, (const uint32_t*)w.t.path,
                       cells, w.figs);
    if (B <= kTotalWide) {
        const uint32_t nt = std::min(1024u, (B + 63u) & ~63u);  // block b < nt stays in the registers of thread b
        hipLaunchKernelGGL(k_total_level, dim3(1), dim3(nt), 0, st, (const unsigned long long*)w.sizes, (const unsigned long long*)w.figs, K, B,
                           (unsigned long long)total_bytes, w.res);
    } else {  // one workgroup would walk the table 64 times: a launch per round, the whole chip on each
        HIPCHK(p, hipMemsetAsync(w.slots, 0, kTotalRounds * sizeof(TotalSlot), st));
        const uint32_t grid = std::min((B + 255u) / 256u, 2u * (uint32_t)p->num_cu);
        for (uint32_t r = 0; r < kTotalRounds; ++r)
            hipLaunchKernelGGL(k_total_round, dim3(grid), dim3(256), 0, st, (const unsigned long long*)w.sizes, (const unsigned long long*)w.figs, K, B,
                               (unsigned long long)total_bytes, r, w.res, w.slots + r);
    }
    hipLaunchKernelGGL(k_total_pick, dim3((B + 255) / 256), dim3(256), 0, st, (const unsigned long long*)w.sizes, (const unsigned long long*)w.figs,
                       (const uint32_t*)w.t.path, K, B, (const unsigned long long*)w.res, c.d_choice, d_prdn, d_level, (unsigned long long*)d_total,
                       (unsigned long long*)d_cand_sizes, d_cand_figs);
    return rate_finish(c);
}

int rspt_hip_compress_total_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder, size_t total_bytes,
                                      void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice, double* d_level, uint64_t* d_total,
                                      double* d_prdn, uint64_t* d_cand_sizes, double* d_cand_figs, void* d_work, void* stream) {
    return compress_total({p, d_src, nullptr, nblocks, ladder, nladder, d_dst, dst_stride, d_sizes, d_choice, d_work, (hipStream_t)stream}, total_bytes,
                          d_level, d_total, d_prdn, d_cand_sizes, d_cand_figs);
}

int rspt_hip_compress_total_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                                             size_t total_bytes, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice, double* d_level,
                                             uint64_t* d_total, double* d_prdn, uint64_t* d_cand_sizes, double* d_cand_figs, void* d_work,
                                             void* stream) {
    return compress_total({p, nullptr, d_planar, nblocks, ladder, nladder, d_dst, dst_stride, d_sizes, d_choice, d_work, (hipStream_t)stream}, total_bytes,
                          d_level, d_total, d_prdn, d_cand_sizes, d_cand_figs);
}
