// host_rate.hip -- the host frame of the rate-control entries: compress to a PRDN target (host_target.hip), to a byte budget per
// block (host_budget.hip) and to one byte total (host_total.hip), each from native blocks or from the planar int32 matrix.
// Included by rspt_hip.hip ahead of the three; the layout of their work areas is rate_work.hpp's.
//
// Every entry is rate_begin -- the refusals and the handle's preparation -- its own tables, its own rule kernel into d_choice, and
// rate_finish: rspt_hip_compress_batch_ladder_dev's path writes the chosen streams.  Every rule has a general route, which runs
// the siblings' own sequences once per ladder entry, and a faster one on hadamard rows of up to kTpMaxNs points, whose probe
// (probe_launch) reads each row once for all entries; where a probe leaves every entry's coefficients in nladder * nblocks block
// slots of ws.planar (slots_begin), ONE pass of the compressor up to k_tree runs over all of them (slots_pass).
enum RateRule { RATE_TARGET, RATE_BUDGET, RATE_TOTAL };
typedef bool (*RateFastOk)(const rspt_hip_packer* p, size_t nblocks, size_t nladder);  // a rule's faster route takes the call

// 1: the faster route, 0: the general one, < 0: a forced faster route on a call it does not take
static int rate_route(const rspt_hip_packer* p, RateRule rule, bool fast_ok) {
    const uint32_t forced = p->rate_route[rule];
    if (forced == 2) return fast_ok ? 1 : RSPT_HIP_ERR_UNSUPPORTED;
    return forced == 0 && fast_ok ? 1 : 0;
}

// rspt_hip_debug_set_*_route: a faster route is refused here on a shape that never takes it (fast_ok of one block and one entry),
// and what depends on the batch is each call's
static int rate_set_route(rspt_hip_packer* p, RateRule rule, int route, RateFastOk fast_ok) {
    if (!p || route < 0 || route > 2) return RSPT_HIP_ERR_ARG;
    if (route == 2 && !fast_ok(p, 1, 1)) return RSPT_HIP_ERR_UNSUPPORTED;
    p->rate_route[rule] = (uint32_t)route;
    return RSPT_HIP_OK;
}

// the refusals that come from the handle and the batch alone: the sizing calls make them too
static int rate_checks(const rspt_hip_packer* p, size_t nblocks, size_t nladder) {
    if (!p || nblocks == 0 || nblocks > 65535) return RSPT_HIP_ERR_ARG;  // (65535: rspt_hip_reserve)
    const Geom& g = p->g;
    if (g.kind != RSPT_HIP_KIND_HADAMARD && !(g.kind == RSPT_HIP_KIND_DCT && !p->dct_fft)) return RSPT_HIP_ERR_UNSUPPORTED;
    if (nladder < 1 || nladder > kMaxLadder) return RSPT_HIP_ERR_ARG;
    return RSPT_HIP_OK;
}

// a sizing call up to its layout -> the route (0 or 1), or the status to return
static int rate_sizing(const rspt_hip_packer* p, size_t nblocks, size_t nladder, const size_t* bytes, RateRule rule, RateFastOk fast_ok) {
    if (!bytes) return RSPT_HIP_ERR_ARG;
    if (int rc = rate_checks(p, nblocks, nladder)) return rc;
    return rate_route(p, rule, fast_ok(p, nblocks, nladder));
}

// One call.  The entry fills everything above `ls`; rate_begin checks it and fills the rest.
struct RateCall {
    rspt_hip_packer* p;
    const void* d_src;        // native blocks, 16-byte aligned ...
    const int32_t* d_planar;  // ... or the matrix, 4-byte aligned: exactly one of the two
    size_t nblocks;
    const double* ladder;
    size_t nladder;
    void* d_dst;
    size_t dst_stride;
    uint64_t* d_sizes;
    uint32_t* d_choice;
    void* d_work;
    hipStream_t st;
    LadderSel ls;
    int route;
};

static bool misaligned(const void* q, uintptr_t to) { return reinterpret_cast<uintptr_t>(q) & (to - 1); }

// Every shared refusal, in this order -- a call wrong in two ways returns the status of the first:
//   ARG          a pointer missing, no block; the source, d_choice or d_work misaligned; a handle with a feed open
//   rate_checks  ARG more than 65535 blocks, UNSUPPORTED the handle's kind, ARG the ladder's length
//   make_ladder  the ladder's values
//   ARG          !rule_ok, the entry's own refusal at this place (the target); the entry's optional pointers it checks itself,
//                ahead of this call -- ARG like everything up to rate_checks, so their place among those is free
//   ARG          dst_stride, as rspt_hip_compress_batch_ladder_dev
//   UNSUPPORTED  a forced faster route that does not take the call
// then rspt_hip_reserve for nblocks and the device.
static int rate_begin(RateCall& c, RateRule rule, RateFastOk fast_ok, bool rule_ok = true) {
    rspt_hip_packer* p = c.p;
    if (!p || !(c.d_src || c.d_planar) || !c.d_dst || !c.d_sizes || !c.d_choice || !c.d_work || c.nblocks == 0) return RSPT_HIP_ERR_ARG;
    if (misaligned(c.d_src, 16) || misaligned(c.d_planar, 4) || misaligned(c.d_choice, 4) || misaligned(c.d_work, 16)) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    if (int rc = rate_checks(p, c.nblocks, c.nladder)) return rc;
    if (int rc = make_ladder(p, c.ladder, c.nladder, c.d_choice, &c.ls)) return rc;
    if (!rule_ok) return RSPT_HIP_ERR_ARG;
    if ((unsigned long long)c.dst_stride >> 32 >= p->g.nblk) return RSPT_HIP_ERR_ARG;
    c.route = rate_route(p, rule, fast_ok(p, c.nblocks, c.nladder));
    if (c.route < 0) return c.route;
    if (int rc = rspt_hip_reserve(p, c.nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    return RSPT_HIP_OK;
}

// behind the rule kernel: the chosen streams
static int rate_finish(const RateCall& c) {
    HIPCHK(c.p, hipGetLastError());
    return compress_batch_serial(c.p, c.d_src, c.nblocks, c.d_dst, c.dst_stride, c.d_sizes, c.st, c.d_planar, &c.ls);
}

// the matrix cut to the sample width, as the planar front end ingests it
static void ingest_cut(const rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, int32_t* dst, hipStream_t st) {
    const Geom& g = p->g;
    hipLaunchKernelGGL(k_planar_ingest, dim3((g.ns + 4095u) / 4096u, g.nch, (unsigned)nblocks), dim3(256), 0, st, d_planar, g, dst, (long long*)nullptr);
}

// A rule's probe, one workgroup per row: the planar kernel on the caller's matrix, or the native one on the converted blocks.
// rows: the padded rows of LDS a workgroup holds -- 1 the transform, 2 the transform and its round trip, which is beyond the
// default limit at kTpMaxNs points.
template <class K, class... A>
static int probe_launch(rspt_hip_packer* p, K native, K planar, const int32_t* orig, const int32_t* d_planar, uint32_t rows, uint32_t B, hipStream_t st,
                        A... args) {
    const Geom& g = p->g;
    const K kern = d_planar ? planar : native;
    const uint32_t nt = std::max(64u, std::min(1024u, g.ns / kTpPer));
    const uint32_t lds = rows * tp_pad(g.ns) * (uint32_t)sizeof(uint32_t);
    if (rows > 1) HIPCHK(p, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(g.nch, B), dim3(nt), lds, st, d_planar ? d_planar : orig, g, args...);
    return RSPT_HIP_OK;
}

// The handle's bookkeeping behind a pass that ends with k_tree, and the sizes of its B slots.  A candidate's stream size is known
// behind k_tree -- k_layout only adds up what k_tree left in BlockMeta -- so k_budget_sizes adds up in k_layout's place.  Such a
// pass leaves the handle as compress_batch_serial's `psel & 512` branch does: the other copy of the zero region is ready (k_tree
// zeroed it) and becomes the next call's; and since neither k_layout has flagged nor k_encode wiped the planes the pass wrote,
// they count as unknown and the next front end flags them all.
static int pass_end(rspt_hip_packer* p, uint32_t B, unsigned long long* sizes, hipStream_t st) {
    const int zset_next = p->ws.zset ^ 1;
    p->ws.zero_ready[zset_next] = true;
    p->ws.zset = zset_next;
    p->ws.planes_unknown = true;
    hipLaunchKernelGGL(k_budget_sizes, dim3(B), dim3(64), 0, st, p->g, (const uint32_t*)p->ws.nbuse, (const BlockMeta*)p->ws.meta, sizes);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

// The workspace for S = nladder * nblocks block slots -- entry k of block b is slot k * nblocks + b -- with a front end begun on
// them.  *orig: native blocks are converted into the last entry's slots, where a probe reads each row before it writes it; the
// matrix needs no place (the planar probes cut it on load: no row of ws.planar is read, every slot is only written).
static int slots_begin(const RateCall& c, uint32_t* S, const int32_t** orig) {
    rspt_hip_packer* p = c.p;
    *S = c.ls.fwd.n * (uint32_t)c.nblocks;
    if (int rc = rspt_hip_reserve(p, *S)) return rc;
    if (int rc = front_begin(p, *S, c.st)) return rc;
    int32_t* last = p->ws.planar + (size_t)(*S - (uint32_t)c.nblocks) * p->g.N;
    *orig = last;
    return c.d_planar ? RSPT_HIP_OK : rspt_hip_native_to_i32_batch_dev(p, c.d_src, last, c.nblocks, (void*)c.st);
}

// What phase_front runs behind a lossy packer's transform, then the compressor up to k_tree, over S slots at once -> their sizes
static int slots_pass(rspt_hip_packer* p, uint32_t S, unsigned long long* sizes, hipStream_t st) {
    const Geom& g = p->g;
    hipLaunchKernelGGL((k_planar_planes<false>), dim3((g.N + 4095) / 4096, S), dim3(256), 0, st, p->ws.planar, g, (uint32_t)p->nb_host, p->ws.planes,
                       p->nzflag, (uint32_t*)nullptr);
    hipLaunchKernelGGL(k_nb_scan, dim3(1), dim3(1024), 0, st, p->needmask, S, p->nb_state, p->ws.nbuse, 0);
    const uint32_t nhb = S * kMaxPlanes * g.nblk;
    hipLaunchKernelGGL(k_histlist, dim3((nhb + 255) / 256), dim3(256), 0, st, p->nzflag, p->ws.nbuse, g, nhb, p->ws.big_list, p->work_ctr + 2, p->psel);
    HIPCHK(p, hipGetLastError());
    if (int rc = phase_hist(p, S, st)) return rc;
    if (int rc = phase_tree(p, S, st)) return rc;
    return pass_end(p, S, sizes, st);
}

// The handle's quantiser fields for the length of a scope: the general probes run every candidate under its own quantiser by
// setting the fields the launches read (kernel arguments: nothing of it outlives them), and the handle has its own again on
// every way out.
class QuantizerScope {
    rspt_hip_packer* p;
    const Quantizer q;
    const double quality;
    const bool had_quant;

  public:
    explicit QuantizerScope(rspt_hip_packer* p)
        : p(p), q{p->dct_scale0, p->dct_scale1, p->idct_scale, p->dct_cs0, p->had_div_fwd, p->had_div_inv}, quality(p->quality), had_quant(p->had_quant) {}
    QuantizerScope(const QuantizerScope&) = delete;
    QuantizerScope& operator=(const QuantizerScope&) = delete;
    ~QuantizerScope() {
        p->dct_scale0 = q.dct_scale0, p->dct_scale1 = q.dct_scale1, p->idct_scale = q.idct_scale, p->dct_cs0 = q.dct_cs0;
        p->had_div_fwd = q.had_div_fwd, p->had_div_inv = q.had_div_inv, p->had_quant = had_quant, p->quality = quality;
    }
};
