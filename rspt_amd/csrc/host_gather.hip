// host_gather.hip: multi-GPU gather over RCCL.  RCCL is bound at run time: a process that never gathers (the C++ drop-in on one
// GPU, the tests on the CPU box) does not load it.  A communicator must never cross library instances -- an ncclComm_t made by one
// copy of RCCL is garbage to another (PyTorch wheels bundle their own librccl.so next to /opt/rocm's) -- so the binding goes to the
// copy the process has ALREADY mapped (that is where the caller's ncclComm_t came from); only a process without any gets
// librccl.so.1 from the loader's path; a process with two different copies mapped is refused unless RSPT_RCCL_LIB names the one.
namespace {
struct Rccl {
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*Send)(const void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    bool ok = false;
};
constexpr int kNcclUint8 = 1, kNcclUint64 = 5;  // ncclDataType_t (rccl.h)
int collect_rccl(struct dl_phdr_info* info, size_t, void* data) {
    auto* v = static_cast<std::vector<std::string>*>(data);
    if (info->dlpi_name && strstr(info->dlpi_name, "librccl.so")) {
        char real[PATH_MAX];
        const std::string path = realpath(info->dlpi_name, real) ? real : info->dlpi_name;
        bool seen = false;
        for (const auto& q : *v) seen = seen || q == path;
        if (!seen) v->push_back(path);
    }
    return 0;
}
}  // namespace
static const Rccl& rccl() {
    static Rccl r = [] {
        Rccl q;
        void* h = nullptr;
        if (const char* want = getenv("RSPT_RCCL_LIB")) {
            h = dlopen(want, RTLD_NOW | RTLD_LOCAL);
        } else {
            std::vector<std::string> mapped;
            dl_iterate_phdr(collect_rccl, &mapped);
            if (mapped.size() > 1) return q;  // two copies in one process: which one made the caller's communicator is not ours to guess
            if (mapped.size() == 1) {
                h = dlopen(mapped[0].c_str(), RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL);  // the instance already in the process
            } else {
                h = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
                if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
            }
        }
        if (!h) return q;
        q.AllGather = reinterpret_cast<decltype(q.AllGather)>(dlsym(h, "ncclAllGather"));
        q.Send = reinterpret_cast<decltype(q.Send)>(dlsym(h, "ncclSend"));
        q.Recv = reinterpret_cast<decltype(q.Recv)>(dlsym(h, "ncclRecv"));
        q.GroupStart = reinterpret_cast<decltype(q.GroupStart)>(dlsym(h, "ncclGroupStart"));
        q.GroupEnd = reinterpret_cast<decltype(q.GroupEnd)>(dlsym(h, "ncclGroupEnd"));
        q.ok = q.AllGather && q.Send && q.Recv && q.GroupStart && q.GroupEnd;
        return q;
    }();
    return r;
}

int rspt_hip_gather_sizes(rspt_hip_packer* p, void* comm, int world, const uint64_t* d_total, uint64_t* d_totals, uint64_t* h_totals, void* stream) {
    if (!p || !comm || world < 1 || !d_total || !d_totals) return RSPT_HIP_ERR_ARG;
    const Rccl& R = rccl();
    if (!R.ok) return RSPT_HIP_ERR_UNSUPPORTED;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    if (R.AllGather(d_total, d_totals, 1, kNcclUint64, comm, st) != 0) return RSPT_HIP_ERR_LAUNCH;
    if (h_totals) HIPCHK(p, hipMemcpyAsync(h_totals, d_totals, (size_t)world * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    return RSPT_HIP_OK;
}

int rspt_hip_gather_payload(rspt_hip_packer* p, void* comm, int rank, int world, int root, const void* d_packed, const uint64_t* h_totals,
                            void* d_recv, size_t recv_stride, void* stream) {
    if (!p || !comm || world < 1 || rank < 0 || rank >= world || root < 0 || root >= world || !d_packed || !h_totals) return RSPT_HIP_ERR_ARG;
    if (rank == root && !d_recv) return RSPT_HIP_ERR_ARG;
    if (recv_stride & 15) return RSPT_HIP_ERR_ARG;  // (every rank's container must land 16-byte aligned: rspt_hip_decompress_packed_dev)
    const Rccl& R = rccl();
    if (!R.ok) return RSPT_HIP_ERR_UNSUPPORTED;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    for (int r = 0; r < world; ++r)
        if (h_totals[r] > recv_stride) return RSPT_HIP_ERR_DST_TOO_SMALL;  // (every rank sees the same sizes and the same stride: nobody posts anything)
    // one group: the root's receives and the peers' sends are matched pairwise, straight over each peer's own link to the root
    if (R.GroupStart() != 0) return RSPT_HIP_ERR_LAUNCH;
    int rc = 0;
    if (rank == root) {
        for (int r = 0; r < world && !rc; ++r)
            if (r != root && h_totals[r]) rc = R.Recv((uint8_t*)d_recv + (size_t)r * recv_stride, (size_t)h_totals[r], kNcclUint8, r, comm, st);
    } else if (h_totals[rank]) {
        rc = R.Send(d_packed, (size_t)h_totals[rank], kNcclUint8, root, comm, st);
    }
    if (R.GroupEnd() != 0 || rc) return RSPT_HIP_ERR_LAUNCH;
    if (rank == root && h_totals[root])
        HIPCHK(p, hipMemcpyAsync((uint8_t*)d_recv + (size_t)root * recv_stride, d_packed, (size_t)h_totals[root], hipMemcpyDeviceToDevice, st));
    return RSPT_HIP_OK;
}

int rspt_hip_gather_containers(rspt_hip_packer* p, void* comm, int rank, int world, int root, const void* d_packed, const uint64_t* d_total,
                               void* d_recv, size_t recv_stride, uint64_t* h_totals, void* stream) {
    if (!p || !h_totals || world < 1) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    if (p->gat_world < world) {  // (a few words, kept with the handle)
        p->gat_world = 0;
        if (hipMalloc(p->gat_totals.out(), (size_t)world * sizeof(uint64_t)) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
        p->gat_world = world;
    }
    uint64_t* d_all = p->gat_totals;
    int rc = rspt_hip_gather_sizes(p, comm, world, d_total, d_all, h_totals, stream);
    if (rc == RSPT_HIP_OK && hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = RSPT_HIP_ERR_LAUNCH;  // the sizes are on the host now
    if (rc == RSPT_HIP_OK) rc = rspt_hip_gather_payload(p, comm, rank, world, root, d_packed, h_totals, d_recv, recv_stride, stream);
    return rc;
}

// The same gather without a host synchronisation in the step (what rspt_amd/shard.py LaggedGather does over torch.distributed):
// the sizes of step i travel by a device all-gather and a copy into page-locked memory of the handle, on the handle's own gather
// stream behind an event on `stream`; the host reads them when it posts the payload -- one step later, when they have long
// arrived -- again on the gather stream, so that the payload of step i overlaps the kernels of step i + 1.
static int gather_lag_ensure(rspt_hip_packer* p, int world) {
    if (p->lag.world >= world) return RSPT_HIP_OK;
    LagGather l;
    bool ok = hipStreamCreateWithFlags(l.stream.out(), hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; i < 2; ++i) {
        ok = ok && hipMalloc(l.dtotals[i].out(), (size_t)world * sizeof(uint64_t)) == hipSuccess;
        ok = ok && hipHostMalloc((void**)l.htotals[i].out(), (size_t)world * sizeof(uint64_t), hipHostMallocDefault) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(l.ev_in[i].out(), hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(l.ev_sizes[i].out(), hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(l.ev_payload[i].out(), hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) return RSPT_HIP_ERR_ALLOC;
    if (p->lag.stream) HIPCHK(p, hipStreamSynchronize(p->lag.stream));  // (nothing may still use the smaller set it replaces)
    l.world = world;
    p->lag = std::move(l);
    return RSPT_HIP_OK;
}

int rspt_hip_gather_post_sizes(rspt_hip_packer* p, void* comm, int world, const uint64_t* d_total, int slot, void* stream) {
    if (!p || !comm || world < 1 || !d_total || slot < 0 || slot > 1) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    int rc = gather_lag_ensure(p, world);
    if (rc) return rc;
    HIPCHK(p, hipEventRecord(p->lag.ev_in[slot], (hipStream_t)stream));  // d_total (and the container) are written on `stream`
    HIPCHK(p, hipStreamWaitEvent(p->lag.stream, p->lag.ev_in[slot], 0));
    rc = rspt_hip_gather_sizes(p, comm, world, d_total, p->lag.dtotals[slot], p->lag.htotals[slot], (void*)p->lag.stream);
    if (rc) return rc;
    HIPCHK(p, hipEventRecord(p->lag.ev_sizes[slot], p->lag.stream));
    p->lag.posted[slot] = true;
    return RSPT_HIP_OK;
}

int rspt_hip_gather_post_payload(rspt_hip_packer* p, void* comm, int rank, int world, int root, const void* d_packed, int slot, void* d_recv,
                                 size_t recv_stride, uint64_t* h_totals) {
    if (!p || slot < 0 || slot > 1 || !p->lag.posted[slot] || world > p->lag.world) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    HIPCHK(p, hipEventSynchronize(p->lag.ev_sizes[slot]));  // (a step old in the steady state: does not wait)
    p->lag.posted[slot] = false;
    if (h_totals) memcpy(h_totals, p->lag.htotals[slot], (size_t)world * sizeof(uint64_t));
    const int rc = rspt_hip_gather_payload(p, comm, rank, world, root, d_packed, p->lag.htotals[slot], d_recv, recv_stride, (void*)p->lag.stream);
    if (rc) return rc;
    HIPCHK(p, hipEventRecord(p->lag.ev_payload[slot], p->lag.stream));
    return RSPT_HIP_OK;
}

int rspt_hip_gather_wait(rspt_hip_packer* p, int slot, void* stream) {
    if (!p || slot < 0 || slot > 1) return RSPT_HIP_ERR_ARG;
    if (!p->lag.ev_payload[slot]) return RSPT_HIP_OK;  // (nothing was ever posted)
    HIPCHK(p, hipSetDevice(p->device));
    HIPCHK(p, hipStreamWaitEvent((hipStream_t)stream, p->lag.ev_payload[slot], 0));
    return RSPT_HIP_OK;
}
