// host_pipeline.hip -- the host pipelines over compress_batch_serial / decompress_dev (rspt_hip.hip): rspt_hip_compress_many,
// rspt_hip_decompress_many and the feed.  Included by rspt_hip.hip.

// the copy streams of the many-block pipeline and the feed: made once, by whichever of the two comes first
static int ensure_copy_streams(rspt_hip_packer* p) {
    if (!p->m_up && hipStreamCreateWithFlags(p->m_up.out(), hipStreamNonBlocking) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
    if (!p->m_down && hipStreamCreateWithFlags(p->m_down.out(), hipStreamNonBlocking) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
    return RSPT_HIP_OK;
}

// the staging stride of one compressed stream in a slot
static size_t slot_stride(const rspt_hip_packer* p) { return (rspt_hip_max_compressed_size(p) + 255) & ~(size_t)255; }

// a slot for n blocks (a caller that gets false drops the slot: nothing half-made is kept)
static bool alloc_slot(const rspt_hip_packer* p, Slot& s, size_t n) {
    return hipMalloc(s.d_src.out(), n * p->g.block_bytes + 64) == hipSuccess && hipMalloc(s.d_dst.out(), n * slot_stride(p)) == hipSuccess &&
           hipMalloc(s.d_sizes.out(), n * sizeof(uint64_t)) == hipSuccess &&
           hipHostMalloc((void**)s.h_sizes.out(), (n + 1) * sizeof(uint64_t), hipHostMallocDefault) == hipSuccess &&
           hipEventCreateWithFlags(s.ev_up.out(), hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(s.ev_comp.out(), hipEventDisableTiming) == hipSuccess &&
           hipEventCreateWithFlags(s.ev_down.out(), hipEventDisableTiming) == hipSuccess;
}

static int ensure_many(rspt_hip_packer* p) {
    if (p->many.chunk) return RSPT_HIP_OK;
    int rc = ensure_copy_streams(p);
    if (rc) return rc;
    // ~64 MiB of samples per chunk: long enough copies for the DMA engines, short enough that the pipeline fills quickly
    size_t chunk = (64ull << 20) / p->g.block_bytes;
    chunk = chunk < 1 ? 1 : chunk > 64 ? 64 : chunk;
    ManyStaging m;
    bool ok = alloc_slot(p, m.slot[0], chunk) && alloc_slot(p, m.slot[1], chunk);
    for (int i = 0; i < 2; ++i) ok = ok && hipMalloc(m.idx[i].out(), (4 + 2 * chunk) * sizeof(uint64_t)) == hipSuccess;
    ok = ok && hipHostMalloc((void**)m.hidx.out(), 2 * (4 + 2 * chunk) * sizeof(uint64_t), hipHostMallocDefault) == hipSuccess;
    if (!ok) return RSPT_HIP_ERR_ALLOC;
    m.chunk = chunk;
    m.stride = slot_stride(p);
    p->many = std::move(m);
    return rspt_hip_reserve(p, chunk);
}

static int compress_many_pipeline(rspt_hip_packer* p, const void* src_host, size_t nblocks, void* dst_host, size_t dst_stride, size_t* dst_len);

int rspt_hip_compress_many(rspt_hip_packer* p, const void* src_host, size_t nblocks, void* dst_host, size_t dst_stride, size_t* dst_len) {
    if (!p || !src_host || !dst_host || !dst_len || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;  // (the feed owns the workspace and the copy streams until rspt_hip_feed_end)
    HIPCHK(p, hipSetDevice(p->device));
    int rc = ensure_many(p);
    if (rc) return rc;
    rc = compress_many_pipeline(p, src_host, nblocks, dst_host, dst_stride, dst_len);
    if (rc != RSPT_HIP_OK && rc != RSPT_HIP_ERR_DST_TOO_SMALL) {
        // a failure in the middle: nothing may still be copying from or into the caller's buffers when we return
        hipStreamSynchronize(p->m_up);
        hipStreamSynchronize(p->stream);
        hipStreamSynchronize(p->m_down);
    }
    return rc;
}

static int compress_many_pipeline(rspt_hip_packer* p, const void* src_host, size_t nblocks, void* dst_host, size_t dst_stride, size_t* dst_len) {
    int rc = RSPT_HIP_OK;
    const size_t C = p->many.chunk, bb = p->g.block_bytes;
    const size_t nchunk = (nblocks + C - 1) / C;
    const uint8_t* src = (const uint8_t*)src_host;
    uint8_t* dst = (uint8_t*)dst_host;
    bool too_small = false;
    // the streams of chunk k leave for the host (exact lengths: its sizes have to be here first)
    auto download = [&](size_t k) -> int {
        Slot& s = p->many.slot[k & 1];
        const size_t first = k * C, cnt = nblocks - first < C ? nblocks - first : C;
        HIPCHK(p, hipEventSynchronize(s.ev_comp));
        const uint64_t* hs = s.h_sizes;
        for (size_t i = 0; i < cnt; ++i) {
            const uint64_t sz = hs[i];
            if ((sz >> 63) || sz > dst_stride) {  // flagged by the device (did not fit the staging stride), or too long for the caller's
                dst_len[first + i] = (sz >> 63) ? 0 : (size_t)sz;
                too_small = true;
                continue;
            }
            dst_len[first + i] = (size_t)sz;
            HIPCHK(p, hipMemcpyAsync(dst + (first + i) * dst_stride, s.d_dst + i * p->many.stride, (size_t)sz, hipMemcpyDeviceToHost, p->m_down));
        }
        HIPCHK(p, hipEventRecord(s.ev_down, p->m_down));
        return RSPT_HIP_OK;
    };
    for (size_t k = 0; k < nchunk; ++k) {
        Slot& s = p->many.slot[k & 1];
        const size_t first = k * C, cnt = nblocks - first < C ? nblocks - first : C;
        if (k >= 2) {
            HIPCHK(p, hipStreamWaitEvent(p->m_up, s.ev_comp, 0));     // chunk k-2 has been read out of this slot
            HIPCHK(p, hipStreamWaitEvent(p->stream, s.ev_down, 0));  // ... and its streams have left it
        }
        HIPCHK(p, hipMemcpyAsync(s.d_src, src + first * bb, cnt * bb, hipMemcpyHostToDevice, p->m_up));
        HIPCHK(p, hipEventRecord(s.ev_up, p->m_up));
        HIPCHK(p, hipStreamWaitEvent(p->stream, s.ev_up, 0));
        rc = compress_batch_serial(p, s.d_src, cnt, s.d_dst, p->many.stride, s.d_sizes, p->stream);
        if (rc) return rc;
        HIPCHK(p, hipMemcpyAsync(s.h_sizes, s.d_sizes, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
        HIPCHK(p, hipEventRecord(s.ev_comp, p->stream));
        if (k >= 1) {
            rc = download(k - 1);
            if (rc) return rc;
        }
    }
    rc = download(nchunk - 1);
    if (rc) return rc;
    uint32_t nb_now = 0;
    HIPCHK(p, hipMemcpyAsync(&nb_now, p->nb_state, sizeof(nb_now), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(p, hipStreamSynchronize(p->stream));
    HIPCHK(p, hipStreamSynchronize(p->m_down));
    if (nb_now >= 1 && nb_now <= 4) p->nb_host = nb_now;
    return too_small ? RSPT_HIP_ERR_DST_TOO_SMALL : RSPT_HIP_OK;
}

// ---- rspt_hip_feed_*: blocks that arrive over time ---------------------------------------------------------------------------
int rspt_hip_feed_begin(rspt_hip_packer* p, size_t blocks_per_launch, size_t slots) {
    if (!p || blocks_per_launch == 0 || blocks_per_launch > 4096 || slots < 2 || slots > 64 || p->feed) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    int rc = ensure_copy_streams(p);
    if (rc) return rc;
    rc = rspt_hip_reserve(p, blocks_per_launch);
    if (rc) return rc;
    std::unique_ptr<Feed> f(new (std::nothrow) Feed());
    if (!f) return RSPT_HIP_ERR_ALLOC;
    f->G = blocks_per_launch;
    f->stride = slot_stride(p);
    f->slots.resize(slots);
    for (auto& s : f->slots) {
        if (!alloc_slot(p, s, f->G)) return RSPT_HIP_ERR_ALLOC;
        s.dst_host.resize(f->G);
        s.dst_cap.resize(f->G);
    }
    p->feed = std::move(f);
    return RSPT_HIP_OK;
}

static int feed_launch(rspt_hip_packer* p, FeedSlot& s) {
    Feed* f = p->feed.get();
    HIPCHK(p, hipEventRecord(s.ev_up, p->m_up));
    HIPCHK(p, hipStreamWaitEvent(p->stream, s.ev_up, 0));
    const int rc = compress_batch_serial(p, s.d_src, s.count, s.d_dst, f->stride, s.d_sizes, p->stream);
    if (rc) return rc;
    HIPCHK(p, hipMemcpyAsync(s.h_sizes, s.d_sizes, s.count * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(p, hipMemcpyAsync(s.h_sizes + f->G, p->nb_state, sizeof(uint32_t), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(p, hipEventRecord(s.ev_comp, p->stream));
    s.state = FeedSlot::COMPRESSING;
    return RSPT_HIP_OK;
}

int rspt_hip_feed_submit(rspt_hip_packer* p) {
    if (!p || !p->feed) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    Feed* f = p->feed.get();
    FeedSlot& s = f->slots[f->tail];
    if (s.state != FeedSlot::FILLING || s.count == 0) return RSPT_HIP_OK;
    const int rc = feed_launch(p, s);
    if (rc) {  // nothing of this group will arrive: its blocks are reported by rspt_hip_feed_poll with the failure as their status
        s.error = rc;
        s.state = FeedSlot::DONE;
    }
    f->tail = (f->tail + 1) % f->slots.size();
    return rc;
}

int rspt_hip_feed_push(rspt_hip_packer* p, const void* src_host, void* dst_host, size_t dst_cap) {
    if (!p || !p->feed || !src_host || !dst_host) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    Feed* f = p->feed.get();
    FeedSlot& s = f->slots[f->tail];
    if (s.state != FeedSlot::FREE && s.state != FeedSlot::FILLING) return RSPT_HIP_ERR_BUSY;  // the ring is full: poll first
    if (s.state == FeedSlot::FREE) {
        s.state = FeedSlot::FILLING;
        s.count = s.delivered = 0;
        s.error = 0;
        s.first_seq = f->next_seq;
    }
    const size_t i = s.count;
    HIPCHK(p, hipMemcpyAsync(s.d_src + i * p->g.block_bytes, src_host, p->g.block_bytes, hipMemcpyHostToDevice, p->m_up));
    s.dst_host[i] = dst_host;
    s.dst_cap[i] = dst_cap;
    ++s.count;
    ++f->next_seq;
    if (s.count == f->G) return rspt_hip_feed_submit(p);
    return RSPT_HIP_OK;
}

// move every slot as far as it can go without waiting (wait = true: wait for each step instead)
static int feed_advance(rspt_hip_packer* p, bool wait) {
    Feed* f = p->feed.get();
    const size_t n = f->slots.size();
    for (size_t k = 0; k < n; ++k) {
        FeedSlot& s = f->slots[(f->head + k) % n];
        if (s.state == FeedSlot::COMPRESSING) {
            if (wait) HIPCHK(p, hipEventSynchronize(s.ev_comp));
            const hipError_t q = hipEventQuery(s.ev_comp);
            if (q == hipErrorNotReady) break;  // (the slots behind it are not further along: one compute stream)
            if (q != hipSuccess) {
                p->last_hip_error = (int)q;
                return RSPT_HIP_ERR_LAUNCH;
            }
            const uint32_t nb_now = (uint32_t)s.h_sizes[f->G];
            if (nb_now >= 1 && nb_now <= 4 && nb_now > p->nb_host) p->nb_host = nb_now;  // the next launch writes exactly the planes it needs
            HIPCHK(p, hipStreamWaitEvent(p->m_down, s.ev_comp, 0));
            for (size_t i = 0; i < s.count; ++i) {
                const uint64_t sz = s.h_sizes[i];
                if (!(sz >> 63) && sz <= s.dst_cap[i])
                    HIPCHK(p, hipMemcpyAsync(s.dst_host[i], s.d_dst + i * f->stride, (size_t)sz, hipMemcpyDeviceToHost, p->m_down));
            }
            HIPCHK(p, hipEventRecord(s.ev_down, p->m_down));
            s.state = FeedSlot::DOWNLOADING;
        }
        if (s.state == FeedSlot::DOWNLOADING) {
            if (wait) HIPCHK(p, hipEventSynchronize(s.ev_down));
            const hipError_t q = hipEventQuery(s.ev_down);
            if (q == hipErrorNotReady) continue;  // (a later slot's compress may still be ready for its downloads)
            if (q != hipSuccess) {
                p->last_hip_error = (int)q;
                return RSPT_HIP_ERR_LAUNCH;
            }
            s.state = FeedSlot::DONE;
        }
    }
    return RSPT_HIP_OK;
}

int rspt_hip_feed_poll(rspt_hip_packer* p, size_t* seq, size_t* dst_len, int* status) {
    if (!p || !p->feed || !seq || !dst_len || !status) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    Feed* f = p->feed.get();
    const int rc = feed_advance(p, false);
    if (rc) return rc;
    FeedSlot& s = f->slots[f->head];
    if (s.state != FeedSlot::DONE) return 0;
    const size_t i = s.delivered;
    const uint64_t sz = s.error ? 0 : s.h_sizes[i];
    *seq = s.first_seq + i;
    if (s.error) {
        *dst_len = 0;
        *status = s.error;
    } else if ((sz >> 63) || sz > s.dst_cap[i]) {
        *dst_len = (sz >> 63) ? 0 : (size_t)sz;
        *status = RSPT_HIP_ERR_DST_TOO_SMALL;
    } else {
        *dst_len = (size_t)sz;
        *status = RSPT_HIP_OK;
    }
    if (++s.delivered == s.count) {
        s.state = FeedSlot::FREE;
        f->head = (f->head + 1) % f->slots.size();
    }
    return 1;
}

int rspt_hip_feed_flush(rspt_hip_packer* p) {
    if (!p || !p->feed) return RSPT_HIP_ERR_ARG;
    int rc = rspt_hip_feed_submit(p);
    if (rc) return rc;
    return feed_advance(p, true);
}

int rspt_hip_feed_end(rspt_hip_packer* p) {
    if (!p || !p->feed) return RSPT_HIP_ERR_ARG;
    hipSetDevice(p->device);
    rspt_hip_feed_submit(p);
    hipStreamSynchronize(p->m_up);
    hipStreamSynchronize(p->stream);
    hipStreamSynchronize(p->m_down);  // nothing is copying from or into the caller's buffers any more
    p->feed.reset();
    return RSPT_HIP_OK;
}

static int decompress_many_pipeline(rspt_hip_packer* p, const void* src_host, size_t src_stride, const size_t* src_len, size_t nblocks, void* dst_host,
                                    size_t* consumed) {
    const size_t C = p->many.chunk, bb = p->g.block_bytes;
    const size_t nchunk = (nblocks + C - 1) / C;
    const uint8_t* src = (const uint8_t*)src_host;
    uint8_t* dst = (uint8_t*)dst_host;
    bool corrupt = false;
    // the slots are used the other way round: streams go up into d_dst, blocks come back out of d_src
    auto finish = [&](size_t k) -> int {
        Slot& s = p->many.slot[k & 1];
        const size_t first = k * C, cnt = nblocks - first < C ? nblocks - first : C;
        HIPCHK(p, hipEventSynchronize(s.ev_comp));
        const uint64_t* hs = s.h_sizes;
        for (size_t i = 0; i < cnt; ++i) {
            const bool bad = (hs[i] >> 63) != 0;
            consumed[first + i] = bad ? 0 : (size_t)hs[i];
            corrupt |= bad;
        }
        return RSPT_HIP_OK;
    };
    for (size_t k = 0; k < nchunk; ++k) {
        const int slot = (int)(k & 1);
        Slot& s = p->many.slot[slot];
        const size_t first = k * C, cnt = nblocks - first < C ? nblocks - first : C;
        if (k >= 2) {
            HIPCHK(p, hipStreamWaitEvent(p->m_up, s.ev_comp, 0));     // chunk k-2 has been decoded out of this slot
            HIPCHK(p, hipStreamWaitEvent(p->stream, s.ev_down, 0));  // ... and its blocks have left it
        }
        uint64_t* hidx = nullptr;
        if (src_len) {
            // Only src_len[i] bytes of every stream go up, into a slot that still holds an earlier chunk's bytes behind them: the
            // decoder is therefore bounded by each stream's OWN length -- an index over the slot in the container's form
            // (offset, length; nb 0 = the handle's state), checked on the device like any container -- and not by the slot stride.
            hidx = p->many.hidx + (size_t)slot * (4 + 2 * C);
            if (k >= 2) HIPCHK(p, hipEventSynchronize(s.ev_up));  // (the upload of chunk k-2 has read this staging index)
            hidx[0] = 0x4B43415054505352ull;
            hidx[1] = cnt;
            hidx[2] = (uint64_t)cnt * p->many.stride;
            hidx[3] = 0;
            for (size_t i = 0; i < cnt; ++i) {
                const size_t nbytes = src_len[first + i] < src_stride ? src_len[first + i] : src_stride;
                hidx[4 + 2 * i] = (uint64_t)i * p->many.stride;
                hidx[4 + 2 * i + 1] = nbytes;
                if (nbytes) HIPCHK(p, hipMemcpyAsync(s.d_dst + i * p->many.stride, src + (first + i) * src_stride, nbytes, hipMemcpyHostToDevice, p->m_up));
            }
            HIPCHK(p, hipMemcpyAsync(p->many.idx[slot], hidx, (4 + 2 * cnt) * sizeof(uint64_t), hipMemcpyHostToDevice, p->m_up));
        } else {
            HIPCHK(p, hipMemcpy2DAsync(s.d_dst, p->many.stride, src + first * src_stride, src_stride, src_stride, cnt, hipMemcpyHostToDevice, p->m_up));
        }
        HIPCHK(p, hipEventRecord(s.ev_up, p->m_up));
        HIPCHK(p, hipStreamWaitEvent(p->stream, s.ev_up, 0));
        const int rc = hidx ? decompress_dev(p, s.d_dst, 0, p->many.idx[slot] + 4, 32 + 16 * cnt + cnt * p->many.stride, cnt, s.d_src,
                                             s.d_sizes, (void*)p->stream)
                            : rspt_hip_decompress_batch_dev(p, s.d_dst, p->many.stride, cnt, s.d_src, s.d_sizes, (void*)p->stream);
        if (rc) return rc;
        HIPCHK(p, hipMemcpyAsync(s.h_sizes, s.d_sizes, cnt * sizeof(uint64_t), hipMemcpyDeviceToHost, p->stream));
        HIPCHK(p, hipEventRecord(s.ev_comp, p->stream));
        // the blocks leave as soon as they are decoded: their size is known beforehand
        HIPCHK(p, hipStreamWaitEvent(p->m_down, s.ev_comp, 0));
        HIPCHK(p, hipMemcpyAsync(dst + first * bb, s.d_src, cnt * bb, hipMemcpyDeviceToHost, p->m_down));
        HIPCHK(p, hipEventRecord(s.ev_down, p->m_down));
        if (k >= 1) {
            const int rf = finish(k - 1);
            if (rf) return rf;
        }
    }
    const int rf = finish(nchunk - 1);
    if (rf) return rf;
    HIPCHK(p, hipStreamSynchronize(p->m_down));
    return corrupt ? RSPT_HIP_ERR_CORRUPT : RSPT_HIP_OK;
}

int rspt_hip_decompress_many(rspt_hip_packer* p, const void* src_host, size_t src_stride, const size_t* src_len, size_t nblocks, void* dst_host,
                             size_t* consumed) {
    if (!p || !src_host || !dst_host || !consumed || nblocks == 0 || src_stride == 0) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;  // (the feed owns the workspace and the copy streams until rspt_hip_feed_end)
    HIPCHK(p, hipSetDevice(p->device));
    int rc = ensure_many(p);
    if (rc) return rc;
    if (src_stride > p->many.stride) return RSPT_HIP_ERR_ARG;
    rc = decompress_many_pipeline(p, src_host, src_stride, src_len, nblocks, dst_host, consumed);
    if (rc != RSPT_HIP_OK && rc != RSPT_HIP_ERR_CORRUPT) {
        hipStreamSynchronize(p->m_up);
        hipStreamSynchronize(p->stream);
        hipStreamSynchronize(p->m_down);
    }
    return rc;
}
