// k_peak_block_body.hpp -- the body of peak_block and of peak_block_planar (peak.hip): included once into each, with BPS, V, TR
// and PLANAR in scope.  Native: the samples of the detector are `stride` bytes apart at p, its trace samples nch doubles apart.
// Planar: they are the int32 row `row`, its traces the rows sig / thr of doubles.  The planar statements are under
// `if constexpr (PLANAR)`; everything else is the native function's, statement for statement.
    constexpr int NB = PeakDet<V>::NB;
    uint32_t cnt = 0;
    auto emit = [&](uint32_t t, bool fire, double s, double h) {
        if (TR) {
            if constexpr (!PLANAR) {
                sig[(size_t)t * nch] = s;
                thr[(size_t)t * nch] = h;
            }
        }
        if (fire) {
            if (cnt < max_peaks) {
                index[cnt] = (int32_t)t;
                value[cnt] = c.marker == -1.0 ? s : c.marker;
            }
            ++cnt;
        }
    };
    // one sample / one trace pair of the planar row (the row's ends; whole chunks go in pieces, below)
    auto xr = [&](uint32_t t) { return (double)row[t]; };
    auto trace1 = [&](uint32_t t, double s, double h) {
        if (TR) {
            sig[t] = s;
            thr[t] = h;
        }
    };
    if (V == kPeakOfflineFw) {  // every detect_fw call
        if constexpr (PLANAR) peak_history(D.bp, c.bb, c.bf, xr(0), c.hist);
        else peak_history(D.bp, c.bb, c.bf, (double)sample_load<BPS>(p, aligned), c.hist);
    }
    // ONLINE: the history runs where sample_indx_ is 0 -- the first sample of a fresh detector, or where the int wraps back
    // to 0 after 2^32 samples (then this block takes the sample-by-sample path below)
    bool simple = false;
    if (V != kPeakOfflineFw) {  // sample 0's `if (!sample_indx_++)`
        const bool first = D.idx == 0;
        simple = !first && (uint64_t)D.idx + ns > (1ull << 32);  // (0 comes back inside this block)
        if (first) {
            if constexpr (PLANAR) peak_history(D.bp, c.bb, c.bf, xr(0), c.hist);
            else peak_history(D.bp, c.bb, c.bf, (double)sample_load<BPS>(p, aligned), c.hist);
        }
        D.idx += 1;
    }
    if (simple) {
        for (uint32_t t = 0; t < ns; ++t) {
            double x;
            if constexpr (PLANAR) x = xr(t);
            else x = (double)sample_load<BPS>(p + (size_t)t * stride, aligned);
            if (t > 0) {  // (sample 0's index was handled above)
                if (D.idx == 0) peak_history(D.bp, c.bb, c.bf, x, c.hist);
                D.idx += 1;
            }
            double s, h;
            const bool f = D.tail(c, D.bp.step_opt(c.bb, c.bf, x), s, h);
            emit(t, f, s, h);
            if constexpr (PLANAR) trace1(t, s, h);
        }
        count[0] = cnt;
        return;
    }
    if (V != kPeakOfflineFw) D.idx += ns - 1;  // (no wrap back to 0 in this block)
    // Chunks of CH samples: the next chunk's loads are in flight while this one runs, and the band-pass feed-forward sums of
    // the chunk (independent of every output) are formed up front, for the scheduler to place into the dependent chain.
    constexpr uint32_t CH = 16;
    int32_t cur[CH], nxt[CH];
    const uint32_t nfull = ns / CH;
    // planar: a chunk is 64 contiguous bytes of the row, four 16-byte loads where every row of the matrix starts on a 16-byte
    // boundary (vec, the same for all lanes), else sixteen dwords; only whole chunks inside the row are ever loaded
    auto chunk = [&](int32_t (&v)[CH], const int32_t* q) {
        if (vec) {
#pragma unroll
            for (uint32_t e = 0; e < CH; e += 4) {
                const int4 w = *reinterpret_cast<const int4*>(q + e);
                v[e] = w.x;
                v[e + 1] = w.y;
                v[e + 2] = w.z;
                v[e + 3] = w.w;
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < CH; ++e) v[e] = q[e];
        }
    };
    if (nfull) {
        if constexpr (PLANAR) {
            chunk(cur, row);
        } else {
#pragma unroll
            for (uint32_t e = 0; e < CH; ++e) cur[e] = sample_load<BPS>(p + (size_t)e * stride, aligned);
        }
    }
    for (uint32_t k = 0; k < nfull; ++k) {
        const uint8_t* q = p + (size_t)k * CH * stride;
        if (k + 1 < nfull) {
            if constexpr (PLANAR) {
                chunk(nxt, row + (size_t)(k + 1) * CH);
            } else {
#pragma unroll
                for (uint32_t e = 0; e < CH; ++e) nxt[e] = sample_load<BPS>(q + (size_t)(CH + e) * stride, aligned);
            }
        }
        double xs[CH + NB - 1], ff[CH];
#pragma unroll
        for (int i = 0; i < NB - 1; ++i) xs[i] = D.bp.x[NB - 2 - i];
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) xs[NB - 1 + e] = (double)cur[e];
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) ff[e] = iir_ff<NB>(c.bf, &xs[NB - 1 + e]);
        double sg[4], hg[4];  // planar traces: four samples in registers, then 32 contiguous bytes of each trace row
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) {
            double s, h;
            const bool f = D.tail(c, D.bp.feedback(c.bb, ff[e]), s, h);
            emit(k * CH + e, f, s, h);
            if constexpr (PLANAR) {
                if (TR) {
                    sg[e & 3u] = s;
                    hg[e & 3u] = h;
                    if ((e & 3u) == 3u) {
                        const size_t t0 = (size_t)k * CH + e - 3u;
                        store_d2(sig + t0, sg[0], sg[1]);
                        store_d2(sig + t0 + 2, sg[2], sg[3]);
                        store_d2(thr + t0, hg[0], hg[1]);
                        store_d2(thr + t0 + 2, hg[2], hg[3]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) D.bp.x[i] = xs[CH + NB - 2 - i];
#pragma unroll
        for (uint32_t e = 0; e < CH; ++e) cur[e] = nxt[e];
    }
    for (uint32_t t = nfull * CH; t < ns; ++t) {
        double s, h;
        bool f;
        if constexpr (PLANAR) f = D.tail(c, D.bp.step_opt(c.bb, c.bf, xr(t)), s, h);
        else f = D.tail(c, D.bp.step_opt(c.bb, c.bf, (double)sample_load<BPS>(p + (size_t)t * stride, aligned)), s, h);
        emit(t, f, s, h);
        if constexpr (PLANAR) trace1(t, s, h);
    }
    count[0] = cnt;
