// k_peak_offline_block_body.hpp -- the body of peak_offline_block and of peak_offline_block_planar (peak.hip): included once into
// each, with BPS, TR and PLANAR in scope.  Only the passes that read samples (the two baseline / band-pass walks) and the one that
// writes traces (the state machine's) see the layout; their planar statements are under `if constexpr (PLANAR)`, everything else
// is the native function's, statement for statement.
    const PeakCoef& c = k.c;
    auto xs = [&](uint32_t t) {
        if constexpr (PLANAR) return (double)row[t];
        else return (double)sample_load<BPS>(p + (size_t)t * stride, aligned);
    };
    const double x0 = xs(0);
    peak_history(D.bp, c.bb, c.bf, x0, c.hist);  // bandpass_ then baseline_ init_history_values(ecg_signal[0], fs)
    peak_history(D.bl, k.lb, k.lf, x0, c.hist);
    // baseline forward (stored), band-pass forward (state only)
    auto pass_fw = [&](uint32_t t, double x) {
        V[(size_t)t * 64] = D.bl.step_opt(k.lb, k.lf, x);
        D.bp.step_opt(c.bb, c.bf, x);
    };
    // baseline backward in place (kept as x - baseline, all the relocation reads), band-pass backward on x again
    auto pass_bw = [&](uint32_t t, OffPair v) {
        V[(size_t)t * 64] = v.a - D.bl.step_opt(k.lb, k.lf, v.b);
        F[(size_t)t * 64] = D.bp.step_opt(c.bb, c.bf, v.a);
    };
    auto xv = [&](uint32_t t) { return OffPair{xs(t), V[(size_t)t * 64]}; };
    if constexpr (PLANAR) {
        // vec (every row of the matrix on a 16-byte boundary, so ns % 4 == 0): the row as ns / 4 16-byte loads, the walks' look-ahead
        // of 16 and 8 samples kept; else dword by dword
        const int4* row4 = reinterpret_cast<const int4*>(row);
        if (vec) {
            off_walk<4, false>(ns / 4u, [&](uint32_t g) { return row4[g]; }, [&](uint32_t g, int4 w) {
                pass_fw(4u * g, (double)w.x);
                pass_fw(4u * g + 1u, (double)w.y);
                pass_fw(4u * g + 2u, (double)w.z);
                pass_fw(4u * g + 3u, (double)w.w);
            });
            off_walk<2, true>(ns / 4u, [&](uint32_t g) { return OffXV4{row4[g], {V[(size_t)(4u * g) * 64], V[(size_t)(4u * g + 1u) * 64], V[(size_t)(4u * g + 2u) * 64], V[(size_t)(4u * g + 3u) * 64]}}; },
                               [&](uint32_t g, OffXV4 q) {
                                   pass_bw(4u * g + 3u, OffPair{(double)q.x.w, q.v[3]});
                                   pass_bw(4u * g + 2u, OffPair{(double)q.x.z, q.v[2]});
                                   pass_bw(4u * g + 1u, OffPair{(double)q.x.y, q.v[1]});
                                   pass_bw(4u * g, OffPair{(double)q.x.x, q.v[0]});
                               });
        } else {
            off_walk<16, false>(ns, xs, pass_fw);
            off_walk<8, true>(ns, xv, pass_bw);
        }
    } else {
        off_walk<16, false>(ns, xs, pass_fw);
        off_walk<8, true>(ns, xv, pass_bw);
    }
    auto fs = [&](uint32_t t) { return F[(size_t)t * 64]; };
    off_walk<16, false>(ns, fs, [&](uint32_t t, double f) { F[(size_t)t * 64] = D.ig.step_opt(c.gb, c.gf, f * f); });
    off_walk<16, true>(ns, fs, [&](uint32_t t, double f) { F[(size_t)t * 64] = D.ig.step_opt(c.gb, c.gf, f); });
    off_walk<16, false>(ns, fs, [&](uint32_t t, double f) { D.th.step_opt(c.tb, c.tf, f); });
    off_walk<16, true>(ns, fs, [&](uint32_t t, double f) { T[(size_t)t * 64] = D.th.step_opt(c.tb, c.tf, f); });
    // the state machine; p over T, the shift folded in; E: the non-zero positions of p, those below nslope first (n0 of them)
    const uint32_t nslope = (uint32_t)c.nslope;  // (>= 1: the host refuses 0)
    uint32_t n = 0, n0 = 0;
    auto ft = [&](uint32_t t) { return OffPair{F[(size_t)t * 64], T[(size_t)t * 64]}; };
    auto sm = [&](uint32_t t, OffPair v) {
        if (TR) {
            if constexpr (!PLANAR) {
                sig[(size_t)t * nch] = v.a;
                thr[(size_t)t * nch] = v.b;
            }
        }
        const bool fire = D.machine(c, v.a, v.b);
        const double val = c.marker == -1.0 ? v.a : c.marker;
        const bool ev = fire && val != 0.0;  // (`if (peak_signal[i])`: NaN is an event, -0.0 is not)
        const bool below = t < nslope;
        T[(size_t)t * 64] = ev && below ? val : 0.0;
        if (ev && (below || nslope > 1)) {
            const uint32_t at = below ? t : t - nslope + 1u;
            if (!below) T[(size_t)at * 64] = val;
            E[(size_t)n * 64] = (int32_t)at;
            n += 1;
            n0 += below ? 1u : 0u;
        }
    };
    if constexpr (PLANAR) {
        // four samples a step, so that their trace values (what the walk loads) leave as 32 contiguous bytes of each trace row; the
        // row's last ns % 4 samples one by one.  The look-ahead stays 8 samples, all in front of what sm writes.
        const uint32_t n4 = ns / 4u;
        off_walk<2, false>(n4, [&](uint32_t g) { return OffFT4{{ft(4u * g), ft(4u * g + 1u), ft(4u * g + 2u), ft(4u * g + 3u)}}; },
                            [&](uint32_t g, OffFT4 q) {
                                if (TR) {
                                    store_d2(sig + (size_t)4u * g, q.v[0].a, q.v[1].a);
                                    store_d2(sig + (size_t)4u * g + 2, q.v[2].a, q.v[3].a);
                                    store_d2(thr + (size_t)4u * g, q.v[0].b, q.v[1].b);
                                    store_d2(thr + (size_t)4u * g + 2, q.v[2].b, q.v[3].b);
                                }
#pragma unroll
                                for (uint32_t e = 0; e < 4u; ++e) sm(4u * g + e, q.v[e]);
                            });
        for (uint32_t t = 4u * n4; t < ns; ++t) {
            const OffPair v = ft(t);
            if (TR) {
                sig[t] = v.a;
                thr[t] = v.b;
            }
            sm(t, v);
        }
    } else {
        off_walk<8, false>(ns, ft, sm);
    }
    // the relocation: visits the non-zero p[i], radius <= i <= ns - radius - 1, in ascending order, as the reference's loop
    // does -- including a value moved ahead of i (visited again) and a value written over another (the later write wins).
    // The candidates past the last visit `pos` are the E positions and, up to `fwd`, the targets of moves ahead.
    const int32_t r = k.radius;
    const int32_t lim = (int32_t)ns - r - 1;
    int32_t pos = r - 1, fwd = -1;
    uint32_t ia = 0, ib = n0;
    constexpr int32_t kNone = 0x7fffffff;
    for (;;) {
        while (ia < n0 && E[(size_t)ia * 64] <= pos) ++ia;
        while (ib < n && E[(size_t)ib * 64] <= pos) ++ib;
        const int32_t ca = ia < n0 ? E[(size_t)ia * 64] : kNone, cb = ib < n ? E[(size_t)ib * 64] : kNone;
        int32_t q = ca < cb ? ca : cb;
        if (fwd > pos) {  // a dense look at (pos, min(fwd, q - 1)], 8 loads at a time
            const int32_t hi = fwd < q - 1 ? fwd : q - 1;
            for (int32_t a0 = pos + 1; a0 <= hi; a0 += 8) {
                double w[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) w[u] = T[(size_t)(a0 + u <= hi ? a0 + u : hi) * 64];
                int32_t f = kNone;
#pragma unroll
                for (int u = 7; u >= 0; --u) f = (a0 + u <= hi && w[u] != 0.0) ? a0 + u : f;
                if (f != kNone) {
                    q = f;
                    break;
                }
            }
        }
        if (q > lim) break;
        const double pv = T[(size_t)q * 64];
        double mx = -2000000.0, mn = 2000000.0;
        int32_t mxi = 0, mni = 0;
        const int32_t j1 = q + r;  // (exclusive)
        for (int32_t j0 = q - r; j0 < j1; j0 += 8) {
            double w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) w[u] = V[(size_t)(j0 + u < j1 ? j0 + u : j1 - 1) * 64];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (j0 + u < j1) {
                    if (mx < w[u]) {
                        mx = w[u];
                        mxi = j0 + u;
                    }
                    if (mn > w[u]) {
                        mn = w[u];
                        mni = j0 + u;
                    }
                }
            }
        }
        const int32_t to = mx > -mn ? mxi : mni;
        T[(size_t)q * 64] = 0.0;
        T[(size_t)to * 64] = pv;
        if (to > q && to > fwd) fwd = to;
        pos = q;
    }
    // the counts and the events: the non-zero final p in ascending order
    uint32_t cnt = 0;
    off_walk<16, false>(ns, [&](uint32_t t) { return T[(size_t)t * 64]; }, [&](uint32_t t, double v) {
        if (v != 0.0) {
            if (cnt < max_peaks) {
                index[cnt] = (int32_t)t;
                value[cnt] = v;
            }
            ++cnt;
        }
    });
    count[0] = cnt;
