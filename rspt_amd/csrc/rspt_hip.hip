// rspt_hip.hip -- C ABI (include/rspt_hip.h) over the gfx950 kernels: the one translation unit of the unity build.
//
// One handle = one reference packer instance: it owns the device workspace
// (what enc_/serialized_ are in signal_packer_base.h:20-21), one HIP stream and
// the persistent nr_bytes_to_compress_ state (signal_packer_xdelta_hzr.cpp:39,66),
// which lives in device memory so that batches chain without a host round trip.
// There is no CPU path: every entry point fails loudly if the device is missing.
// Here: create / reserve / destroy, the compress phases, the decoder, the single-block entries.  Included at the end: host_pipeline.hip
// (compress_many / decompress_many / feed), host_gather.hip (RCCL), host_stages.hip (IIR, FIR, median, peak, PRDN, converters),
// host_target.hip (compress to a PRDN target), host_budget.hip (compress to a byte budget), host_total.hip (compress a batch to one
// byte total).
#include "../../include/rspt_hip.h"

#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <link.h>
#include <climits>
#include <string>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "common.hpp"

// unity build: the kernels live in the same translation unit
#include "preprocess.hip"
#include "hzr_kernels.hip"
#include "hzr_rows.hip"
#include "transforms.hip"
#include "decode.hip"
#include "filter.hip"
#include "iir_cascade.hip"
#include "iir_zero_phase.hip"
#include "fir.hip"
#include "fir_planar.hip"
#include "median.hip"
#include "median_planar.hip"
#include "peak.hip"
#include "quality.hip"
#include "quality_planar.hip"
#include "convert.hip"
#include "bytes.hip"
#include "planar.hip"
#include "target.hip"
#include "pack_choice.hip"
#include "budget.hip"
#include "total.hip"

using namespace rspt;

#include "host_handle.hpp"
#include "rate_work.hpp"

namespace {

// GF(2) helpers on the host (tools/kernel_model.py has the same math)
uint32_t x_pow_bytes(uint64_t nbytes) {
    uint32_t r = 0x80000000u, base = 0x00800000u;
    while (nbytes) {
        if (nbytes & 1) r = gf_mul(r, base);
        base = gf_mul(base, base);
        nbytes >>= 1;
    }
    return r;
}

uint32_t raw_crc4(uint32_t le) {
    uint32_t c = le;
    for (int i = 0; i < 32; ++i) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
    return c;
}

void make_crc_consts(CrcConsts& cc) {
    for (uint32_t b = 0; b < 256; ++b) {
        uint32_t r = b;
        for (int k = 0; k < 8; ++k) r = (r >> 1) ^ (kCrcPoly & (0u - (r & 1u)));
        cc.table[0][b] = r;
    }
    for (int t = 1; t < 4; ++t)  // slice-by-4: table[t][b] = state after byte b followed by t zero bytes
        for (uint32_t b = 0; b < 256; ++b) cc.table[t][b] = (cc.table[t - 1][b] >> 8) ^ cc.table[0][cc.table[t - 1][b] & 0xFFu];
    for (int i = 0; i < 81; ++i) {
        const uint32_t K = i < 64 ? x_pow_bytes(64ull * (63 - i)) : i < 80 ? x_pow_bytes(4096ull * (15 - (i - 64))) : x_pow_bytes(65536);
        for (int jx = 0; jx < 4; ++jx)
            for (uint32_t b = 0; b < 256; ++b) cc.shift[i][jx][b] = gf_mul(b << (8 * jx), K);
    }
    for (int l = 0; l < 64; ++l) {
        const uint32_t K = x_pow_bytes(4ull * (l + 1));
        for (int jx = 0; jx < 4; ++jx)
            for (uint32_t b = 0; b < 256; ++b) cc.shift4[l][jx][b] = gf_mul(b << (8 * jx), K);
    }
    // X with raw_crc(X) = 0xFFFFFFFF: the 4-byte raw CRC map is linear and invertible
    uint32_t img[32];
    for (int b = 0; b < 32; ++b) img[b] = raw_crc4(1u << b);
    uint32_t rows_v[32], rows_t[32];
    for (int b = 0; b < 32; ++b) {
        rows_v[b] = img[b];
        rows_t[b] = 1u << b;
    }
    int piv[32];
    bool used[32] = {false};
    for (int bit = 0; bit < 32; ++bit) {
        piv[bit] = -1;
        for (int i = 0; i < 32; ++i)
            if (!used[i] && ((rows_v[i] >> bit) & 1u)) {
                piv[bit] = i;
                used[i] = true;
                for (int jx = 0; jx < 32; ++jx)
                    if (jx != i && ((rows_v[jx] >> bit) & 1u)) {
                        rows_v[jx] ^= rows_v[i];
                        rows_t[jx] ^= rows_t[i];
                    }
                break;
            }
    }
    uint32_t x = 0;
    for (int bit = 0; bit < 32; ++bit) x ^= rows_t[piv[bit]];  // target has every bit set
    cc.prefix = x;
    cc.pad[0] = cc.pad[1] = cc.pad[2] = 0;
}

static_assert(kKindBytes == (uint32_t)RSPT_HIP_KIND_BYTES, "common.hpp and rspt_hip.h name the same kind");

}  // namespace

// tile of k_tile_planar_i32x4 / k_planar_native_i32x4: T4 samples x nch channels in at most 32 KiB of LDS (four workgroups
// per CU), T4 a multiple of 4
static uint32_t tile_i32x4(const Geom& g) {
    uint32_t T4 = (uint32_t)((32768ull / (4ull * g.nch) - 1) & ~3ull);
    T4 = T4 > 1024 ? 1024 : T4 < 4 ? 4 : T4;
    return T4 > g.ns ? g.ns : T4;
}

template <int BPS, bool XD>
static void launch_planes(rspt_hip_packer* p, const uint8_t* d_src, size_t nblocks, uint32_t kfirst, uint32_t kcount, const uint32_t* nbuse,
                          hipStream_t st) {
    const Geom& g = p->g;
    const uint32_t T = p->Tp[kcount];
    const bool stream_ok = (reinterpret_cast<uintptr_t>(d_src) & 3u) == 0 && g.ns >= 16 && g.block_bytes < (1ull << 32) && !(p->ablate & (1u << 22));
    const uint32_t lds = kcount * g.nch * (T + 16u) + 32u * g.nch + 96u;
    const uint32_t ntiles = (uint32_t)((g.ns + T - 1) / T * nblocks);
    const uint32_t per_cu = lds <= 40 * 1024 ? 4u : lds <= 80 * 1024 ? 2u : 1u;
    uint32_t want = per_cu * (uint32_t)p->num_cu;
    if (p->k1_grid) want = p->k1_grid;
    dim3 grid(want < ntiles ? want : ntiles);
    // every sample width streams (k_tile_stream, one load per sample: dword / unaligned dword / short / byte)
    const bool stream = stream_ok;
    if (stream) {
        constexpr int SB = BPS;
        auto go = [&](auto kern) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, d_src, g, T, kfirst, kcount, p->ws.planes, p->needmask, p->nzflag, nbuse, p->ablate,
                               (uint32_t)nblocks, nbuse ? nullptr : p->work_ctr + 1, p->nb_state, p->ws.nbuse, p->ws.plane_dirty, p->dirty_shift);
        };
        if (g.ns & 15u)
            go(&k_tile_stream<SB, XD, true>);  // (a short last group per channel, plane rows at any byte alignment)
        else
            go(&k_tile_stream<SB, XD, false>);
        return;
    }
    hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tile_planes<BPS, XD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((k_tile_planes<BPS, XD>), grid, dim3(p->k1_threads), lds, st, d_src, g, T, kfirst, kcount, p->ws.planes, p->needmask, p->nzflag, nbuse, p->ablate, (uint32_t)nblocks,
                       nbuse ? nullptr : p->work_ctr + 1, p->nb_state, p->ws.nbuse);
}

// main front-end pass; returns the number of planes it wrote (xdelta: nb as last seen by the host)
template <int BPS>
static uint32_t launch_front(rspt_hip_packer* p, const uint8_t* d_src, size_t nblocks, hipStream_t st) {
    const Geom& g = p->g;
    if (p->wide) {
        // wide blocks (> ~1000 channels): transpose to the planar block, then -- for the two hzr packers -- the flat stage over it.
        // All four planes are written (an escalation inside the batch needs no second pass), nbuse[] says how many the encoders take.
        hipLaunchKernelGGL(k_wide_planar<BPS>, dim3((g.ns + 63) / 64, (g.nch + 63) / 64, (unsigned)nblocks), dim3(256), 0, st, d_src, g, p->ws.planar);
        if (g.kind == RSPT_HIP_KIND_XDELTA_HZR || g.kind == RSPT_HIP_KIND_HZR) {
            const bool xd = g.kind == RSPT_HIP_KIND_XDELTA_HZR;
            const dim3 pg((g.N + 4095) / 4096, (unsigned)nblocks);
            if (xd)
                hipLaunchKernelGGL((k_planar_planes<true>), pg, dim3(256), 0, st, p->ws.planar, g, 4u, p->ws.planes, p->nzflag, p->needmask);
            else
                hipLaunchKernelGGL((k_planar_planes<false>), pg, dim3(256), 0, st, p->ws.planar, g, 4u, p->ws.planes, p->nzflag, (uint32_t*)nullptr);
            hipLaunchKernelGGL(k_nb_scan, dim3(1), dim3(1024), 0, st, p->needmask, (uint32_t)nblocks, p->nb_state, p->ws.nbuse, xd ? 1 : 0);
        }
        return 4;
    }
    if (g.kind == RSPT_HIP_KIND_XDELTA_HZR) {
        const uint32_t np = p->nb_host;
        launch_planes<BPS, true>(p, d_src, nblocks, 0, np, nullptr, st);
        return np;
    }
    if (g.kind == RSPT_HIP_KIND_HZR) {
        launch_planes<BPS, false>(p, d_src, nblocks, 0, 4, nullptr, st);
        return 4;
    }
    if (BPS == 4 && (g.nch & 3) == 0 && (g.ns & 3) == 0 && g.nch <= 1024 && (reinterpret_cast<uintptr_t>(d_src) & 15) == 0) {
        const uint32_t T4 = tile_i32x4(g);
        hipLaunchKernelGGL(k_tile_planar_i32x4, dim3((g.ns + T4 - 1) / T4, (unsigned)nblocks), dim3(256), g.nch * (T4 + 1) * 4, st, d_src, g, T4,
                           p->ws.planar, p->row_sum);
        p->have_row_sum = p->row_sum != nullptr;
        return 4;
    }
    dim3 grid((g.ns + p->T - 1) / p->T, (unsigned)nblocks);
    hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tile_planar<BPS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->in_lds);
    hipLaunchKernelGGL((k_tile_planar<BPS>), grid, dim3(256), p->in_lds, st, d_src, g, p->T, p->ws.planar);
    return 4;
}

// the front end of the two hzr packers over a planar source (planar.hip): planes [kfirst, kfirst + kcount); nbuse: the fix-up pass
template <bool XD>
static void launch_planar_stream(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, uint32_t kfirst, uint32_t kcount, const uint32_t* nbuse,
                                 hipStream_t st) {
    const Geom& g = p->g;
    const uint64_t units = (uint64_t)nblocks * ((g.N + 4095u) >> 12);
    const uint64_t want = 8ull * (uint64_t)p->num_cu;  // eight 256-thread workgroups per CU
    hipLaunchKernelGGL(k_planar_stream<XD>, dim3((uint32_t)(units < want ? units : want)), dim3(kPlanarThreads), 0, st, d_planar, g, kfirst, kcount, p->ws.planes,
                       p->needmask, p->nzflag, nbuse, (uint32_t)nblocks, nbuse ? nullptr : p->work_ctr + 1, p->nb_state, p->ws.nbuse, p->ws.plane_dirty,
                       p->dirty_shift);
}

// main front-end pass over a planar source (rspt_hip_compress_planar_batch_dev); returns the number of planes it wrote.  There is
// no native tile here: a wide handle takes the same route as a narrow one.
static uint32_t launch_front_planar(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, hipStream_t st) {
    const Geom& g = p->g;
    if (g.kind == RSPT_HIP_KIND_XDELTA_HZR) {
        const uint32_t np = p->nb_host;
        launch_planar_stream<true>(p, d_planar, nblocks, 0, np, nullptr, st);
        return np;
    }
    if (g.kind == RSPT_HIP_KIND_HZR) {
        launch_planar_stream<false>(p, d_planar, nblocks, 0, 4, nullptr, st);
        return 4;
    }
    // the transform packers work in place on ws.planar: the caller's matrix is copied there, cut to the sample width
    hipLaunchKernelGGL(k_planar_ingest, dim3((g.ns + 4095u) / 4096u, g.nch, (unsigned)nblocks), dim3(256), 0, st, d_planar, g, p->ws.planar, p->row_sum);
    p->have_row_sum = p->row_sum != nullptr;
    return 4;
}

// escalation fix-up: planes [np, 4) for the blocks whose nb grew past np in this call
// dct / idct of every channel of B blocks through the fp64 FFT path, `fft_bpp` blocks per pass (scratch bound)
template <bool FORWARD>
static void launch_dct_fft(rspt_hip_packer* p, uint32_t B, const int32_t* in, int32_t* out, hipStream_t st) {
    const Geom& g = p->g;
    const uint32_t l1 = p->fft_l1, l2 = p->fft_l2;
    const uint32_t lw = std::min(kFftLdsLog - l1, l2), lr = std::min(kFftLdsLog - l2, l1);
    const uint32_t lds_c = ((uint32_t)sizeof(double2) << (l1 + lw)) + ((uint32_t)sizeof(double2) << (l1 - 1)),
                   lds_r = ((uint32_t)sizeof(double2) << (l2 + lr)) + ((uint32_t)sizeof(double2) << (l2 - 1));  // points + stage twiddles
    hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dctfft_cols<FORWARD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_c);
    hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dctfft_rows<FORWARD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_r);
    const uint32_t fthr = 1024;  // 4096 points per workgroup: 256 threads (4 waves) left the LDS passes latency-bound (34 -> 46 GS/s)
    if (FORWARD && p->dct_real) {
        // real-input form (k_dctr_*): M = n/2 complex points, half the scratch round trip
        const uint32_t la = p->fftr_la, lb = p->fftr_lb;
        const uint32_t lwr = std::min(kFftLdsLog - la, lb);
        const uint32_t ldsc = ((uint32_t)sizeof(double2) << (la + lwr)) + ((uint32_t)sizeof(double2) << (la - 1));
        const uint32_t ldsr = ((uint32_t)sizeof(double2) << kFftLdsLog) + ((uint32_t)sizeof(double2) << (lb - 1));
        const uint32_t R = 1u << (kFftLdsLog - lb - 1), npairs = (1u << (la - 1)) - 1, ngroups = (npairs + R - 1) / R;
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dctr_cols), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsc);
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_dctr_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsr);
        for (uint32_t b0 = 0; b0 < B; b0 += (uint32_t)p->ws.fft_bpp) {
            const uint32_t nbk = std::min<uint32_t>((uint32_t)p->ws.fft_bpp, B - b0);
            hipLaunchKernelGGL(k_dctr_cols, dim3(1u << (lb - lwr), g.nch, nbk), dim3(fthr), ldsc, st, in, g, p->ws.mean_i32, p->fft_tw, p->ws.fft_scratch, la, lb, b0);
            hipLaunchKernelGGL(k_dctr_rows, dim3(ngroups + 1, g.nch, nbk), dim3(fthr), ldsr, st, p->ws.fft_scratch, g, p->fft_tw, p->fft_post, out, la, lb, b0,
                               p->dct_scale0, p->dct_scale1);
        }
        return;
    }
    if (!FORWARD && p->dct_real) {
        // real-output form (k_idctr_*)
        const uint32_t la = p->fftr_la, lb = p->fftr_lb;
        const uint32_t lwr = std::min(kFftLdsLog - la, lb), lrr = std::min(kFftLdsLog - lb, la);
        const uint32_t ldsc = ((uint32_t)sizeof(double2) << (la + lwr)) + ((uint32_t)sizeof(double2) << (la - 1));
        const uint32_t ldsr = ((uint32_t)sizeof(double2) << (lb + lrr)) + ((uint32_t)sizeof(double2) << (lb - 1));
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_idctr_cols), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsc);
        hipFuncSetAttribute(reinterpret_cast<const void*>(&k_idctr_rows), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsr);
        for (uint32_t b0 = 0; b0 < B; b0 += (uint32_t)p->ws.fft_bpp) {
            const uint32_t nbk = std::min<uint32_t>((uint32_t)p->ws.fft_bpp, B - b0);
            hipLaunchKernelGGL(k_idctr_cols, dim3(1u << (lb - lwr), g.nch, nbk), dim3(fthr), ldsc, st, in, g, p->fft_tw, p->fft_post, p->ws.fft_scratch, la, lb, b0,
                               p->dct_cs0);
            hipLaunchKernelGGL(k_idctr_rows, dim3(1u << (la - lrr), g.nch, nbk), dim3(fthr), ldsr, st, p->ws.fft_scratch, g, p->ws.means, p->fft_tw, out, la, lb, b0,
                               p->idct_scale);
        }
        return;
    }
    for (uint32_t b0 = 0; b0 < B; b0 += (uint32_t)p->ws.fft_bpp) {
        const uint32_t nbk = std::min<uint32_t>((uint32_t)p->ws.fft_bpp, B - b0);
        hipLaunchKernelGGL((k_dctfft_cols<FORWARD>), dim3(1u << (l2 - lw), g.nch, nbk), dim3(fthr), lds_c, st, in, g, p->ws.mean_i32, p->fft_tw,
                           p->fft_post, p->ws.fft_scratch, l1, l2, b0, p->dct_cs0);
        hipLaunchKernelGGL((k_dctfft_rows<FORWARD>), dim3(1u << (l1 - lr), g.nch, nbk), dim3(fthr), lds_r, st, p->ws.fft_scratch, g, p->ws.means,
                           p->fft_tw, p->fft_post, out, l1, l2, b0, FORWARD ? p->dct_scale0 : 0.0, FORWARD ? p->dct_scale1 : p->idct_scale);
    }
}

// WHT of rows longer than 65536 points, in place in `planar` (transforms.hip: k_fwht_seg / k_fwht_cross)
template <bool FORWARD>
static void launch_fwht_big(rspt_hip_packer* p, uint32_t B, hipStream_t st, const QLadder* lad = nullptr, const uint32_t* choice = nullptr) {
    const Geom& g = p->g;
    const uint32_t segs = g.ns >> 15;  // 32768-point pieces per row: 4 .. 128
    hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht_seg), hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * 4);
    hipLaunchKernelGGL(k_fwht_seg, dim3(segs, g.nch, B), dim3(1024), 32768 * 4, st, p->ws.planar, g);
    const uint32_t m1 = segs > 64u ? 64u : segs, m2 = segs / m1;
    // the last cross pass ends the transform: the truncating /n or + mean, or the general quantiser (k_fwht_cross_q)
    auto cross = [&](uint32_t m, uint32_t stride, uint32_t last) {
        const dim3 grid(g.ns / m / 256u, g.nch, B);
        if (last && lad)  // a ladder call: the divisor of each block's own entry (k_fwht_cross_l)
            hipLaunchKernelGGL((k_fwht_cross_l<FORWARD>), grid, dim3(256), 0, st, p->ws.planar, g, p->ws.means, p->ws.mean_i32, m, stride, last, *lad, choice);
        else if (last && p->had_quant)
            hipLaunchKernelGGL((k_fwht_cross_q<FORWARD>), grid, dim3(256), 0, st, p->ws.planar, g, p->ws.means, p->ws.mean_i32, m, stride, last,
                               FORWARD ? p->had_div_fwd : p->had_div_inv);
        else
            hipLaunchKernelGGL((k_fwht_cross<FORWARD>), grid, dim3(256), 0, st, p->ws.planar, g, p->ws.means, p->ws.mean_i32, m, stride, last);
    };
    cross(m1, 32768u, m2 == 1u ? 1u : 0u);
    if (m2 > 1u) cross(m2, 32768u * m1, 1u);
}

// The quantiser of a lossy handle from the reference's `quality` constant, in the reference's evaluation order: the three dct
// scales (signal_packer_dct.cpp:84, 97: `Cs[i] * ratio1 / quality` with Cs a float, `ratio1 * quality`) or the two hadamard
// divisors (fwht.c:33, 39: `n / ratio` with n an int, `ratio`).  Shared by rspt_hip_packer_create and rspt_hip_set_quantizer.
// false, and the handle as it was: a quality the arithmetic cannot take -- not finite, not > 0, or one that leaves a scale or
// a divisor that is not finite and non-zero.  commit = false only asks whether q can be taken.  quantizer_of is the arithmetic
// alone, for a handle's shape: the ladder entries take theirs from it too.
struct Quantizer {
    double dct_scale0, dct_scale1, idct_scale;
    float dct_cs0;
    double had_div_fwd, had_div_inv;
};
static bool quantizer_of(const Geom& g, double q, Quantizer* out) {
    auto usable = [](double v) { return std::isfinite(v) && v != 0.0; };
    if (!std::isfinite(q) || !(q > 0.0)) return false;
    Quantizer z{};
    if (g.kind == RSPT_HIP_KIND_DCT) {
        const double ratio1 = sqrt(2.0 / (double)(int)g.ns);
        const float cs0 = (float)(1 / sqrt(2));
        z.dct_cs0 = cs0;
        z.dct_scale0 = cs0 * ratio1 / q;   // Cs[0]*ratio1/quality (dct.cpp:84)
        z.dct_scale1 = 1.0f * ratio1 / q;  // Cs[i>0] = 1
        z.idct_scale = ratio1 * q;         // dct.cpp:97
        if (!usable(z.dct_scale0) || !usable(z.dct_scale1) || !usable(z.idct_scale)) return false;
    } else if (g.kind == RSPT_HIP_KIND_HADAMARD) {
        z.had_div_fwd = (double)(int)g.ns / q;  // fwht_normalize: src[i] /= (n / ratio)
        z.had_div_inv = q;                      // fwht_normalize2: src[i] /= ratio
        if (!usable(z.had_div_fwd)) return false;
    } else {
        return false;
    }
    *out = z;
    return true;
}

static bool set_quality(rspt_hip_packer* p, double q, bool commit = true) {
    Quantizer z;
    if (!quantizer_of(p->g, q, &z)) return false;
    if (!commit) return true;
    if (p->g.kind == RSPT_HIP_KIND_DCT) {
        p->dct_cs0 = z.dct_cs0;
        p->dct_scale0 = z.dct_scale0;
        p->dct_scale1 = z.dct_scale1;
        p->idct_scale = z.idct_scale;
    } else {
        p->had_div_fwd = z.had_div_fwd;
        p->had_div_inv = z.had_div_inv;
        p->had_quant = q != 1.0;  // quality 1: the all-integer kernels (truncating /n, and no division on the way back)
    }
    p->quality = q;
    return true;
}

// The quantisers of a ladder call (rspt_hip_compress_batch_ladder_dev and its kin): every entry through quantizer_of, as kernel
// arguments -- nothing goes to the device ahead of the launch.  fwd / inv: what the forward and the inverse transform kernels take.
struct LadderSel {
    QLadder fwd, inv;
    const uint32_t* choice;
};

// RSPT_HIP_ERR_UNSUPPORTED: a kind or a path the ladder kernels do not cover; RSPT_HIP_ERR_ARG: no ladder, more than kMaxLadder
// entries, or an entry that rspt_hip_set_quantizer would not take
static int make_ladder(const rspt_hip_packer* p, const double* ladder, size_t nladder, const uint32_t* d_choice, LadderSel* out) {
    const Geom& g = p->g;
    if (g.kind != RSPT_HIP_KIND_HADAMARD && !(g.kind == RSPT_HIP_KIND_DCT && !p->dct_fft)) return RSPT_HIP_ERR_UNSUPPORTED;
    if (!ladder || nladder < 1 || nladder > kMaxLadder) return RSPT_HIP_ERR_ARG;
    LadderSel ls{};
    for (size_t k = 0; k < nladder; ++k) {
        Quantizer z;
        if (!quantizer_of(g, ladder[k], &z)) return RSPT_HIP_ERR_ARG;
        if (g.kind == RSPT_HIP_KIND_DCT) {
            ls.fwd.a[k] = z.dct_scale0, ls.fwd.b[k] = z.dct_scale1;
            ls.inv.b[k] = z.idct_scale;
        } else {
            ls.fwd.a[k] = z.had_div_fwd;
            ls.inv.a[k] = z.had_div_inv;
        }
    }
    ls.fwd.n = ls.inv.n = (uint32_t)nladder;
    ls.choice = d_choice;
    *out = ls;
    return RSPT_HIP_OK;
}

template <int BPS>
static void launch_fixup(rspt_hip_packer* p, const uint8_t* d_src, size_t nblocks, uint32_t np, hipStream_t st) {
    launch_planes<BPS, true>(p, d_src, nblocks, np, 4 - np, p->ws.nbuse, st);
}

// The reference's channel limit: convert_native_to_i32 / convert_i32_to_native, which every one of its programs runs first and
// last, count channels with a uint16_t (utils.cpp:57, 129) -- 65536 channels never terminate there.
static constexpr size_t kMaxChannels = 65535;

template <int BPS>
static void launch_wide_native(const Geom& g, const int32_t* planar, uint8_t* dst, uint32_t B, hipStream_t st) {
    hipLaunchKernelGGL(k_wide_native<BPS>, dim3((g.ns + 63) / 64, (g.nch + 63) / 64, B), dim3(256), 0, st, planar, g, dst);
}

template <bool XDELTA, int CG>
static void launch_inv_native(rspt_hip_packer* p, uint32_t B, uint32_t nrow, void* d_dst, hipStream_t st) {
    const Geom& g = p->g;
    constexpr uint32_t S = (1024u / CG) * 16u, lds = CG * (S + 1u) * 4u;  // > 64 KiB: the limit is raised per kernel
    hipFuncSetAttribute(reinterpret_cast<const void*>(&k_inv_native<XDELTA, CG>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const dim3 ng((g.ns + S - 1) / S, (g.nch + CG - 1) / CG, B);
    hipLaunchKernelGGL((k_inv_native<XDELTA, CG>), ng, dim3(1024), lds, st, p->ws.planes, g, p->ws.dec_nb, nrow, p->ws.txor, p->ws.tsum, (uint8_t*)d_dst);
}

extern "C" {

const char* rspt_hip_status_string(int s) {
    switch (s) {
        case RSPT_HIP_OK: return "ok";
        case RSPT_HIP_ERR_ARG: return "invalid argument";
        case RSPT_HIP_ERR_NO_DEVICE: return "no usable gfx950 device (there is no CPU path)";
        case RSPT_HIP_ERR_ALLOC: return "allocation failed";
        case RSPT_HIP_ERR_LAUNCH: return "HIP call or kernel launch failed";
        case RSPT_HIP_ERR_DST_TOO_SMALL: return "destination too small for the compressed stream";
        case RSPT_HIP_ERR_CORRUPT: return "malformed stream";
        case RSPT_HIP_ERR_UNSUPPORTED: return "shape not supported by the kernels";
        case RSPT_HIP_ERR_BUSY: return "every slot of the feed is in flight";
        default: return "unknown status";
    }
}

int rspt_hip_last_hip_error(const rspt_hip_packer* p) { return p ? p->last_hip_error : 0; }

int rspt_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int rspt_hip_packer_create(rspt_hip_packer** out, int kind_and_flags, size_t bps, size_t nch, size_t ns, size_t nb, int device) {
    if (!out) return RSPT_HIP_ERR_ARG;
    *out = nullptr;
    const bool force_fft = (kind_and_flags & RSPT_HIP_DCT_FORCE_FFT) != 0;  // (test hook, see rspt_hip.h)
    const int kind = kind_and_flags & ~RSPT_HIP_DCT_FORCE_FFT;
    if (kind < 0 || kind > RSPT_HIP_KIND_BYTES || bps < 1 || bps > 4 || nch == 0 || ns == 0) return RSPT_HIP_ERR_ARG;
    if (kind == RSPT_HIP_KIND_BYTES && (bps != 1 || nch != 1)) return RSPT_HIP_ERR_ARG;  // a byte buffer of ns bytes (nb is ignored)
    if ((unsigned long long)nch * ns >= (1ull << 31)) return RSPT_HIP_ERR_ARG;  // the reference indexes with int
    if (nch > kMaxChannels) return RSPT_HIP_ERR_UNSUPPORTED;  // the reference's converters count channels in a uint16_t (utils.cpp:57, 129)
    if (kind == RSPT_HIP_KIND_XDELTA_HZR && (nb < 1 || nb > 4)) return RSPT_HIP_ERR_ARG;
    if (kind == RSPT_HIP_KIND_HADAMARD && (ns & (ns - 1))) return RSPT_HIP_ERR_ARG;  // fwht.c needs n = 2^k
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return RSPT_HIP_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return RSPT_HIP_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return RSPT_HIP_ERR_NO_DEVICE;  // code objects are gfx950 only
    if (hipSetDevice(device) != hipSuccess) return RSPT_HIP_ERR_NO_DEVICE;

    std::unique_ptr<rspt_hip_packer> p(new (std::nothrow) rspt_hip_packer());  // (released on every error exit)
    if (!p) return RSPT_HIP_ERR_ALLOC;
    p->device = device;
    Geom& g = p->g;
    g.bps = (uint32_t)bps;
    g.nch = (uint32_t)nch;
    g.ns = (uint32_t)ns;
    g.N = (uint32_t)(nch * ns);
    g.nblk = (g.N + kHzrBlock - 1) / kHzrBlock;
    g.kind = (uint32_t)kind;
    g.hdr_len = (kind == RSPT_HIP_KIND_DCT || kind == RSPT_HIP_KIND_HADAMARD) ? 3u * g.nch : 0u;
    g.method = kind == RSPT_HIP_KIND_DCT ? 1u : kind == RSPT_HIP_KIND_HADAMARD ? 2u : 0u;
    g.plane_stride = ((uint64_t)g.N + 255ull) & ~255ull;
    g.block_bytes = (uint64_t)bps * nch * ns;
    p->nb_host = p->nb_ctor = kind == RSPT_HIP_KIND_HZR ? 4u : kind == RSPT_HIP_KIND_DCT ? 2u : kind == RSPT_HIP_KIND_HADAMARD ? 3u : kind == RSPT_HIP_KIND_BYTES ? 1u : (unsigned)nb;

    // tile geometry
    {
        const uint64_t rowb = (uint64_t)g.nch * g.bps;
        const uint32_t ns16 = (g.ns + 15u) & ~15u;
        // k_tile_planar stages the contiguous input tile (T*nch*bps + 32 bytes) in LDS
        uint64_t t = (64 * 1024 - 32) / rowb;
        t &= ~15ull;
        if (t < 16) {  // a 16-sample tile of all channels does not fit: the wide-block front end (k_wide_planar), any packer
            p->wide = true;
            t = 16;
        }
        p->T = (uint32_t)(t > 4096 ? 4096 : t);
        if (p->T > ns16) p->T = ns16;
        p->in_lds = (uint32_t)(((uint64_t)p->T * rowb + 16 + 15) & ~15ull);
        // k_tile_planes keeps only the plane rows in LDS: kcount*nch*(Tp+16) + 32*nch bytes, <= 79 KiB
        // (two workgroups per CU).  Long row segments matter more than occupancy here: 256-byte plane
        // rows beat 64-byte ones by 2.5x (profiles/r01_tile_sweep.txt); segments that are whole 128-byte
        // lines beat ragged ones of about the same length (384 vs 352: -4 %).
        for (uint32_t kc = 1; kc <= 4; ++kc) {
            auto fit = [&](uint64_t budget) -> uint32_t {
                const uint64_t fixed = (16ull * kc + 32ull) * g.nch + 96;  // row padding, non-zero dedupe masks, escalation word + dirty bits
                if (budget <= fixed) return 0;
                uint64_t tt = (budget - fixed) / ((uint64_t)kc * g.nch);
                tt &= tt >= 256 ? ~127ull : ~15ull;
                return (uint32_t)(tt > 2048 ? 2048 : tt);
            };
            uint32_t Tp = fit(79 * 1024);
            if (Tp < 16) Tp = fit(150 * 1024);
#ifdef RSPT_DIAG
            if (const char* e = getenv("RSPT_TILE")) Tp = (uint32_t)atoi(e) & ~15u;  // tuning knob (diagnostic builds only)
#endif
            if (Tp < 16) {  // the plane rows of a 16-sample tile do not fit either way (about a thousand channels and up)
                p->wide = true;
                Tp = 16;
            }
            if (Tp > ns16) Tp = ns16;
            p->Tp[kc] = Tp;
        }
    }
#ifdef RSPT_DIAG  // timing probes and tuning knobs: never in the product library
    if (const char* e = getenv("RSPT_ABLATE")) p->ablate = (uint32_t)atoi(e);
    if (const char* e = getenv("RSPT_PLANESEL")) p->psel = (uint32_t)atoi(e);
    if (const char* e = getenv("RSPT_K1_THREADS")) p->k1_threads = (uint32_t)atoi(e) / 64 * 64;
    if (const char* e = getenv("RSPT_K1_GRID")) p->k1_grid = (uint32_t)atoi(e);
    if (const char* e = getenv("RSPT_HIST_GRID")) p->hist_grid = (uint32_t)atoi(e);
    if (const char* e = getenv("RSPT_ENC_GRID")) p->enc_grid = (uint32_t)atoi(e);
    if (const char* e = getenv("RSPT_QP_FORM")) p->qp_form = (uint32_t)atoi(e);
#endif
    if (p->k1_threads < 64 || p->k1_threads > 256) p->k1_threads = 256;  // (k_tile_planes is compiled for <= 256)
    p->ntile = (g.N + kInvTile - 1) / kInvTile;
    {
        // k_planar_native tile: nch rows of (T+1) int32 within 64 KiB
        uint32_t T = (uint32_t)(65536ull / (4ull * g.nch));
        T = T > 1 ? T - 1 : 0;
        if (T > 1024) T = 1024;
        p->Tn_native = T;  // (0 beyond 8192 channels: decompress ends in k_wide_native, convert.hip)
    }
    if (kind == RSPT_HIP_KIND_HADAMARD && ns > (1u << 22)) return RSPT_HIP_ERR_UNSUPPORTED;  // (up to 65536 one workgroup per channel; beyond, two passes: launch_fwht_big)
    if (kind == RSPT_HIP_KIND_DCT) {
        // The reference's dense n x n table (bit-exact) for every n it can run itself -- its table index `(2x+1)*i` is an
        // int (signal_packer_dct.cpp:60-74): n <= 32768 -- except n = 2^k > 8192, which take the fp64 FFT path (PRDN / CR
        // tolerance) as do the sizes beyond the reference's reach, n = 2^k <= 2^22.  The table is n^2 floats twice over
        // (8.6 GB at 32768).  RSPT_HIP_DCT_FORCE_FFT forces the FFT path for small n = 2^k (cross-check against the table).
        const bool pow2 = (ns & (ns - 1)) == 0;
        p->dct_fft = (ns > 8192 && pow2) || (force_fft && pow2 && ns >= 16);
        if (p->dct_fft ? ns > (1u << 22) : ns > 32768) return RSPT_HIP_ERR_UNSUPPORTED;
        if (p->dct_fft) {
            uint32_t k = 0;
            while ((1ull << k) < ns) ++k;
            p->fft_l1 = (k + 1) / 2;
            p->fft_l2 = k / 2;
            bool real_form = true;
#ifdef RSPT_DIAG
            if (const char* noreal = getenv("RSPT_DCT_REAL")) real_form = atoi(noreal) != 0;  // complex-input form, for comparison
#endif
            if (k >= 8 && real_form) {  // n/2 = m1*m2 with m2 = 64 where it can be (whole-line output runs)
                const uint32_t lM = k - 1;
                p->fftr_lb = lM > 18 ? lM - 12 : 6;
                p->fftr_la = lM - p->fftr_lb;
                p->dct_real = true;
            }
        }
    }
    if (hipStreamCreateWithFlags(p->stream.out(), hipStreamNonBlocking) != hipSuccess) return RSPT_HIP_ERR_LAUNCH;
    p->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (hipMalloc(p->stamps.out(), (512 * 16 * 8 + 2 * 16384) * sizeof(unsigned long long)) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
    {
        // ~87 KB of constants, computed once per process (a function-local static: packers are created from several host
        // threads at once -- one per device, tests/cxx/shard_devices.cpp -- and the initialisation of such a static is thread-safe)
        static const CrcConsts& cc = *[] {
            CrcConsts* c = new CrcConsts;
            make_crc_consts(*c);
            return c;
        }();
        if (hipMalloc(p->crc.out(), sizeof(CrcConsts)) != hipSuccess || hipMalloc(p->nb_state.out(), 4 * sizeof(uint32_t)) != hipSuccess)
            return RSPT_HIP_ERR_ALLOC;
        uint32_t nb0 = p->nb_ctor;
        if (hipMemcpy(p->crc, &cc, sizeof(cc), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(p->nb_state, &nb0, sizeof(nb0), hipMemcpyHostToDevice) != hipSuccess)
            return RSPT_HIP_ERR_LAUNCH;
    }
    for (int i = 0; i <= ST_COUNT; ++i) hipEventCreate(p->ev[i].out());
    // the reference's constants (signal_packer_dct.cpp:39, signal_packer_hadamard.cpp:37)
    if ((kind == RSPT_HIP_KIND_DCT && !set_quality(p.get(), 128.0)) || (kind == RSPT_HIP_KIND_HADAMARD && !set_quality(p.get(), 1.0)))
        return RSPT_HIP_ERR_ARG;
    if (kind == RSPT_HIP_KIND_DCT && p->dct_fft) {
        const size_t n = ns;
        std::vector<double2> tw(n), post(n);
        const double PI = 3.14159265358979323846;
        for (size_t t = 0; t < n; ++t) {
            const double a = 2.0 * PI * (double)t / (double)n, b = PI * (double)t / (2.0 * (double)n);
            tw[t] = make_double2(cos(a), sin(a));
            post[t] = make_double2(cos(b), sin(b));
        }
        if (hipMalloc(p->fft_tw.out(), n * sizeof(double2)) != hipSuccess || hipMalloc(p->fft_post.out(), n * sizeof(double2)) != hipSuccess)
            return RSPT_HIP_ERR_ALLOC;
        if (hipMemcpy(p->fft_tw, tw.data(), n * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(p->fft_post, post.data(), n * sizeof(double2), hipMemcpyHostToDevice) != hipSuccess)
            return RSPT_HIP_ERR_LAUNCH;
    } else if (kind == RSPT_HIP_KIND_DCT) {
        // init_cos_table (signal_packer_dct.cpp:60-74), host libm, same expression and types.  Built in slabs of rows by
        // all host threads (10^9 cosines at n = 32768) and uploaded slab by slab; the transposed copy is made on the device.
        const size_t n = ns;
        if (hipMalloc(p->cos_tab.out(), n * n * sizeof(float)) != hipSuccess || hipMalloc(p->cos_tab_t.out(), n * n * sizeof(float)) != hipSuccess)
            return RSPT_HIP_ERR_ALLOC;
        const double PI = 3.14159265358979323846;
        const double pi_n_2 = PI / ((double)(int)n * 2.0);
        const size_t slab = std::max<size_t>(1, std::min<size_t>(n, (64u << 20) / (n * sizeof(float))));
        std::vector<float> tab(slab * n);
        unsigned nthr = std::thread::hardware_concurrency();
        nthr = nthr < 1 ? 1 : nthr > 32 ? 32 : nthr;
        for (size_t x0 = 0; x0 < n; x0 += slab) {
            const size_t nr = std::min(slab, n - x0);
            auto fill = [&](size_t r0, size_t r1) {
                for (size_t x = x0 + r0; x < x0 + r1; ++x)
                    for (size_t i = 0; i < n; ++i) {
                        const int arg = ((int)x << 1) * (int)i + (int)i;
                        tab[(x - x0) * n + i] = (float)cos(arg * pi_n_2);
                    }
            };
            if (nr * n < (1u << 20) || nthr == 1) {
                fill(0, nr);
            } else {
                std::vector<std::thread> th;
                for (unsigned t = 0; t < nthr; ++t) th.emplace_back(fill, nr * t / nthr, nr * (t + 1) / nthr);
                for (auto& t : th) t.join();
            }
            if (hipMemcpy(p->cos_tab + x0 * n, tab.data(), nr * n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return RSPT_HIP_ERR_LAUNCH;
        }
        hipLaunchKernelGGL(k_transpose_f32, dim3((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32)), dim3(256), 0, 0, p->cos_tab, p->cos_tab_t,
                           (uint32_t)n);
        if (hipGetLastError() != hipSuccess) return RSPT_HIP_ERR_LAUNCH;
    }
    // setup copies ran on the null stream; the handle's stream does not wait for it
    if (hipDeviceSynchronize() != hipSuccess) return RSPT_HIP_ERR_LAUNCH;
    *out = p.release();
    return RSPT_HIP_OK;
}

void rspt_hip_packer_destroy(rspt_hip_packer* p) {
    if (!p) return;
    hipSetDevice(p->device);
    // An open feed ends first: its partly filled group is still submitted, and that launch needs the workspace and constants.
    if (p->feed) rspt_hip_feed_end(p);
    const hipStream_t streams[] = {p->stream, p->lag.stream};
    for (hipStream_t s : streams)
        if (s) hipStreamSynchronize(s);
    p->fir.wait_all();  // (the FIR and median stages run on the caller's streams)
    p->med.last.wait();
    delete p;  // the members go in reverse order of construction
}

size_t rspt_hip_block_bytes(const rspt_hip_packer* p) { return p ? (size_t)p->g.block_bytes : 0; }

size_t rspt_hip_max_compressed_size(const rspt_hip_packer* p) {
    if (!p) return 0;
    // (a lossy handle never escalates: the planes of its current setting, rspt_hip_set_quantizer)
    const bool lossy = p->g.kind == RSPT_HIP_KIND_DCT || p->g.kind == RSPT_HIP_KIND_HADAMARD;
    const unsigned nbmax = p->g.kind == RSPT_HIP_KIND_XDELTA_HZR ? 4u : lossy ? p->nb_host : p->nb_ctor;
    const size_t hzr_max = 4 + (size_t)p->g.N + 7ull * p->g.nblk;  // hzr_encode.c:489-497
    if (p->g.kind == RSPT_HIP_KIND_BYTES) return hzr_max;  // the bare stream
    return 1 + p->g.hdr_len + (size_t)nbmax * (4 + hzr_max);
}

size_t rspt_hip_hzr_max_compressed_size(size_t uncompressed_size) {  // hzr_encode.c:489-497
    return 4 + (uncompressed_size ? uncompressed_size + 7 * ((uncompressed_size + kHzrBlock - 1) / kHzrBlock) : 0);
}

// block slots (four planes each) that `nblocks` blocks take: a bare-stream handle keeps buffer i in flat plane i
static size_t slots_of(const rspt_hip_packer* p, size_t nblocks) { return p->g.kind == RSPT_HIP_KIND_BYTES ? (nblocks + 3) / 4 : nblocks; }

int rspt_hip_reserve(rspt_hip_packer* p, size_t max_blocks) {
    if (!p || max_blocks == 0) return RSPT_HIP_ERR_ARG;
    if (max_blocks <= p->ws.cap_blocks) return RSPT_HIP_OK;
    if (max_blocks > 65535) return RSPT_HIP_ERR_ARG;  // grid.y / grid.z limit; shard larger batches
    HIPCHK(p, hipSetDevice(p->device));
    HIPCHK(p, hipStreamSynchronize(p->stream));
    p->ws = Workspace();  // (released before the new one is made: the two are never held at once)
    const Geom& g = p->g;
    Workspace w;
    // Everything per plane or per hzr block is sized by block slots: for a bare-stream handle a quarter of the blocks (one
    // plane per buffer), and it needs none of the int32 / scan buffers of the sample packers.
    const bool bare = g.kind == RSPT_HIP_KIND_BYTES;
    const size_t slots = slots_of(p, max_blocks);
    const size_t nhb = slots * kMaxPlanes * g.nblk;
    bool ok = true;
    ok &= hipMalloc(w.planes.out(), slots * kMaxPlanes * g.plane_stride + 4096) == hipSuccess;
    ok &= hipMalloc(w.nbuse.out(), max_blocks * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.dec_nb.out(), max_blocks * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.plane_dirty.out(), slots * kMaxPlanes * 4 * sizeof(uint32_t)) == hipSuccess;
    // one region zeroed per call by a single memset: [nzflag: B*4*nblk][needmask: B][work counters: 16]; the last two are
    // placed per call right behind the part of nzflag in use
    w.zcap_words = nhb + max_blocks + 32 + 2 * max_blocks * (size_t)g.nch + 2;
    for (int i = 0; i < 2; ++i) ok &= hipMalloc(w.zbuf[i].out(), w.zcap_words * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.big_list.out(), nhb * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.staging.out(), nhb * (size_t)kStageSlotWords * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.hist.out(), nhb * kSymStride * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.cw.out(), nhb * kSymStride * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.seghist.out(), nhb * (size_t)kSegHistStride * sizeof(uint16_t)) == hipSuccess;
    ok &= hipMalloc(w.segbase.out(), nhb * (size_t)kEncWaves * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.lists.out(), nhb * (size_t)kEncWaves * kListCap * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.listinfo.out(), nhb * (size_t)kEncWaves * sizeof(uint2)) == hipSuccess;
    ok &= hipMalloc(w.tdesc.out(), nhb * kTdescWords * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.meta.out(), nhb * sizeof(BlockMeta)) == hipSuccess;
    ok &= hipMalloc(w.out_off.out(), nhb * sizeof(uint64_t)) == hipSuccess;
    ok &= hipMalloc(w.means.out(), max_blocks * (size_t)(g.hdr_len ? g.hdr_len : 4)) == hipSuccess;
    // planar int32 scratch: transform packers on compress, every packer on decompress
    if (!bare) ok &= hipMalloc(w.planar.out(), max_blocks * (size_t)g.N * sizeof(int32_t) + 4096) == hipSuccess;
    const size_t nscan = std::max<size_t>(p->ntile, g.N / kRowTile + 1);  // tiles of 4096, or row tiles of 256 (k_inv_native)
    if (!bare) ok &= hipMalloc(w.txor.out(), max_blocks * nscan * sizeof(uint32_t)) == hipSuccess;
    if (!bare) ok &= hipMalloc(w.tsum.out(), max_blocks * nscan * sizeof(uint32_t)) == hipSuccess;
    if (g.ns % kRowTile == 0 && g.bps == 4) ok &= hipMalloc(w.rowrec.out(), max_blocks * (g.N / kRowTile) * (size_t)kRowRec * sizeof(uint32_t)) == hipSuccess;
    ok &= hipMalloc(w.blk_off.out(), nhb * sizeof(uint64_t)) == hipSuccess;
    if (g.kind == RSPT_HIP_KIND_DCT) ok &= hipMalloc(w.planar2.out(), max_blocks * (size_t)g.N * sizeof(int32_t) + 4096) == hipSuccess;
    if (g.kind == RSPT_HIP_KIND_HADAMARD && g.ns > 65536u) ok &= hipMalloc(w.mean_i32.out(), max_blocks * (size_t)g.nch * sizeof(int32_t)) == hipSuccess;
    if (g.kind == RSPT_HIP_KIND_DCT && p->dct_fft) {
        const size_t per_block = (size_t)g.N * sizeof(double2);
        w.fft_bpp = std::max<size_t>(1, std::min<size_t>(max_blocks, ((size_t)1 << 30) / per_block));
        ok &= hipMalloc(w.fft_scratch.out(), w.fft_bpp * per_block) == hipSuccess;
        ok &= hipMalloc(w.mean_i32.out(), max_blocks * (size_t)g.nch * sizeof(int32_t)) == hipSuccess;
    }
    ok &= hipMalloc(w.quality.out(), max_blocks * quality_words(g.nch) * sizeof(unsigned long long)) == hipSuccess;
    if (g.kind == RSPT_HIP_KIND_DCT || g.kind == RSPT_HIP_KIND_HADAMARD) {
        ok &= hipMalloc(w.idx_choice.out(), max_blocks * sizeof(uint32_t)) == hipSuccess;
        ok &= hipMalloc(w.pack_sizes.out(), max_blocks * sizeof(uint64_t)) == hipSuccess;
        ok &= hipMalloc(w.target_tab.out(), rate_work::Tables(max_blocks * kMaxLadder).bytes) == hipSuccess;
    }
    if (!ok) return RSPT_HIP_ERR_ALLOC;
    // the clean-plane invariant starts from zeroed planes
    HIPCHK(p, hipMemset(w.planes, 0, slots * kMaxPlanes * g.plane_stride + 4096));
    HIPCHK(p, hipMemset(w.plane_dirty, 0, slots * kMaxPlanes * 4 * sizeof(uint32_t)));
    p->dirty_shift = 0;
    while (((g.nblk - 1) >> p->dirty_shift) >= 128u) ++p->dirty_shift;
    HIPCHK(p, hipDeviceSynchronize());  // (the calls that follow may come on any stream)
    w.cap_blocks = max_blocks;
    w.cap_slots = slots;
    p->ws = std::move(w);
    p->nzflag = p->ws.zbuf[0];
    return RSPT_HIP_OK;
}

// The transform of the two lossy packers in a compress call, behind the front end's planar block in ws.planar: the coefficients'
// low bytes leave as planes.  nzflag: where the plane kernels mark the non-zero segments (a compress call: the zero region).
// ls: a ladder call -- the transform kernels take each block's quantiser from its ladder entry, not the handle's.
static void launch_forward_transform(rspt_hip_packer* p, uint32_t B, hipStream_t st, uint32_t* nzflag, const LadderSel* ls) {
    const Geom& g = p->g;
    const uint32_t lossy_nb = p->nb_host;  // nr_bytes_to_compress_ of the lossy packers (rspt_hip_set_quantizer): they never escalate
    if (g.kind == RSPT_HIP_KIND_HADAMARD) {
        // per channel: mean removal, WHT, truncating /n (signal_packer_hadamard.cpp:57-72); with a quality other than 1 the
        // kernels that divide by n / quality instead (transforms.hip: QUANT)
        const uint32_t fw_lds = (g.ns > 32768u ? 32768u : g.ns) * 4u;
        if (g.ns > 65536u) {  // two passes over the planar row (any 2^k the reference's own transform takes, fwht.c:4-28)
            hipLaunchKernelGGL(k_row_means, dim3(g.nch, B), dim3(1024), 0, st, p->ws.planar, g, p->ws.means, p->ws.mean_i32);
            launch_fwht_big<true>(p, B, st, ls ? &ls->fwd : nullptr, ls ? ls->choice : nullptr);
            hipLaunchKernelGGL((k_planar_planes<false>), dim3((g.N + 4095) / 4096, B), dim3(256), 0, st, p->ws.planar, g, lossy_nb, p->ws.planes, nzflag, (uint32_t*)nullptr);
        } else if (g.ns == 65536u) {  // the whole row in registers: read once, and the byte planes written straight from them
            if (ls) {
                hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht64k_l<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
                hipLaunchKernelGGL((k_fwht64k_l<true, true>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, p->ws.planes, nzflag,
                                   lossy_nb, ls->fwd, ls->choice);
            } else if (p->had_quant) {
                hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht64k_q<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
                hipLaunchKernelGGL((k_fwht64k_q<true, true>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, p->ws.planes, nzflag,
                                   lossy_nb, p->had_div_fwd);
            } else {
                hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht64k<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
                hipLaunchKernelGGL((k_fwht64k<true, true>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, p->ws.planes, nzflag,
                                   lossy_nb);
            }
        } else {
            if (ls) {
                hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht_l<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
                hipLaunchKernelGGL((k_fwht_l<true>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, ls->fwd, ls->choice);
            } else if (p->had_quant) {
                hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht_q<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
                hipLaunchKernelGGL((k_fwht_q<true>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, p->had_div_fwd);
            } else {
                hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
                hipLaunchKernelGGL((k_fwht<true>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means);
            }
            hipLaunchKernelGGL((k_planar_planes<false>), dim3((g.N + 4095) / 4096, B), dim3(256), 0, st, p->ws.planar, g, lossy_nb, p->ws.planes, nzflag, (uint32_t*)nullptr);
        }
    } else if (g.kind == RSPT_HIP_KIND_DCT) {
        if (p->dct_fft) {
            if (p->have_row_sum)  // the de-interleave pass summed the channels on its way: no second pass over the planar block
                hipLaunchKernelGGL(k_means_from_sums, dim3((B * g.nch + 255) / 256), dim3(256), 0, st, p->row_sum, g, B, p->ws.means, p->ws.mean_i32);
            else
                hipLaunchKernelGGL(k_row_means, dim3(g.nch, B), dim3(1024), 0, st, p->ws.planar, g, p->ws.means, p->ws.mean_i32);
            launch_dct_fft<true>(p, B, p->ws.planar, p->ws.planar2, st);
        } else if (ls) {
            hipLaunchKernelGGL((k_dct_l<true>), dim3((g.ns + 255) / 256, (g.nch + kDctCh - 1) / kDctCh, B), dim3(256), 0, st, p->ws.planar, g, p->ws.means,
                               p->cos_tab, ls->fwd, ls->choice, p->dct_cs0, p->ws.planar2);
        } else {
            hipLaunchKernelGGL((k_dct<true>), dim3((g.ns + 255) / 256, (g.nch + kDctCh - 1) / kDctCh, B), dim3(256), 0, st, p->ws.planar, g, p->ws.means,
                               p->cos_tab, p->dct_scale0, p->dct_scale1, p->dct_cs0, p->ws.planar2);
        }
        hipLaunchKernelGGL((k_planar_planes<true>), dim3((g.N + 4095) / 4096, B), dim3(256), 0, st, p->ws.planar2, g, lossy_nb, p->ws.planes, nzflag, (uint32_t*)nullptr);
    }
}

// What every compress pass starts with, for `nblocks` blocks: the views into the per-call zero region -- the copy the pass works in,
// zeroed here only where the call before has not done it -- and, where something else wrote the planes, every plane flagged dirty.
static int front_begin(rspt_hip_packer* p, size_t nblocks, hipStream_t st) {
    const Geom& g = p->g;
    const size_t nhb_call = slots_of(p, nblocks) * kMaxPlanes * g.nblk;
    p->nzflag = p->ws.zbuf[p->ws.zset];
    p->needmask = p->nzflag + nhb_call;
    p->work_ctr = p->needmask + ((nblocks + 3) & ~(size_t)3);
    size_t zwords = (size_t)((p->work_ctr + 16) - p->nzflag);
    p->row_sum = nullptr;
    p->have_row_sum = false;
    if (g.kind == RSPT_HIP_KIND_DCT && p->dct_fft) {  // channel sums of the de-interleave pass, 8-byte aligned behind the counters
        zwords = (zwords + 1) & ~(size_t)1;
        p->row_sum = reinterpret_cast<long long*>(p->nzflag + zwords);
        zwords += 2 * nblocks * (size_t)g.nch;
    }
    if (!p->ws.zero_ready[p->ws.zset]) HIPCHK(p, hipMemsetAsync(p->nzflag, 0, zwords * sizeof(uint32_t), st));  // (first call, or after a failed one)
    p->ws.zero_ready[0] = p->ws.zero_ready[1] = false;  // this copy is in use now; the other one becomes ready once k_tree is launched
    if (p->ws.planes_unknown || (p->ablate & ~(3u << 26)) || p->psel) {  // (diagnostic runs skip kernels and stores: never trust the planes they leave; probes 26 / 27 store everything)
        HIPCHK(p, hipMemsetAsync(p->ws.plane_dirty, 0xFF, p->ws.cap_slots * kMaxPlanes * 4 * sizeof(uint32_t), st));
        p->ws.planes_unknown = false;
    }
    return RSPT_HIP_OK;
}

// ---- the compress sequence, phase by phase ----------------------------------------------------------------------------------------
// (Round 4 measured whether the phases of TWO batches can overlap -- two whole batches racing on two streams, and an ordered
// schedule with the latency-bound middle of batch i on a second stream beside the front end of batch i+1: neither beats one
// batch at a time on one stream; profiles/r04_notes.md, profiles/r04_pipeline_experiment.patch.)
// front:  zero region, front-end kernel(s), escalation scan / fix-up, list of k_hist's blocks     (HBM-bound)
// hist:   k_hist                                                                                  (vector-issue bound)
// tree:   k_tree + k_layout                                                                       (latency chains, chip mostly idle; the
//                                                                                                  small blocks are encoded under the dense trees)
// encode: k_encode                                                                                (vector-issue bound)
// d_planar: the source is a planar int32 matrix (rspt_hip_compress_planar_batch_dev) and src is not looked at
// ls: a ladder call -- the transform kernels take each block's quantiser from its ladder entry, not the handle's
static int phase_front(rspt_hip_packer* p, const uint8_t* src, size_t nblocks, hipStream_t st, const int32_t* d_planar = nullptr, const LadderSel* ls = nullptr) {
    const Geom& g = p->g;
    const uint32_t B = (uint32_t)nblocks;
    stamp(p, ST_PRE, st);
    const bool xd = g.kind == RSPT_HIP_KIND_XDELTA_HZR;
    if (int rc = front_begin(p, nblocks, st)) return rc;
    if (g.kind == RSPT_HIP_KIND_BYTES) {
        // the ingest kernel is the whole front end: planes, segment bits and nbuse[] (no escalation: nb_state stays 1)
        const uint64_t units = (uint64_t)nblocks * ((g.N + 4095u) >> 12);
        const uint64_t want = 8ull * (uint64_t)p->num_cu;  // eight 256-thread workgroups per CU
        hipLaunchKernelGGL(k_bytes_ingest, dim3((uint32_t)(units < want ? units : want)), dim3(kIngestThreads), 0, st, src, g, B, p->ws.planes, p->nzflag,
                           p->ws.nbuse, p->ws.plane_dirty, p->dirty_shift);
        HIPCHK(p, hipGetLastError());
        stamp(p, ST_NB, st);
        stamp(p, ST_HIST, st);
        const uint32_t nhb = (uint32_t)slots_of(p, nblocks) * kMaxPlanes * g.nblk;
        hipLaunchKernelGGL(k_histlist, dim3((nhb + 255) / 256), dim3(256), 0, st, p->nzflag, p->ws.nbuse, g, nhb, p->ws.big_list, p->work_ctr + 2, p->psel);
        HIPCHK(p, hipGetLastError());
        return RSPT_HIP_OK;
    }
    const uint32_t np = d_planar ? launch_front_planar(p, d_planar, nblocks, st)
                                 : by_bps(g.bps, [&](auto bps) { return launch_front<decltype(bps)::value>(p, src, nblocks, st); });
    launch_forward_transform(p, B, st, p->nzflag, ls);
    HIPCHK(p, hipGetLastError());

    stamp(p, ST_NB, st);
    if (g.kind != RSPT_HIP_KIND_XDELTA_HZR && g.kind != RSPT_HIP_KIND_HZR)  // (k_tile_planes runs the scan in its last workgroup)
        hipLaunchKernelGGL(k_nb_scan, dim3(1), dim3(1024), 0, st, p->needmask, B, p->nb_state, p->ws.nbuse, 0);
    if (xd && np < 4) {  // nb may have escalated in this call: add the planes the main pass did not write
        if (d_planar)
            launch_planar_stream<true>(p, d_planar, nblocks, np, 4 - np, p->ws.nbuse, st);
        else
            by_bps(g.bps, [&](auto bps) { launch_fixup<decltype(bps)::value>(p, src, nblocks, np, st); });
    }
    stamp(p, ST_HIST, st);
    // (the list of k_hist's blocks sits in big_list until k_layout refills that array for k_encode; its count in work_ctr[2])
    const uint32_t nhb = B * kMaxPlanes * g.nblk;
    hipLaunchKernelGGL(k_histlist, dim3((nhb + 255) / 256), dim3(256), 0, st, p->nzflag, p->ws.nbuse, g, nhb, p->ws.big_list, p->work_ctr + 2, p->psel);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

static uint32_t persistent_grid(const rspt_hip_packer* p, uint32_t nhb, uint32_t knob) {
    const uint32_t persist = (uint32_t)(2 * p->num_cu) < nhb ? (uint32_t)(2 * p->num_cu) : nhb;  // 2 x 1024 threads fill a CU
    return knob && knob < persist ? knob : persist;
}

static int phase_hist(rspt_hip_packer* p, uint32_t B, hipStream_t st) {
    const Geom& g = p->g;
    const uint32_t nhb = B * kMaxPlanes * g.nblk;
    hipLaunchKernelGGL(k_hist, dim3(persistent_grid(p, nhb, p->hist_grid)), dim3(kEncThreads), 0, st, p->ws.planes, g, p->nzflag, p->ws.hist, p->ws.seghist, p->work_ctr,
                       p->ws.big_list, p->work_ctr + 2, p->ws.lists, p->ws.listinfo);
    HIPCHK(p, hipGetLastError());  // (a failing launch is reported at its own stage)
    return RSPT_HIP_OK;
}

static int phase_tree(rspt_hip_packer* p, uint32_t B, hipStream_t st) {
    const Geom& g = p->g;
    const uint32_t nhb = B * kMaxPlanes * g.nblk;
    hipLaunchKernelGGL(k_tree, dim3((nhb + 3) / 4), dim3(256), 0, st, p->ws.hist, p->ws.planes, g, p->ws.nbuse, p->nzflag, nhb, p->ws.cw, p->ws.tdesc, p->ws.meta, p->ws.seghist, p->ws.segbase,
                       p->ws.zbuf[p->ws.zset ^ 1], (uint32_t)p->ws.zcap_words, p->crc, p->ws.staging, p->psel);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

static int phase_layout(rspt_hip_packer* p, uint32_t B, void* d_dst, size_t dst_stride, uint64_t* d_sizes, hipStream_t st) {
    const Geom& g = p->g;
    WorkQueues* wq = reinterpret_cast<WorkQueues*>(p->work_ctr + 4);
    // (B = block slots; a bare-stream handle's k_layout writes one stream and one size per plane of a slot)
    hipLaunchKernelGGL(k_layout, dim3(B), dim3(256), 0, st, g, p->ws.nbuse, p->ws.meta, p->ws.means, (uint8_t*)d_dst, (uint64_t)dst_stride, p->ws.out_off,
                       d_sizes, p->crc, p->nzflag, wq, p->ws.big_list, p->ws.plane_dirty, p->dirty_shift, p->psel);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

static int phase_encode(rspt_hip_packer* p, uint32_t B, void* d_dst, size_t dst_stride, hipStream_t st) {
    const Geom& g = p->g;
    const uint32_t nhb = B * kMaxPlanes * g.nblk;
    WorkQueues* wq = reinterpret_cast<WorkQueues*>(p->work_ctr + 4);
    hipLaunchKernelGGL(k_encode, dim3(persistent_grid(p, nhb, p->enc_grid)), dim3(kEncThreads), 0, st, p->ws.planes, g, p->nzflag, p->ws.meta, p->ws.cw, p->ws.tdesc, p->ws.out_off,
                       p->crc, (uint8_t*)d_dst, (uint64_t)dst_stride * (g.kind == RSPT_HIP_KIND_BYTES ? kMaxPlanes : 1), wq, p->ws.big_list, p->ws.segbase, p->ws.lists, p->ws.listinfo, p->stamps, p->ws.staging, nhb);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

// one batch, start to end on one stream
static int compress_batch_serial(rspt_hip_packer* p, const void* d_src, size_t nblocks, void* d_dst, size_t dst_stride, uint64_t* d_sizes, hipStream_t st,
                                 const int32_t* d_planar = nullptr, const LadderSel* ls = nullptr) {
    int rc = rspt_hip_reserve(p, nblocks);
    if (rc) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    const uint32_t B = (uint32_t)slots_of(p, nblocks);  // what the hzr kernels count in
    if ((rc = phase_front(p, (const uint8_t*)d_src, nblocks, st, d_planar, ls)) != 0) return rc;
    if ((rc = phase_hist(p, B, st)) != 0) return rc;

    stamp(p, ST_TREE, st);
    if (p->psel & 256u) {  // (diagnostic builds only: time the front end and k_hist alone)
        for (int i = ST_TREE + 1; i <= ST_COUNT; ++i) stamp(p, i, st);
        if (p->profiling) p->ev_valid = true;
        return RSPT_HIP_OK;
    }
    if ((rc = phase_tree(p, B, st)) != 0) return rc;
    const int zset_next = p->ws.zset ^ 1;

    stamp(p, ST_LAYOUT, st);
    if (p->psel & 512u) {  // (diagnostic builds only: stop behind k_tree)
        for (int i = ST_LAYOUT + 1; i <= ST_COUNT; ++i) stamp(p, i, st);
        if (p->profiling) p->ev_valid = true;
        p->ws.zero_ready[zset_next] = true;
        p->ws.zset = zset_next;
        return RSPT_HIP_OK;
    }
    // a choice outside the ladder: the block's transform has not run; k_layout is made to treat it as a stream that does not fit
    if (ls) hipLaunchKernelGGL(k_ladder_refuse, dim3(B), dim3(256), 0, st, ls->choice, ls->fwd.n, p->g, (const uint32_t*)p->ws.nbuse, p->ws.meta);
    if ((rc = phase_layout(p, B, d_dst, dst_stride, d_sizes, st)) != 0) return rc;

    stamp(p, ST_ENCODE, st);
    if ((rc = phase_encode(p, B, d_dst, dst_stride, st)) != 0) return rc;
    if (ls) hipLaunchKernelGGL(k_ladder_flag, dim3((B + 255) / 256), dim3(256), 0, st, ls->choice, ls->fwd.n, B, d_sizes, 0u);
    stamp(p, ST_COUNT, st);
    if (p->profiling) p->ev_valid = true;
    HIPCHK(p, hipGetLastError());
    p->ws.zero_ready[zset_next] = true;  // every launch went out: the other copy is zero when the next call starts
    p->ws.zset = zset_next;
    return RSPT_HIP_OK;
}

int rspt_hip_compress_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, void* d_dst, size_t dst_stride, uint64_t* d_sizes,
                                void* stream) {
    if (!p || !d_src || !d_dst || !d_sizes || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_src) & 15) return RSPT_HIP_ERR_ARG;  // tile loads are 16-byte aligned chunks
    if (p->feed) return RSPT_HIP_ERR_ARG;  // (the feed owns the handle's workspace until rspt_hip_feed_end)
    return compress_batch_serial(p, d_src, nblocks, d_dst, dst_stride, d_sizes, (hipStream_t)stream);
}

int rspt_hip_compress_batch_ladder_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder,
                                       const uint32_t* d_choice, void* d_dst, size_t dst_stride, uint64_t* d_sizes, void* stream) {
    if (!p || !d_src || !d_dst || !d_sizes || !d_choice || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_src) & 15) || (reinterpret_cast<uintptr_t>(d_choice) & 3)) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    LadderSel ls;
    if (int rc = make_ladder(p, ladder, nladder, d_choice, &ls)) return rc;
    // (k_ladder_refuse's payload lengths must exceed the stride: 2^32 per hzr block, where a stream has at most 65543 bytes of one)
    if ((unsigned long long)dst_stride >> 32 >= p->g.nblk) return RSPT_HIP_ERR_ARG;
    return compress_batch_serial(p, d_src, nblocks, d_dst, dst_stride, d_sizes, (hipStream_t)stream, nullptr, &ls);
}

int rspt_hip_compress_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, void* d_dst, size_t dst_stride, uint64_t* d_sizes,
                                       void* stream) {
    if (!p || !d_planar || !d_dst || !d_sizes || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(d_planar) & 3) return RSPT_HIP_ERR_ARG;
    if (p->g.kind == RSPT_HIP_KIND_BYTES) return RSPT_HIP_ERR_ARG;  // (a byte buffer has no samples)
    if (p->feed) return RSPT_HIP_ERR_ARG;  // (the feed owns the handle's workspace until rspt_hip_feed_end)
    return compress_batch_serial(p, nullptr, nblocks, d_dst, dst_stride, d_sizes, (hipStream_t)stream, d_planar);
}

int rspt_hip_compress_planar_batch_ladder_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                                              const uint32_t* d_choice, void* d_dst, size_t dst_stride, uint64_t* d_sizes, void* stream) {
    if (!p || !d_planar || !d_dst || !d_sizes || !d_choice || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_planar) & 3) || (reinterpret_cast<uintptr_t>(d_choice) & 3)) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    LadderSel ls;
    if (int rc = make_ladder(p, ladder, nladder, d_choice, &ls)) return rc;  // (every kind without samples or without a ladder: unsupported)
    if ((unsigned long long)dst_stride >> 32 >= p->g.nblk) return RSPT_HIP_ERR_ARG;  // (as rspt_hip_compress_batch_ladder_dev)
    return compress_batch_serial(p, nullptr, nblocks, d_dst, dst_stride, d_sizes, (hipStream_t)stream, d_planar, &ls);
}

size_t rspt_hip_pack_bound(const rspt_hip_packer* p, size_t nblocks) {
    if (!p) return 0;
    return 32 + 16 * nblocks + nblocks * ((rspt_hip_max_compressed_size(p) + 15) & ~(size_t)15);
}

int rspt_hip_pack_batch_dev(rspt_hip_packer* p, const void* d_dst, size_t dst_stride, const uint64_t* d_sizes, size_t nblocks, void* d_packed,
                            uint64_t* d_total, void* stream) {
    if (!p || !d_dst || !d_sizes || !d_packed || !d_total || nblocks == 0 || nblocks > 65535) return RSPT_HIP_ERR_ARG;
    if (nblocks > p->ws.cap_blocks) return RSPT_HIP_ERR_ARG;  // the per-stream nb comes from the handle's last compress call of >= nblocks blocks
    if ((reinterpret_cast<uintptr_t>(d_dst) & 15) || (dst_stride & 15) || (reinterpret_cast<uintptr_t>(d_packed) & 15)) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_pack_index, dim3(1), dim3(1024), 0, st, d_sizes, (uint32_t)nblocks, p->nb_state, p->ws.nbuse, (uint8_t*)d_packed, d_total,
                       p->g.kind == RSPT_HIP_KIND_BYTES ? 1u : 0u);
    hipLaunchKernelGGL(k_pack_copy, dim3(32, (unsigned)nblocks), dim3(256), 0, st, (const uint8_t*)d_dst, (uint64_t)dst_stride, (uint32_t)nblocks,
                       (uint8_t*)d_packed);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_pack_batch_choice_dev(rspt_hip_packer* p, const void* d_dst, size_t dst_stride, const uint64_t* d_sizes, size_t nblocks,
                                   const uint32_t* d_choice, size_t nladder, void* d_packed, uint64_t* d_total, void* stream) {
    if (!p || !d_dst || !d_sizes || !d_choice || !d_packed || !d_total || nblocks == 0 || nblocks > 65535) return RSPT_HIP_ERR_ARG;
    const Geom& g = p->g;
    if (g.kind != RSPT_HIP_KIND_HADAMARD && !(g.kind == RSPT_HIP_KIND_DCT && !p->dct_fft)) return RSPT_HIP_ERR_UNSUPPORTED;  // (make_ladder's kinds)
    if (nladder < 1 || nladder > kMaxLadder || (reinterpret_cast<uintptr_t>(d_choice) & 3)) return RSPT_HIP_ERR_ARG;
    if (nblocks > p->ws.cap_blocks) return RSPT_HIP_ERR_ARG;  // (as rspt_hip_pack_batch_dev)
    if ((reinterpret_cast<uintptr_t>(d_dst) & 15) || (dst_stride & 15) || (reinterpret_cast<uintptr_t>(d_packed) & 15)) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const uint32_t B = (uint32_t)nblocks;
    // k_pack_index and k_pack_copy as rspt_hip_pack_batch_dev launches them, between the two kernels of pack_choice.hip
    hipLaunchKernelGGL(k_pack_choice_sizes, dim3((B + 255) / 256), dim3(256), 0, st, d_sizes, d_choice, (uint32_t)nladder, B, (uint64_t*)p->ws.pack_sizes);
    hipLaunchKernelGGL(k_pack_index, dim3(1), dim3(1024), 0, st, (const uint64_t*)p->ws.pack_sizes, B, p->nb_state, p->ws.nbuse, (uint8_t*)d_packed, d_total, 0u);
    hipLaunchKernelGGL(k_pack_choice_bits, dim3((B + 255) / 256), dim3(256), 0, st, d_choice, B, (uint8_t*)d_packed);
    hipLaunchKernelGGL(k_pack_copy, dim3(32, (unsigned)nblocks), dim3(256), 0, st, (const uint8_t*)d_dst, (uint64_t)dst_stride, B, (uint8_t*)d_packed);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

void* rspt_hip_stream(rspt_hip_packer* p) { return p ? (void*)p->stream : nullptr; }

int rspt_hip_synchronize(rspt_hip_packer* p) {
    if (!p) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    HIPCHK(p, hipStreamSynchronize(p->stream));
    return RSPT_HIP_OK;
}

unsigned rspt_hip_current_nb(rspt_hip_packer* p) {
    if (!p) return 0;
    hipSetDevice(p->device);
    hipDeviceSynchronize();
    uint32_t nb = 0;
    if (hipMemcpy(&nb, p->nb_state, sizeof(nb), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (nb >= 1 && nb <= 4) p->nb_host = nb;
    return nb;
}

int rspt_hip_set_nb(rspt_hip_packer* p, unsigned nb) {
    if (!p || nb < 1 || nb > 4) return RSPT_HIP_ERR_ARG;
    if (p->g.kind != RSPT_HIP_KIND_XDELTA_HZR) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    HIPCHK(p, hipDeviceSynchronize());
    uint32_t v = nb;
    HIPCHK(p, hipMemcpy(p->nb_state, &v, sizeof(v), hipMemcpyHostToDevice));
    p->nb_host = nb;
    return RSPT_HIP_OK;
}

int rspt_hip_set_quantizer(rspt_hip_packer* p, double quality, unsigned nb) {
    if (!p || nb < 1 || nb > 4) return RSPT_HIP_ERR_ARG;
    if (p->g.kind != RSPT_HIP_KIND_DCT && p->g.kind != RSPT_HIP_KIND_HADAMARD) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;  // (groups in flight were launched with the setting they were pushed under)
    HIPCHK(p, hipSetDevice(p->device));
    HIPCHK(p, hipDeviceSynchronize());  // ordered like rspt_hip_set_nb: behind everything launched under the old setting
    if (!set_quality(p, quality, false)) return RSPT_HIP_ERR_ARG;
    uint32_t v = nb;
    HIPCHK(p, hipMemcpy(p->nb_state, &v, sizeof(v), hipMemcpyHostToDevice));  // (a failure leaves the handle as it was)
    set_quality(p, quality);
    // the staging of rspt_hip_compress_many / rspt_hip_decompress_many holds one stream per rspt_hip_max_compressed_size, which
    // follows nb: it is made again, for the new size, by the next of those calls (nothing of it is in flight behind the
    // synchronisation above)
    if (nb != p->nb_host) p->many = ManyStaging();
    p->nb_host = nb;
    return RSPT_HIP_OK;
}

int rspt_hip_get_quantizer(const rspt_hip_packer* p, double* quality, unsigned* nb) {
    if (!p || !quality || !nb) return RSPT_HIP_ERR_ARG;
    if (p->g.kind != RSPT_HIP_KIND_DCT && p->g.kind != RSPT_HIP_KIND_HADAMARD) return RSPT_HIP_ERR_ARG;
    *quality = p->quality;
    *nb = p->nb_host;
    return RSPT_HIP_OK;
}

int rspt_hip_set_byte_order(rspt_hip_packer* p, int big_endian) {
    if (!p) return RSPT_HIP_ERR_ARG;
    p->big_endian = big_endian ? 1 : 0;
    p->g.be = p->big_endian && p->g.bps > 1 ? 1u : 0u;  // compress: every front end reverses the bytes of a sample as it reads it (no extra pass)
    return RSPT_HIP_OK;
}

void* rspt_hip_host_alloc(size_t bytes) {
    void* q = nullptr;
    if (bytes == 0 || hipHostMalloc(&q, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return q;
}

void rspt_hip_host_free(void* q) {
    if (q) hipHostFree(q);
}

int rspt_hip_set_verify(rspt_hip_packer* p, int on) {
    if (!p) return RSPT_HIP_ERR_ARG;
    p->verify = on ? 1 : 0;
    return RSPT_HIP_OK;
}

static int ensure_host_staging(rspt_hip_packer* p) {
    if (p->stage.src) return RSPT_HIP_OK;
    HostStaging s;
    // The stream buffer serves both directions.  What compress writes fits rspt_hip_max_compressed_size; what decompress is
    // given may be longer: a Huffman block of another writer can have up to 65536 bytes of payload whatever it decodes to
    // (hzr_decode takes it: tests/test_hzr_foreign.py, the full tree over a 16-byte block), so every block counts in full.
    const size_t hzr_longest = 4 + (size_t)p->g.nblk * (7 + (size_t)kHzrBlock);
    const size_t longest = p->g.kind == RSPT_HIP_KIND_BYTES ? hzr_longest : 1 + p->g.hdr_len + (size_t)kMaxPlanes * (4 + hzr_longest);
    s.dst_cap = std::max(rspt_hip_max_compressed_size(p), longest) + 64;
    if (hipMalloc(s.src.out(), p->g.block_bytes + 64) != hipSuccess || hipMalloc(s.dst.out(), s.dst_cap) != hipSuccess ||
        hipMalloc(s.size.out(), sizeof(uint64_t)) != hipSuccess)
        return RSPT_HIP_ERR_ALLOC;
    hipMemset(s.src, 0, p->g.block_bytes + 64);
    hipDeviceSynchronize();  // the memset runs on the null stream; our copies use a non-blocking stream
    p->stage = std::move(s);
    return RSPT_HIP_OK;
}

// Page-locked host memory (rspt_hip_host_alloc, hipHostMalloc, hipHostRegister) is visible to the device: returns its device
// address, or nullptr for pageable memory (which has to be staged).
static void* device_view_of_host(const void* host_ptr) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, host_ptr) != hipSuccess) {
        (void)hipGetLastError();  // (pageable memory: not an error of ours)
        return nullptr;
    }
    if (a.type != hipMemoryTypeHost || !a.devicePointer) return nullptr;
    return a.devicePointer;
}

int rspt_hip_compress(rspt_hip_packer* p, const void* src_host, void* dst_host, size_t dst_max_len, size_t* dst_len) {
    if (!p || !src_host || !dst_host || !dst_len) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    int rc = ensure_host_staging(p);
    if (rc) return rc;
    // With page-locked buffers neither copy is a phase of its own: the front end reads the samples across the link as it
    // transforms them, the encoders write the stream straight into the caller's buffer -- one synchronisation at the end.
    // Pageable buffers go through the device staging copies as before.
    uint8_t* d_dst = dst_max_len >= 64 ? (uint8_t*)device_view_of_host(dst_host) : nullptr;
    // A page-locked, 16-byte aligned source is read in place by the front end (the upload IS the front end, at ~44 GB/s of 4-byte
    // loads across the link: 0.513 ms per 16 MiB block against 0.551 with a copy phase; measured and dropped: the upload cut
    // into four sample ranges on the copy stream with a front-end launch behind each range's event -- 0.627 ms, every
    // cross-stream dependency costs 25-60 us on this runtime).
    const uint8_t* d_src = (const uint8_t*)device_view_of_host(src_host);
    if (d_src && (reinterpret_cast<uintptr_t>(d_src) & 15)) d_src = nullptr;  // (tile loads are 16-byte aligned chunks)
    if (!d_src) {
        HIPCHK(p, hipMemcpyAsync(p->stage.src, src_host, p->g.block_bytes, hipMemcpyHostToDevice, p->stream));
        d_src = p->stage.src;
    }
    rc = compress_batch_serial(p, d_src, 1, d_dst ? d_dst : p->stage.dst, d_dst ? dst_max_len : p->stage.dst_cap, p->stage.size, p->stream);
    if (rc) return rc;
    uint64_t sz = 0;
    uint32_t nb_now = 0;
    HIPCHK(p, hipMemcpyAsync(&sz, p->stage.size, sizeof(sz), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(p, hipMemcpyAsync(&nb_now, p->nb_state, sizeof(nb_now), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(p, hipStreamSynchronize(p->stream));
    if (nb_now >= 1 && nb_now <= 4) p->nb_host = nb_now;  // the next call writes exactly the planes it needs
    if (sz >> 63) {  // did not fit the space the kernels were given (nothing written): the size it needs is in the low bits
        *dst_len = (size_t)(sz & ~(1ull << 63));
        return RSPT_HIP_ERR_DST_TOO_SMALL;
    }
    if (sz > dst_max_len) {
        *dst_len = (size_t)sz;
        return RSPT_HIP_ERR_DST_TOO_SMALL;
    }
    if (!d_dst) {
        HIPCHK(p, hipMemcpyAsync(dst_host, p->stage.dst, (size_t)sz, hipMemcpyDeviceToHost, p->stream));
        HIPCHK(p, hipStreamSynchronize(p->stream));
    }
    *dst_len = (size_t)sz;
    return RSPT_HIP_OK;
}

// The decoder behind k_dec_block: the planes of B blocks (ws.planes, dec_nb[b] of them each) -> planar values -> the inverse
// transform of the lossy packers.  inv_out, inv_sx: where the lossless packers' last inverse pass writes, and its sign extension
// (the lossy packers' goes to ws.planar, for their transform).  Returns where a lossy packer's planar result lies.
static const int32_t* launch_inverse(rspt_hip_packer* p, uint32_t B, hipStream_t st, int32_t* inv_out, uint32_t inv_sx, const LadderSel* ls) {
    const Geom& g = p->g;
    const bool xd = g.kind == RSPT_HIP_KIND_XDELTA_HZR || g.kind == RSPT_HIP_KIND_DCT;
    const dim3 tg(p->ntile, B);
    if (xd) {
        hipLaunchKernelGGL((k_inv_tile<0, true>), tg, dim3(256), 0, st, p->ws.planes, g, p->ws.dec_nb, p->ntile, p->ws.txor, p->ws.tsum, p->ws.planar, 0u);
        hipLaunchKernelGGL((k_inv_scan_tiles<true>), dim3(B), dim3(1024), 0, st, p->ws.txor, p->ntile);
        hipLaunchKernelGGL((k_inv_tile<1, true>), tg, dim3(256), 0, st, p->ws.planes, g, p->ws.dec_nb, p->ntile, p->ws.txor, p->ws.tsum, p->ws.planar, 0u);
        hipLaunchKernelGGL((k_inv_scan_tiles<false>), dim3(B), dim3(1024), 0, st, p->ws.tsum, p->ntile);
        hipLaunchKernelGGL((k_inv_tile<2, true>), tg, dim3(256), 0, st, p->ws.planes, g, p->ws.dec_nb, p->ntile, p->ws.txor, p->ws.tsum, inv_out, inv_sx);
    } else {
        hipLaunchKernelGGL((k_inv_tile<2, false>), tg, dim3(256), 0, st, p->ws.planes, g, p->ws.dec_nb, p->ntile, p->ws.txor, p->ws.tsum, inv_out, inv_sx);
    }
    const int32_t* final_planar = p->ws.planar;
    if (g.kind == RSPT_HIP_KIND_HADAMARD) {
        const uint32_t fw_lds = (g.ns > 32768u ? 32768u : g.ns) * 4u;
        if (g.ns > 65536u) {
            launch_fwht_big<false>(p, B, st, ls ? &ls->inv : nullptr, ls ? ls->choice : nullptr);
        } else if (g.ns == 65536u && ls) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht64k_l<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
            hipLaunchKernelGGL((k_fwht64k_l<false, false>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, (uint8_t*)nullptr,
                               (uint32_t*)nullptr, 0u, ls->inv, ls->choice);
        } else if (ls) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht_l<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
            hipLaunchKernelGGL((k_fwht_l<false>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, ls->inv, ls->choice);
        } else if (g.ns == 65536u && p->had_quant) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht64k_q<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
            hipLaunchKernelGGL((k_fwht64k_q<false, false>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, (uint8_t*)nullptr,
                               (uint32_t*)nullptr, 0u, p->had_div_inv);
        } else if (g.ns == 65536u) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht64k<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
            hipLaunchKernelGGL((k_fwht64k<false, false>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, (uint8_t*)nullptr,
                               (uint32_t*)nullptr, 0u);
        } else if (p->had_quant) {
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht_q<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
            hipLaunchKernelGGL((k_fwht_q<false>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, p->had_div_inv);
        } else {
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
            hipLaunchKernelGGL((k_fwht<false>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means);
        }
    } else if (g.kind == RSPT_HIP_KIND_DCT) {
        if (p->dct_fft)
            launch_dct_fft<false>(p, B, p->ws.planar, p->ws.planar2, st);
        else if (ls)
            hipLaunchKernelGGL((k_dct_l<false>), dim3((g.ns + 255) / 256, (g.nch + kDctCh - 1) / kDctCh, B), dim3(256), 0, st, p->ws.planar, g,
                               p->ws.means, p->cos_tab_t, ls->inv, ls->choice, p->dct_cs0, p->ws.planar2);
        else
            hipLaunchKernelGGL((k_dct<false>), dim3((g.ns + 255) / 256, (g.nch + kDctCh - 1) / kDctCh, B), dim3(256), 0, st, p->ws.planar, g,
                               p->ws.means, p->cos_tab_t, 0.0, p->idct_scale, p->dct_cs0, p->ws.planar2);
        final_planar = p->ws.planar2;
    }
    return final_planar;
}

// to_planar: d_dst is the caller's planar int32 matrix (rspt_hip_decompress_planar_batch_dev), not the native batch
static int decompress_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, const uint64_t* pidx, size_t packed_len, size_t nblocks,
                          void* d_dst, uint64_t* d_consumed, void* stream, bool to_planar = false, const LadderSel* ls = nullptr);

int rspt_hip_decompress_batch_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, size_t nblocks, void* d_dst, uint64_t* d_consumed,
                                  void* stream) {
    return decompress_dev(p, d_src, src_stride, nullptr, 0, nblocks, d_dst, d_consumed, stream);
}

int rspt_hip_decompress_batch_ladder_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, size_t nblocks, const double* ladder, size_t nladder,
                                         const uint32_t* d_choice, void* d_dst, uint64_t* d_consumed, void* stream) {
    if (!p || !d_src || !d_dst || !d_consumed || !d_choice || nblocks == 0 || (reinterpret_cast<uintptr_t>(d_choice) & 3)) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    LadderSel ls;
    if (int rc = make_ladder(p, ladder, nladder, d_choice, &ls)) return rc;
    return decompress_dev(p, d_src, src_stride, nullptr, 0, nblocks, d_dst, d_consumed, stream, false, &ls);
}

int rspt_hip_decompress_packed_dev(rspt_hip_packer* p, const void* d_packed, size_t packed_len, size_t nblocks, void* d_dst, uint64_t* d_consumed,
                                   void* stream) {
    if (!d_packed || (reinterpret_cast<uintptr_t>(d_packed) & 15)) return RSPT_HIP_ERR_ARG;
    // header + index must be there before the device reads them (compared without a product that could wrap for a huge nblocks)
    if (nblocks == 0 || nblocks > 65535) return RSPT_HIP_ERR_ARG;
    if (packed_len < 32 || nblocks > (packed_len - 32) / 16) return RSPT_HIP_ERR_CORRUPT;
    const uint8_t* base = (const uint8_t*)d_packed;
    // header 32 bytes, index 16 bytes per stream, then the payload the offsets are relative to
    return decompress_dev(p, base + 32 + 16 * nblocks, 0, reinterpret_cast<const uint64_t*>(base + 32), packed_len, nblocks, d_dst, d_consumed,
                          stream);
}

// what both planar decompress entries refuse in front of decompress_dev's own checks
static bool planar_out_refused(const rspt_hip_packer* p, const int32_t* d_planar) {
    return !p || !d_planar || (reinterpret_cast<uintptr_t>(d_planar) & 3) || p->g.kind == RSPT_HIP_KIND_BYTES;
}

int rspt_hip_decompress_planar_batch_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, size_t nblocks, int32_t* d_planar,
                                         uint64_t* d_consumed, void* stream) {
    if (planar_out_refused(p, d_planar)) return RSPT_HIP_ERR_ARG;
    return decompress_dev(p, d_src, src_stride, nullptr, 0, nblocks, d_planar, d_consumed, stream, true);
}

int rspt_hip_decompress_packed_planar_dev(rspt_hip_packer* p, const void* d_packed, size_t packed_len, size_t nblocks, int32_t* d_planar,
                                          uint64_t* d_consumed, void* stream) {
    if (planar_out_refused(p, d_planar)) return RSPT_HIP_ERR_ARG;
    if (!d_packed || (reinterpret_cast<uintptr_t>(d_packed) & 15)) return RSPT_HIP_ERR_ARG;
    if (nblocks == 0 || nblocks > 65535) return RSPT_HIP_ERR_ARG;
    if (packed_len < 32 || nblocks > (packed_len - 32) / 16) return RSPT_HIP_ERR_CORRUPT;
    const uint8_t* base = (const uint8_t*)d_packed;
    return decompress_dev(p, base + 32 + 16 * nblocks, 0, reinterpret_cast<const uint64_t*>(base + 32), packed_len, nblocks, d_planar, d_consumed,
                          stream, true);
}

int rspt_hip_decompress_planar_batch_ladder_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, size_t nblocks, const double* ladder,
                                                size_t nladder, const uint32_t* d_choice, int32_t* d_planar, uint64_t* d_consumed, void* stream) {
    if (!p || !d_src || !d_planar || !d_consumed || !d_choice || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d_planar) & 3) || (reinterpret_cast<uintptr_t>(d_choice) & 3)) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    LadderSel ls;
    if (int rc = make_ladder(p, ladder, nladder, d_choice, &ls)) return rc;
    return decompress_dev(p, d_src, src_stride, nullptr, 0, nblocks, d_planar, d_consumed, stream, true, &ls);
}

// Both packed ladder decoders: the container checks of rspt_hip_decompress_packed_dev, the choices of the index into the handle's
// array (k_index_choices; the workspace is made first, so that decompress_dev's own rspt_hip_reserve leaves the array where it
// is), and the decoder with that array as the ladder call's choice.
static int decompress_packed_ladder(rspt_hip_packer* p, const void* d_packed, size_t packed_len, size_t nblocks, const double* ladder, size_t nladder,
                                    void* d_dst, uint64_t* d_consumed, void* stream, bool to_planar) {
    if (!p || !d_dst || !d_consumed || !d_packed || (reinterpret_cast<uintptr_t>(d_packed) & 15)) return RSPT_HIP_ERR_ARG;
    if (to_planar && (reinterpret_cast<uintptr_t>(d_dst) & 3)) return RSPT_HIP_ERR_ARG;
    if (nblocks == 0 || nblocks > 65535) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;
    LadderSel ls;
    if (int rc = make_ladder(p, ladder, nladder, nullptr, &ls)) return rc;
    // header + index must be there before the device reads them (rspt_hip_decompress_packed_dev)
    if (packed_len < 32 || nblocks > (packed_len - 32) / 16) return RSPT_HIP_ERR_CORRUPT;
    if (int rc = rspt_hip_reserve(p, nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    const uint8_t* base = (const uint8_t*)d_packed;
    const uint64_t* index = reinterpret_cast<const uint64_t*>(base + 32);
    hipLaunchKernelGGL(k_index_choices, dim3(((uint32_t)nblocks + 255) / 256), dim3(256), 0, (hipStream_t)stream, index, (uint32_t)nblocks,
                       (uint32_t*)p->ws.idx_choice);
    HIPCHK(p, hipGetLastError());
    ls.choice = p->ws.idx_choice;
    return decompress_dev(p, base + 32 + 16 * nblocks, 0, index, packed_len, nblocks, d_dst, d_consumed, stream, to_planar, &ls);
}

int rspt_hip_decompress_packed_ladder_dev(rspt_hip_packer* p, const void* d_packed, size_t packed_len, size_t nblocks, const double* ladder,
                                          size_t nladder, void* d_dst, uint64_t* d_consumed, void* stream) {
    return decompress_packed_ladder(p, d_packed, packed_len, nblocks, ladder, nladder, d_dst, d_consumed, stream, false);
}

int rspt_hip_decompress_packed_planar_ladder_dev(rspt_hip_packer* p, const void* d_packed, size_t packed_len, size_t nblocks, const double* ladder,
                                                 size_t nladder, int32_t* d_planar, uint64_t* d_consumed, void* stream) {
    return decompress_packed_ladder(p, d_packed, packed_len, nblocks, ladder, nladder, d_planar, d_consumed, stream, true);
}

static int decompress_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, const uint64_t* pidx, size_t packed_len, size_t nblocks,
                          void* d_dst, uint64_t* d_consumed, void* stream, bool to_planar, const LadderSel* ls) {
    if (!p || !d_src || !d_dst || !d_consumed || nblocks == 0) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;  // (the feed owns the plane workspace until rspt_hip_feed_end)
    int rc = rspt_hip_reserve(p, nblocks);
    if (rc) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    p->ws.planes_unknown = true;  // the decoded planes land in the compressor's plane workspace
    hipStream_t st = (hipStream_t)stream;
    {
        const Geom& g = p->g;
        const uint32_t B = (uint32_t)nblocks;
        const uint8_t* src = (const uint8_t*)d_src;
        HIPCHK(p, hipMemsetAsync(d_consumed, 0, nblocks * sizeof(uint64_t), st));
        const bool bare = g.kind == RSPT_HIP_KIND_BYTES;  // one thread and one flat plane per stream
        hipLaunchKernelGGL(k_dec_frame, dim3(((bare ? B : B * kMaxPlanes) + 63) / 64), dim3(64), 0, st, src, (uint64_t)src_stride, B, g, p->nb_state, p->ws.blk_off,
                           d_consumed, p->ws.means, pidx, p->nb_state + 2, (uint64_t)packed_len, p->ws.dec_nb);
        {
            // persistent: block costs differ 10x (dense plane 0 against light planes) and the dispatcher places workgroup i
            // on XCD i % 8 in order, so a plain grid ran its second half at a quarter of the slots (tools/census_decode.py)
            // (k_dec_block takes the blocks plane-fastest: dense and light ones in turns)
            const uint32_t total = bare ? g.nblk * B : g.nblk * B * kMaxPlanes;
            const uint32_t want = 2u * (uint32_t)p->num_cu;  // two 1024-thread workgroups (76 KiB of LDS each) per CU
            hipLaunchKernelGGL(k_dec_block, dim3(want < total ? want : total), dim3(kDecThreads), 0, st, src, (uint64_t)src_stride, g, p->ws.dec_nb, p->ws.blk_off,
                               p->ws.planes, d_consumed, p->ablate ? p->stamps : nullptr, p->verify ? p->crc : nullptr, pidx, p->nb_state + 2, total);
        }
        if (bare) {  // the planes are the output: out to the caller's buffers, whatever their alignment
            const uint64_t units = (uint64_t)B * ((g.N + 15u) >> 4);
            const uint64_t wgs = (units + 255) / 256, want = 16ull * (uint64_t)p->num_cu;
            hipLaunchKernelGGL(k_bytes_emit, dim3((uint32_t)(wgs < want ? wgs : want)), dim3(256), 0, st, p->ws.planes, g, B, (uint8_t*)d_dst);
            HIPCHK(p, hipGetLastError());
            return RSPT_HIP_OK;
        }
        const bool xd = g.kind == RSPT_HIP_KIND_XDELTA_HZR || g.kind == RSPT_HIP_KIND_DCT;
        // int32 samples of the two hzr packers: the last inverse pass writes the interleaved block itself (k_inv_native)
        const bool lossless = g.kind == RSPT_HIP_KIND_XDELTA_HZR || g.kind == RSPT_HIP_KIND_HZR;
        const bool direct = lossless && !to_planar && g.bps == 4 && (g.nch & 3) == 0 && g.ns % kRowTile == 0 && (reinterpret_cast<uintptr_t>(d_dst) & 15) == 0;
        // planar out, lossless packers: the last inverse pass writes the caller's matrix itself, sign-extended from the sample width
        int32_t* inv_out = lossless && to_planar ? (int32_t*)d_dst : (int32_t*)p->ws.planar;
        const uint32_t inv_sx = lossless && to_planar ? 32u - 8u * g.bps : 0u;
        if (direct) {
            const uint32_t nrow = g.N / kRowTile;
            const dim3 rg((g.N / 16 + 255) / 256, B);
            if (xd) {
                hipLaunchKernelGGL(k_inv_rows, rg, dim3(256), 0, st, p->ws.planes, g, p->ws.dec_nb, nrow, p->ws.rowrec);
                hipLaunchKernelGGL(k_inv_scan_rows, dim3(B), dim3(1024), 0, st, p->ws.rowrec, nrow, p->ws.txor, p->ws.tsum);
            }
            if (g.nch <= 16) {
                if (xd)
                    launch_inv_native<true, 16>(p, B, nrow, d_dst, st);
                else
                    launch_inv_native<false, 16>(p, B, nrow, d_dst, st);
            } else {
                if (xd)
                    launch_inv_native<true, 64>(p, B, nrow, d_dst, st);
                else
                    launch_inv_native<false, 64>(p, B, nrow, d_dst, st);
            }
            // (big-endian samples: k_inv_native reverses each sample as it writes it -- g.be)
            HIPCHK(p, hipGetLastError());
            return RSPT_HIP_OK;
        }
        const int32_t* final_planar = launch_inverse(p, B, st, inv_out, inv_sx, ls);
        if (to_planar) {
            if (!lossless) {  // the transform packers: the inverse transform's output, cut to the sample width as the native back ends cut it
                const uint64_t wgs = ((uint64_t)B * g.N + 255) / 256, want = 16ull * (uint64_t)p->num_cu;
                if (ls) {  // a ladder call: the elements of a block whose choice lies outside the ladder are passed over, and its flag
                    hipLaunchKernelGGL(k_planar_emit_l, dim3((uint32_t)(wgs < want ? wgs : want)), dim3(256), 0, st, final_planar, g, B, (int32_t*)d_dst,
                                       ls->choice, ls->inv.n);
                    hipLaunchKernelGGL(k_ladder_flag, dim3((B + 255) / 256), dim3(256), 0, st, ls->choice, ls->inv.n, B, d_consumed, 1u);
                } else {
                    hipLaunchKernelGGL(k_planar_emit, dim3((uint32_t)(wgs < want ? wgs : want)), dim3(256), 0, st, final_planar, g, B, (int32_t*)d_dst);
                }
            }
            HIPCHK(p, hipGetLastError());
            return RSPT_HIP_OK;
        }
        const uint32_t T = min(p->Tn_native, g.ns);
        const uint32_t lds = g.nch * (T + 1) * 4;
        const dim3 ng(T ? (g.ns + T - 1) / T : 0u, B);
        if (ls) {  // a ladder call: the 64 x 64 tiles that pass over a block whose choice lies outside the ladder, and its flag
            by_bps(g.bps, [&](auto bps) {
                hipLaunchKernelGGL(k_wide_native_l<decltype(bps)::value>, dim3((g.ns + 63) / 64, (g.nch + 63) / 64, B), dim3(256), 0, st, final_planar, g,
                                   (uint8_t*)d_dst, ls->choice, ls->inv.n);
            });
            hipLaunchKernelGGL(k_ladder_flag, dim3((B + 255) / 256), dim3(256), 0, st, ls->choice, ls->inv.n, B, d_consumed, 1u);
        } else if (T == 0) {  // more channels than k_planar_native holds a row of: 64 x 64 tiles
            by_bps(g.bps, [&](auto bps) { launch_wide_native<decltype(bps)::value>(g, final_planar, (uint8_t*)d_dst, B, st); });
        } else if (g.bps == 4 && (g.nch & 3) == 0 && (g.ns & 3) == 0 && g.nch <= 1024 && (reinterpret_cast<uintptr_t>(d_dst) & 15) == 0) {
            const uint32_t T4 = tile_i32x4(g);
            hipLaunchKernelGGL(k_planar_native_i32x4, dim3((g.ns + T4 - 1) / T4, B), dim3(256), g.nch * (T4 + 1) * 4, st, final_planar, g, T4,
                               (uint8_t*)d_dst);
        } else {
            by_bps(g.bps, [&](auto bps) {
                hipLaunchKernelGGL((k_planar_native<decltype(bps)::value>), ng, dim3(256), lds, st, final_planar, g, T, (uint8_t*)d_dst);
            });
        }
        // (big-endian samples: the kernels above reverse each sample as they write it -- g.be)
    }
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

// src_cap: bytes readable at src_host (SIZE_MAX: the reference's contract -- the stream says how long it is)
static int decompress_host(rspt_hip_packer* p, const void* src_host, size_t src_cap, size_t* src_len, void* dst_host) {
    if (!p || !src_host || !src_len || !dst_host) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    int rc = ensure_host_staging(p);
    if (rc) return rc;
    // The stream length is not an input (signal_packer.h:50-57): walk the chunk
    // lengths on the host to find it -- framing only, no decoding.
    const uint8_t* s = (const uint8_t*)src_host;
    const unsigned nb = p->g.kind == RSPT_HIP_KIND_BYTES ? 0u : rspt_hip_current_nb(p);
    size_t pos = 1 + p->g.hdr_len;
    if (p->g.kind == RSPT_HIP_KIND_BYTES) {  // a bare stream has no length word: master header, then nblk block headers
        if (src_cap < 4) return RSPT_HIP_ERR_CORRUPT;
        pos = 4;
        for (uint32_t j = 0; j < p->g.nblk; ++j) {
            if (src_cap - pos < 7) return RSPT_HIP_ERR_CORRUPT;
            pos += 7 + ((size_t)s[pos] | ((size_t)s[pos + 1] << 8)) + 1;
            if (pos > p->stage.dst_cap || pos > src_cap) return RSPT_HIP_ERR_CORRUPT;
        }
    }
    for (unsigned k = 0; k < nb; ++k) {
        if (pos > src_cap || src_cap - pos < 4) return RSPT_HIP_ERR_CORRUPT;  // (never a read past what the caller vouched for)
        uint32_t len;
        memcpy(&len, s + pos, 4);
        pos += 4 + (size_t)len;
        if (pos > p->stage.dst_cap || pos > src_cap) return RSPT_HIP_ERR_CORRUPT;
    }
    HIPCHK(p, hipMemcpyAsync(p->stage.dst, src_host, pos, hipMemcpyHostToDevice, p->stream));
    // a page-locked destination takes the samples straight from the inverse's last kernel (the download is that kernel's
    // stores, across the link): one synchronisation, no copy phase of its own
    uint8_t* d_out = (uint8_t*)device_view_of_host(dst_host);
    if (d_out && (reinterpret_cast<uintptr_t>(d_out) & 15)) d_out = nullptr;
    rc = rspt_hip_decompress_batch_dev(p, p->stage.dst, p->stage.dst_cap, 1, d_out ? d_out : p->stage.src, p->stage.size, (void*)p->stream);
    if (rc) return rc;
    uint64_t used = 0;
    HIPCHK(p, hipMemcpyAsync(&used, p->stage.size, sizeof(used), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(p, hipStreamSynchronize(p->stream));
    if (used >> 63) return RSPT_HIP_ERR_CORRUPT;
    if (!d_out) {
        HIPCHK(p, hipMemcpyAsync(dst_host, p->stage.src, p->g.block_bytes, hipMemcpyDeviceToHost, p->stream));
        HIPCHK(p, hipStreamSynchronize(p->stream));
    }
    *src_len = (size_t)used;
    return RSPT_HIP_OK;
}

int rspt_hip_hzr_verify_batch_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, const uint64_t* d_src_len, size_t nblocks,
                                  uint64_t* d_decoded, void* stream) {
    if (!p || !d_src || !d_src_len || !d_decoded || nblocks == 0 || nblocks > 0xFFFFFFFFu) return RSPT_HIP_ERR_ARG;
    if (p->g.kind != RSPT_HIP_KIND_BYTES) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    const uint64_t want = 2ull * (uint64_t)p->num_cu;  // a 1024-thread workgroup per stream, two to a CU
    hipLaunchKernelGGL(k_hzr_verify, dim3((uint32_t)(nblocks < want ? nblocks : want)), dim3(kVerThreads), 0, (hipStream_t)stream, (const uint8_t*)d_src,
                       (uint64_t)src_stride, d_src_len, (uint32_t)nblocks, p->crc, d_decoded);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_decompress(rspt_hip_packer* p, const void* src_host, size_t* src_len, void* dst_host) {
    return decompress_host(p, src_host, (size_t)-1, src_len, dst_host);
}

int rspt_hip_decompress_bounded(rspt_hip_packer* p, const void* src_host, size_t src_cap, size_t* src_len, void* dst_host) {
    return decompress_host(p, src_host, src_cap, src_len, dst_host);
}

long long rspt_hip_debug_read(rspt_hip_packer* p, int which, void* host_buf, size_t cap) {
    if (!p || !host_buf || p->ws.cap_blocks == 0) return RSPT_HIP_ERR_ARG;
    if (hipSetDevice(p->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return RSPT_HIP_ERR_LAUNCH;
    const Geom& g = p->g;
    const size_t nhb = p->ws.cap_slots * kMaxPlanes * g.nblk;
    const void* src = nullptr;
    size_t n = 0;
    switch (which) {
        case 0: src = p->ws.planes; n = p->ws.cap_slots * kMaxPlanes * g.plane_stride; break;
        case 1: src = p->ws.planar; n = p->ws.cap_blocks * (size_t)g.N * 4; break;
        case 2: src = p->ws.planar2; n = p->ws.planar2 ? p->ws.cap_blocks * (size_t)g.N * 4 : 0; break;
        case 3: src = p->ws.hist; n = nhb * kSymStride * 4; break;
        case 4: src = p->ws.meta; n = nhb * sizeof(BlockMeta); break;
        case 5: src = p->ws.nbuse; n = p->ws.cap_blocks * 4; break;
        case 6: src = p->ws.means; n = p->ws.cap_blocks * (size_t)g.hdr_len; break;
        case 8: src = p->nzflag; n = nhb * 4; break;
        case 7: src = p->stamps; n = (512 * 16 * 8 + 2 * 16384) * sizeof(unsigned long long); break;
        default: return RSPT_HIP_ERR_ARG;
    }
    if (!src || n == 0) return 0;
    if (n > cap) n = cap;
    if (hipMemcpy(host_buf, src, n, hipMemcpyDeviceToHost) != hipSuccess) return RSPT_HIP_ERR_LAUNCH;
    return (long long)n;
}

int rspt_hip_set_profiling(rspt_hip_packer* p, int on) {
    if (!p) return RSPT_HIP_ERR_ARG;
    p->profiling = on != 0;
    p->ev_valid = false;
    return RSPT_HIP_OK;
}

int rspt_hip_stage_count(const rspt_hip_packer*) { return ST_COUNT; }
const char* rspt_hip_stage_name(const rspt_hip_packer*, int i) { return (i >= 0 && i < ST_COUNT) ? kStageNames[i] : ""; }

int rspt_hip_stage_times(rspt_hip_packer* p, float* ms, int n) {
    if (!p || !ms || !p->ev_valid) return RSPT_HIP_ERR_ARG;
    HIPCHK(p, hipSetDevice(p->device));
    HIPCHK(p, hipEventSynchronize(p->ev[ST_COUNT]));
    for (int i = 0; i < n && i < ST_COUNT; ++i) {
        float t = 0;
        HIPCHK(p, hipEventElapsedTime(&t, p->ev[i], p->ev[i + 1]));
        ms[i] = t;
    }
    return RSPT_HIP_OK;
}

#include "host_pipeline.hip"
#include "host_gather.hip"

}  // extern "C"

#include "host_stages.hip"  // (templates: outside the block; rspt_hip.h declares every entry extern "C")
#include "host_rate.hip"
#include "host_target.hip"
#include "host_budget.hip"
#include "host_total.hip"
