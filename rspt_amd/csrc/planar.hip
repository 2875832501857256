// planar.hip -- planar int32 [nblocks][nch][ns] in and out of the packers, without the pass through the native block
// (rspt_hip_compress_planar_batch_dev / rspt_hip_decompress_planar_batch_dev).
//
//   k_planar_stream  compress front end of the two hzr packers over a planar source: the flat [nch][ns] order IS the order the
//                    xdelta transform and the byte planes are defined on, so nothing is transposed -- a lane takes 16 consecutive
//                    elements, cuts them to the sample width and leaves one 16-byte unit per plane, under the clean-block
//                    invariant (rspt_hip_packer::plane_dirty), with the nzflag segment bits, the escalation magnitudes and the
//                    escalation scan of the native front end (preprocess.hip: k_tile_stream)
//   k_planar_ingest  compress front end of the transform packers: caller's matrix -> ws.planar, cut to the sample width (the
//                    transforms work in place there; the caller's buffer is only read), with the dct's channel sums
//   k_planar_emit    decompress back end of the transform packers: inverse transform's output -> caller's matrix, cut
//   k_planar_emit_l  the same behind a ladder call: the blocks whose choice lies outside the ladder are passed over
// The lossless packers decode straight into the caller's matrix: k_inv_tile<2, *> (decode.hip) with its sign-extension shift.
#include "common.hpp"

namespace rspt {

constexpr uint32_t kPlanarThreads = 256;  // x 16 elements: one 4 KiB segment of every plane (one nzflag bit) per workgroup step

// the low bps bytes of a value, sign-extended (sx = 32 - 8 * bps): what convert_i32_to_native keeps and convert_native_to_i32 reads back
__device__ __forceinline__ uint32_t cut_to_width(uint32_t v, uint32_t sx) { return (uint32_t)((int32_t)(v << sx) >> sx); }

// Persistent.  A workgroup takes a run of consecutive 4 KiB segments of the batch's (block, segment) list, a lane 16 consecutive
// elements of the block's flat array: 64 bytes in (four 16-byte loads, which need the 4-byte alignment of an int32 only), one
// 16-byte unit per plane out.  XDELTA: v[i] = (p[i]-p[i-1]-128) ^ (p[i-1]-p[i-2]-128) in flat order, from zeros in front of
// flat index 0 -- p[i-1], p[i-2] of a lane's first element are its neighbour's last two (DPP), for lane 0 of a wave two more
// dwords.  Planes [kfirst, kfirst + kcount) are written: all-zero 128-byte lines (eight aligned lanes) of a clean hzr block
// are left out, a dirty block takes every line of the array, its last unit padded with zeros.  The main pass (nbuse == nullptr)
// also sets the non-zero map of all four planes, folds the magnitudes into needmask[b] and runs the escalation scan in the
// last workgroup; the fix-up pass (nbuse != nullptr, launched blind) adds the planes above kfirst for the blocks whose nb
// grew past it in this call.
template <bool XDELTA>
__global__ __launch_bounds__(kPlanarThreads) void k_planar_stream(const int32_t* __restrict__ src, Geom g, uint32_t kfirst, uint32_t kcount,
                                                                 uint8_t* __restrict__ planes, uint32_t* __restrict__ needmask,
                                                                 uint32_t* __restrict__ nzflag, const uint32_t* __restrict__ nbuse, uint32_t nblocks,
                                                                 uint32_t* __restrict__ ticket, uint32_t* __restrict__ nb_state,
                                                                 uint32_t* __restrict__ nbuse_out, const uint32_t* __restrict__ plane_dirty,
                                                                 uint32_t dirty_shift) {
    const uint32_t tid = threadIdx.x, l = lane_id();
    const bool fixup = nbuse != nullptr;
    if (fixup && *nb_state <= kfirst) return;  // (nb did not grow past the planes the main pass wrote: see k_tile_stream)
    const uint32_t sx = 32u - 8u * g.bps;
    const uint32_t segs = (g.N + 4095u) >> 12;
    const uint64_t total = (uint64_t)nblocks * segs;
    const uint64_t per = (total + gridDim.x - 1) / gridDim.x;
    const uint64_t w0 = (uint64_t)blockIdx.x * per, w1 = w0 + per < total ? w0 + per : total;
    uint32_t sent_b = 0xFFFFFFFFu, sent_f = 0;  // the escalation bits this wave has already sent for block sent_b
    for (uint64_t w = w0; w < w1; ++w) {
        const uint32_t b = (uint32_t)(w / segs), seg = (uint32_t)(w - (uint64_t)b * segs);
        if (fixup && nbuse[b] <= kfirst) continue;  // (workgroup-uniform)
        const uint32_t off = (seg << 12) + tid * 16u;  // (N < 2^31)
        const uint32_t cnt = off < g.N ? min(16u, g.N - off) : 0u;
        const int32_t* pb = src + (size_t)b * g.N;
        uint32_t x[16];
        if (cnt == 16u) {
            uint4 q4[4];
            __builtin_memcpy(q4, pb + off, 64);
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                x[4 * q] = q4[q].x;
                x[4 * q + 1] = q4[q].y;
                x[4 * q + 2] = q4[q].z;
                x[4 * q + 3] = q4[q].w;
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 16; ++e) x[e] = e < cnt ? (uint32_t)pb[off + e] : 0u;
        }
#pragma unroll
        for (uint32_t e = 0; e < 16; ++e) x[e] = cut_to_width(x[e], sx);
        uint32_t v[16];
        uint32_t mag = 0;
        if (XDELTA) {
            // (a lane with elements has a full lane in front of it: only a block's last lanes are short)
            uint32_t p1 = dpp<0x138>(0u, x[15]), p2 = dpp<0x138>(0u, x[14]);  // wave_shr:1
            if (l == 0) {
                p1 = cnt && off >= 1u ? cut_to_width((uint32_t)pb[off - 1], sx) : 0u;
                p2 = cnt && off >= 2u ? cut_to_width((uint32_t)pb[off - 2], sx) : 0u;
            }
            uint32_t oprev = off ? p1 - p2 - 128u : 0u;  // flat index 0: delta_encode and xor_encode_32 start from 0
#pragma unroll
            for (uint32_t e = 0; e < 16; ++e) {
                const uint32_t o = x[e] - p1 - 128u;
                const uint32_t t = o ^ oprev;
                oprev = o;
                p1 = x[e];
                v[e] = e < cnt ? t : 0u;  // (elements past cnt are never stored or flagged)
                mag |= (uint32_t)((int32_t)cut_to_width(v[e], sx) ^ ((int32_t)cut_to_width(v[e], sx) >> 31));
            }
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 16; ++e) v[e] = x[e];
        }
        // byte-plane split of four values at a time: the 4 x 4 byte transpose of transform_item (preprocess.hip)
        uint32_t pw[4][4];
#pragma unroll
        for (uint32_t g4 = 0; g4 < 4; ++g4) {
            const uint32_t a0 = v[4 * g4], a1 = v[4 * g4 + 1], a2 = v[4 * g4 + 2], a3 = v[4 * g4 + 3];
            const uint32_t lo01 = __builtin_amdgcn_perm(a1, a0, 0x05010400u), hi01 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
            const uint32_t lo23 = __builtin_amdgcn_perm(a3, a2, 0x05010400u), hi23 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
            pw[0][g4] = __builtin_amdgcn_perm(lo23, lo01, 0x05040100u);
            pw[1][g4] = __builtin_amdgcn_perm(lo23, lo01, 0x07060302u);
            pw[2][g4] = __builtin_amdgcn_perm(hi23, hi01, 0x05040100u);
            pw[3][g4] = __builtin_amdgcn_perm(hi23, hi01, 0x07060302u);
        }
        const uint32_t j = off >> 16, bucket = j >> dirty_shift;  // (a segment lies in one hzr block: workgroup-uniform)
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const unsigned long long bal = __ballot((pw[k][0] | pw[k][1] | pw[k][2] | pw[k][3]) != 0u);
            if (k >= kfirst && k < kfirst + kcount) {
                const bool line_nz = ((bal >> (l & ~7u)) & 0xFFull) != 0ull;
                const bool dirty = ((plane_dirty[((size_t)b * kMaxPlanes + k) * 4u + (bucket >> 5)] >> (bucket & 31u)) & 1u) != 0u;
                if (cnt && (line_nz || dirty))  // (a short last unit ends inside the plane: plane_stride = N rounded up to 256)
                    *reinterpret_cast<uint4*>(planes + ((size_t)b * kMaxPlanes + k) * g.plane_stride + off) = make_uint4(pw[k][0], pw[k][1], pw[k][2], pw[k][3]);
            }
            if (!fixup && bal && l == (uint32_t)__builtin_ctzll(bal)) atomicOr(&nzflag[hb_index(g, b, k, j)], 1u << (seg & 15u));
        }
        if (XDELTA && !fixup) {  // only the three thresholds matter (need_from_mask); a wave sends each of them once per block
            mag = wave_or_u32(mag);
            const uint32_t f = (mag >= 0x80u ? 0x80u : 0u) | (mag >= 0x8000u ? 0x8000u : 0u) | (mag >= 0x800000u ? 0x800000u : 0u);
            if (b != sent_b) {
                sent_b = b;
                sent_f = 0;
            }
            if ((f & ~sent_f) && l == 0) atomicOr(&needmask[b], f);
            sent_f |= f;
        }
    }
    // main pass: the last workgroup to get here runs the escalation scan over the blocks (as k_tile_stream does)
    if (ticket) {
        __shared__ uint32_t s_last, s_wmax[16];
        __syncthreads();
        if (tid == 0) {
            __threadfence();  // this workgroup's needmask atomics are out
            s_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
        }
        __syncthreads();
        if (s_last) {
            __threadfence();
            nb_scan_body(needmask, nblocks, nb_state, nbuse_out, XDELTA ? 1 : 0, s_wmax);
        }
    }
}
template __global__ void k_planar_stream<true>(const int32_t*, Geom, uint32_t, uint32_t, uint8_t*, uint32_t*, uint32_t*, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*, const uint32_t*, uint32_t);
template __global__ void k_planar_stream<false>(const int32_t*, Geom, uint32_t, uint32_t, uint8_t*, uint32_t*, uint32_t*, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*, const uint32_t*, uint32_t);

// caller's matrix -> ws.planar, every value cut to the sample width.  A workgroup takes up to 4096 samples of one channel row;
// row_sum (optional): [block][channel] int64 sums of the cut samples, one atomic per wave (the dct's channel means without a
// second pass over the block, as k_tile_planar_i32x4 leaves them)
__global__ __launch_bounds__(256) void k_planar_ingest(const int32_t* __restrict__ src, Geom g, int32_t* __restrict__ planar,
                                                      long long* __restrict__ row_sum) {
    const uint32_t c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    const uint32_t sx = 32u - 8u * g.bps;
    const size_t base = (size_t)b * g.N + (size_t)c * g.ns;
    const uint32_t t0 = blockIdx.x * 4096u, t1 = min(g.ns, t0 + 4096u);
    long long sm = 0;
    for (uint32_t t = t0 + tid; t < t1; t += 256u) {
        const int32_t v = (int32_t)cut_to_width((uint32_t)src[base + t], sx);
        planar[base + t] = v;
        sm += v;
    }
    if (row_sum) {
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) sm += __shfl_xor(sm, d);
        if (lane_id() == 0) atomicAdd(reinterpret_cast<unsigned long long*>(row_sum + (size_t)b * g.nch + c), (unsigned long long)sm);
    }
}

// inverse transform's output -> caller's matrix, every value cut to the sample width (what the native back ends keep of it)
__global__ __launch_bounds__(256) void k_planar_emit(const int32_t* __restrict__ planar, Geom g, uint32_t nblocks, int32_t* __restrict__ dst) {
    constexpr bool kLadder = false;
    constexpr const uint32_t* choice = nullptr;
    constexpr uint32_t n = 0;
#include "k_planar_emit_body.hpp"
}

// k_planar_emit_l: the back end of rspt_hip_decompress_planar_batch_ladder_dev -- no element of a block whose choice lies outside
// the ladder of n entries is written
__global__ __launch_bounds__(256) void k_planar_emit_l(const int32_t* __restrict__ planar, Geom g, uint32_t nblocks, int32_t* __restrict__ dst,
                                                      const uint32_t* __restrict__ choice, uint32_t n) {
    constexpr bool kLadder = true;
#include "k_planar_emit_body.hpp"
}

}  // namespace rspt
