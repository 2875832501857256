// convert.hip -- the wide inverse converter: planar int32 [nch][ns] -> interleaved native samples for any channel count.
//
//   k_wide_native   the mirror image of preprocess.hip: k_wide_planar.  k_planar_native (decode.hip) keeps one row of ALL channels
//                   in LDS and so ends at 8192 channels; this kernel takes a 64 x 64 tile (channels x samples) per workgroup and
//                   has no such limit.  It is the last kernel of decompress where k_planar_native cannot run, and the kernel of
//                   rspt_hip_i32_to_native_batch_dev for everything but the common int32 shape of a narrow handle and handles
//                   of fewer than 32 channels (rspt_hip.hip).
//
// A workgroup's three steps, a barrier between them:
//   1. channel rows of the planar block -> tile[c][t] (rows of 65 words).  16-byte loads where the planar rows are 16-byte
//      aligned (ns % 4 == 0 and an aligned buffer), else one dword per lane, consecutive lanes on consecutive samples.
//   2. lane <-> (sample t, four channels): the four words come out of the tile transposed -- bank (4 c4 + k + t) mod 64, all
//      64 lanes apart -- get their bytes reversed for a big-endian handle (one v_perm_b32 per sample) and are packed into BPS
//      whole dwords of the output row rows[t], which is the tile's piece of sample row s0 + t as it will lie in memory.
//   3. the rows go out.  Where every row of the tile starts and ends on a 16-byte boundary: 16-byte stores.  Otherwise whole
//      aligned dwords -- a row's piece may start at any byte, so the dword comes from two LDS words through v_alignbyte_b32 --
//      and single bytes only in the first and last dword of a row.
// No division by a run-time value anywhere (the row length of step 3 is a compile-time constant).
#include "common.hpp"

namespace rspt {

template <int BPS>
__global__ __launch_bounds__(256) void k_wide_native(const int32_t* __restrict__ planar, Geom g, uint8_t* __restrict__ dst) {
#include "k_wide_native_body.hpp"
}
template __global__ void k_wide_native<1>(const int32_t*, Geom, uint8_t*);
template __global__ void k_wide_native<2>(const int32_t*, Geom, uint8_t*);
template __global__ void k_wide_native<3>(const int32_t*, Geom, uint8_t*);
template __global__ void k_wide_native<4>(const int32_t*, Geom, uint8_t*);

// k_wide_native_l: the back end of rspt_hip_decompress_batch_ladder_dev -- a block whose choice lies outside the ladder of n
// entries is not written (the inverse transform has left it alone, k_fwht_l)
template <int BPS>
__global__ __launch_bounds__(256) void k_wide_native_l(const int32_t* __restrict__ planar, Geom g, uint8_t* __restrict__ dst,
                                                      const uint32_t* __restrict__ choice, uint32_t n) {
    if (choice[blockIdx.z] >= n) return;
#include "k_wide_native_body.hpp"
}
template __global__ void k_wide_native_l<1>(const int32_t*, Geom, uint8_t*, const uint32_t*, uint32_t);
template __global__ void k_wide_native_l<2>(const int32_t*, Geom, uint8_t*, const uint32_t*, uint32_t);
template __global__ void k_wide_native_l<3>(const int32_t*, Geom, uint8_t*, const uint32_t*, uint32_t);
template __global__ void k_wide_native_l<4>(const int32_t*, Geom, uint8_t*, const uint32_t*, uint32_t);

// what the ladder entries do for a block whose choice lies outside the ladder, one workgroup per block:
//   k_ladder_refuse  (compress, between k_tree and k_layout) every hzr block of it is given a payload length that no dst_stride
//                    holds, so that k_layout writes nothing for the block and tells k_encode to leave it alone
//   k_ladder_flag    (behind the last kernel) bit 63 of sizes[b]: compress sets the word to it, decompress adds it
__global__ __launch_bounds__(256) void k_ladder_refuse(const uint32_t* __restrict__ choice, uint32_t n, Geom g, const uint32_t* __restrict__ nbuse,
                                                      BlockMeta* __restrict__ meta) {
    const uint32_t b = blockIdx.x;
    if (choice[b] < n) return;
    const uint32_t hb0 = hb_index(g, b, 0, 0);
    for (uint32_t q = threadIdx.x; q < nbuse[b] * g.nblk; q += 256u) meta[hb0 + q].payload_len = 0xFFFFFFFFu;
}

__global__ __launch_bounds__(256) void k_ladder_flag(const uint32_t* __restrict__ choice, uint32_t n, uint32_t nblocks, uint64_t* __restrict__ sizes,
                                                    uint32_t keep) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b < nblocks && choice[b] >= n) sizes[b] = (keep ? sizes[b] : 0ull) | (1ull << 63);
}

}  // namespace rspt
