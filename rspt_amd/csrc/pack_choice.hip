// pack_choice.hip -- the per-block choice of a ladder or target compress in the container index (rspt_hip_pack_batch_choice_dev,
// rspt_hip_decompress_packed_ladder_dev, rspt_hip_decompress_packed_planar_ladder_dev).
//
// The index length word is length | choice << 60 | nb << 56 | invalid << 63 (hzr_kernels.hip: k_pack_index).  Bits 60..62 are zero
// in what k_pack_index writes and masked away by every reader (k_pack_copy, k_dec_frame), so the kernels here stand around the
// existing ones, which stay what they are:
//   k_pack_choice_sizes  in front of k_pack_index: the sizes it reads, with bit 63 set on a block whose choice lies outside the
//                        ladder although its stream was written -- an empty flagged entry, not a choice that aliases another
//   k_pack_choice_bits   behind k_pack_index: the choice into bits 60..62 of every entry that is not flagged
//   k_index_choices      in front of the decoder: the choices of a container's index as the uint32 array the ladder kernels read;
//                        a flagged entry becomes a choice outside every ladder, so that nothing is written for its block
#include "common.hpp"

namespace rspt {

constexpr uint32_t kPackChoiceShift = 60;  // (kMaxLadder == 8: three bits)
static_assert(kMaxLadder <= 8, "a choice has three bits in the index length word");

__global__ __launch_bounds__(256) void k_pack_choice_sizes(const uint64_t* __restrict__ sizes, const uint32_t* __restrict__ choice, uint32_t n,
                                                          uint32_t nblocks, uint64_t* __restrict__ out) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nblocks) return;
    const uint64_t sz = sizes[b];
    out[b] = !(sz >> 63) && choice[b] >= n ? 1ull << 63 : sz;
}

__global__ __launch_bounds__(256) void k_pack_choice_bits(const uint32_t* __restrict__ choice, uint32_t nblocks, uint8_t* __restrict__ packed) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nblocks) return;
    uint64_t* index = reinterpret_cast<uint64_t*>(packed) + 4;
    const uint64_t w = index[2 * b + 1];
    if (!(w >> 63)) index[2 * b + 1] = w | (uint64_t)(choice[b] & 7u) << kPackChoiceShift;  // (choice[b] < n <= 8: k_pack_choice_sizes)
}

__global__ __launch_bounds__(256) void k_index_choices(const uint64_t* __restrict__ index, uint32_t nblocks, uint32_t* __restrict__ choice) {
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b >= nblocks) return;
    const uint64_t w = index[2 * b + 1];
    choice[b] = w >> 63 ? 0xFFFFFFFFu : (uint32_t)(w >> kPackChoiceShift) & 7u;
}

}  // namespace rspt
