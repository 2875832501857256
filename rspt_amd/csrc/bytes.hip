// bytes.hip -- the raw byte-buffer codec (RSPT_HIP_KIND_BYTES): libhzr's hzr_encode / hzr_decode / hzr_verify on the GPU.
//
//   k_bytes_ingest   compress front end: nbuf caller buffers (any byte alignment) -> one workspace plane each, under the
//                    clean-block invariant (rspt_hip_packer::plane_dirty), with the nzflag segment bits and nbuse[] the hzr
//                    kernels go by.  From k_histlist on the encoder runs unchanged; k_layout frames bare streams.
//   k_bytes_emit     decompress back end: decoded planes -> the caller's buffers (any byte alignment)
//   k_hzr_verify     hzr_verify (hzr_decode.c:569-624) of device-resident streams: frame walk, mode bytes, CRC-32C of every
//                    block's payload -- no decoding, no output bytes
//
// Buffer i of a call lives in flat plane i of the workspace: plane (i & 3) of block slot (i >> 2).
#include "common.hpp"

namespace rspt {

constexpr uint32_t kIngestThreads = 256;  // x 16 bytes: one 4 KiB segment (one nzflag bit) per workgroup step

// the 16-byte aligned unit at `al`, never a byte at or past `end`
__device__ __forceinline__ uint4 ld_unit_bounded(const uint8_t* al, const uint8_t* end) {
    if (al >= end) return make_uint4(0, 0, 0, 0);
    if (al + 16 <= end) return *reinterpret_cast<const uint4*>(al);
    const uint32_t n = (uint32_t)(end - al);
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t i = 0; i < 16; ++i)
        if (i < n) w[i >> 2] |= (uint32_t)al[i] << ((i & 3u) * 8u);
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// Persistent streaming copy.  A workgroup step is one 4 KiB segment of one buffer, a lane one 16-byte unit of the plane (the
// plane is 16-byte aligned, the buffer at `src + b * N` is not unless N is a multiple of 16): the source comes in as the 16-byte
// ALIGNED units around it -- a lane's second unit is its neighbour's first, so it crosses lanes instead of being loaded twice --
// and is shifted into place by the buffer's misalignment, which is uniform over the workgroup.  Stores follow the streaming
// sample front end (preprocess.hip: k_tile_stream): a clean hzr block takes only the 128-byte lines that hold a non-zero byte
// (eight aligned lanes), a dirty one every line of the buffer, the bytes between N and the end of its last line as zeros.
__global__ __launch_bounds__(kIngestThreads) void k_bytes_ingest(const uint8_t* __restrict__ src, Geom g, uint32_t nbuf, uint8_t* __restrict__ planes,
                                                                uint32_t* __restrict__ nzflag, uint32_t* __restrict__ nbuse,
                                                                const uint32_t* __restrict__ plane_dirty, uint32_t dirty_shift) {
    const uint32_t tid = threadIdx.x, l = lane_id();
    // planes in use per block slot: four buffers to a slot, the last slot as many as are left (there is no escalation)
    const uint32_t nslot = (nbuf + 3u) >> 2;
    for (uint32_t s = blockIdx.x * kIngestThreads + tid; s < nslot; s += gridDim.x * kIngestThreads) nbuse[s] = min(4u, nbuf - 4u * s);
    const uint32_t segs = (g.N + 4095u) >> 12;
    const uint64_t total = (uint64_t)nbuf * segs;
    const uint8_t* end = src + (size_t)nbuf * g.N;  // of the batch: what lies between a buffer's end and a unit's is masked below
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {
        const uint32_t b = (uint32_t)(w / segs), seg = (uint32_t)(w - (uint64_t)b * segs);
        const uint32_t off = (seg << 12) + tid * 16u;  // (N < 2^31)
        const uintptr_t a0 = reinterpret_cast<uintptr_t>(src) + (size_t)b * g.N + off;
        const uint32_t sh = (uint32_t)(a0 & 15u);  // workgroup-uniform
        const uint8_t* al = reinterpret_cast<const uint8_t*>(a0 - sh);  // (>= src: the batch base is 16-byte aligned)
        const uint4 lo = ld_unit_bounded(al, end);
        uint32_t o[4] = {lo.x, lo.y, lo.z, lo.w};
        if (sh) {
            uint4 hi;
            hi.x = (uint32_t)__shfl_down((int)lo.x, 1, 64);
            hi.y = (uint32_t)__shfl_down((int)lo.y, 1, 64);
            hi.z = (uint32_t)__shfl_down((int)lo.z, 1, 64);
            hi.w = (uint32_t)__shfl_down((int)lo.w, 1, 64);
            if (l == 63u) hi = ld_unit_bounded(al + 16, end);
            const uint32_t d[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            const uint32_t q = sh >> 2, r = sh & 3u;
            uint32_t e[5];
#pragma unroll
            for (uint32_t i = 0; i < 5; ++i) e[i] = q == 0 ? d[i] : q == 1 ? d[i + 1] : q == 2 ? d[i + 2] : d[i + 3];
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) o[i] = __builtin_amdgcn_alignbyte(e[i + 1], e[i], r);
        }
        const uint32_t nv = off < g.N ? min(16u, g.N - off) : 0u;  // bytes of the buffer in this unit
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) o[i] = nv >= 4u * i + 4u ? o[i] : nv <= 4u * i ? 0u : (o[i] & ((1u << ((nv - 4u * i) * 8u)) - 1u));
        const unsigned long long bal = __ballot((o[0] | o[1] | o[2] | o[3]) != 0u);
        const bool line_nz = ((bal >> (l & ~7u)) & 0xFFull) != 0ull;
        const uint32_t j = off >> 16;
        if ((off & ~127u) < g.N) {  // the line holds a byte of the buffer (it ends inside the plane: plane_stride = N rounded up to 256)
            const uint32_t bucket = j >> dirty_shift;
            const bool dirty = ((plane_dirty[(size_t)b * 4u + (bucket >> 5)] >> (bucket & 31u)) & 1u) != 0u;
            if (line_nz || dirty) *reinterpret_cast<uint4*>(planes + (size_t)b * g.plane_stride + off) = make_uint4(o[0], o[1], o[2], o[3]);
        }
        if (bal && l == (uint32_t)__builtin_ctzll(bal)) atomicOr(&nzflag[(size_t)b * g.nblk + j], 1u << (seg & 15u));
    }
}

// decoded planes -> caller buffers: aligned 16-byte loads, unaligned 16-byte stores (the hardware takes them), the last unit of
// a buffer byte by byte
__global__ __launch_bounds__(256) void k_bytes_emit(const uint8_t* __restrict__ planes, Geom g, uint32_t nbuf, uint8_t* __restrict__ dst) {
    const uint32_t units = (g.N + 15u) >> 4;
    const uint64_t total = (uint64_t)nbuf * units;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t b = (uint32_t)(i / units), u = (uint32_t)(i - (uint64_t)b * units);
        const uint4 v = *reinterpret_cast<const uint4*>(planes + (size_t)b * g.plane_stride + (size_t)u * 16u);
        uint8_t* dp = dst + (size_t)b * g.N + (size_t)u * 16u;
        const uint32_t nbytes = min(16u, g.N - u * 16u);
        if (nbytes == 16u) {
            __builtin_memcpy(dp, &v, 16);
        } else {
            const uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t q = 0; q < 16; ++q)
                if (q < nbytes) dp[q] = (uint8_t)(x[q >> 2] >> ((q & 3u) * 8u));
        }
    }
}

// ---------------------------------------------------------------------------
// k_hzr_verify: one 1024-thread workgroup per stream walks its blocks in order (every header is read by all threads: the walk
// is workgroup-uniform); the payload CRC is the decoder's word-strided one (decode.hip: dec_block), read from global memory.
// Nothing at or beyond s + len is read: a header is read once its 7 bytes are known to lie inside, a payload once its last does.
// ---------------------------------------------------------------------------
constexpr uint32_t kVerThreads = 1024;

__device__ __forceinline__ uint32_t payload_crc32c(const uint8_t* __restrict__ pb, uint32_t L, const CrcConsts* __restrict__ cc, uint32_t* s_wsum) {
    const uint32_t tid = threadIdx.x, l = tid & 63u, w = tid >> 6;
    const uint32_t nvw = (L + 3u) >> 2;
    const uint32_t Kst = (nvw + kVerThreads - 1) / kVerThreads;
    auto vword = [&](uint32_t r) -> uint32_t {  // payload bytes [L - 4(r+1), L - 4r), zero in front
        const int32_t lo = (int32_t)L - 4 * (int32_t)(r + 1);
        uint32_t v = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) v |= (lo + q >= 0 ? (uint32_t)pb[lo + q] : 0u) << (8 * q);
        return v;
    };
    uint32_t c = 0;
    if (tid < nvw) {
        for (uint32_t kk = Kst - 1; kk >= 1; --kk) {
            const uint32_t r = tid + kVerThreads * kk;
            if (r < nvw) c ^= vword(r);
            c = gf_shift(cc, 78, c);  // * x^(8*4096)
        }
        c ^= vword(tid);
        c = gf_shift4(cc, l, c);  // to the end of the wave's 64 words
    }
    c = wave_xor_u32(c);
    __syncthreads();  // (s_wsum of the block before has been read)
    if (l == 0) s_wsum[w] = gf_shift(cc, 63u - 4u * w, c);  // * x^(8*256*w): to the end of the payload
    __syncthreads();
    uint32_t raw = 0;
    for (uint32_t i = 0; i < kVerThreads / 64; ++i) raw ^= s_wsum[i];
    // the initial state 0xFFFFFFFF travels through L bytes: 4096 a + 64 b + 4 c4 + dbytes
    uint32_t init = 0xFFFFFFFFu;
    const uint32_t a = L >> 12, bq = (L >> 6) & 63u, c4 = (L >> 2) & 15u, dbytes = L & 3u;
    if (a) init = gf_shift(cc, a == 16 ? 80u : 64u + (15u - a), init);  // x^(8*4096*a); a = 16 only for L = 65536
    if (bq) init = gf_shift(cc, 63u - bq, init);                         // x^(8*64*bq)
    if (c4) init = gf_shift4(cc, c4 - 1u, init);                         // x^(8*4*c4)
    for (uint32_t q = 0; q < dbytes; ++q) init = cc->table[0][init & 0xFFu] ^ (init >> 8);
    return ~(raw ^ init);  // (every thread has it)
}

__global__ __launch_bounds__(kVerThreads) void k_hzr_verify(const uint8_t* __restrict__ src, uint64_t src_stride, const uint64_t* __restrict__ src_len,
                                                           uint32_t nstreams, const CrcConsts* __restrict__ cc, uint64_t* __restrict__ decoded) {
    __shared__ uint32_t s_wsum[kVerThreads / 64];
    for (uint32_t b = blockIdx.x; b < nstreams; b += gridDim.x) {
        const uint8_t* s = src + (size_t)b * src_stride;
        const uint64_t len = src_len[b];
        uint64_t size = 0;
        bool bad = len < 4;  // the master header (hzr_decode.c:581-585)
        if (!bad) {
            size = ld_le32(s);
            uint64_t left = size, pos = 4;
            while (left > 0) {
                if (pos + 7 > len) {  // the block header (:593-599)
                    bad = true;
                    break;
                }
                const uint32_t L = ld_le16(s + pos) + 1u, want = ld_le32(s + pos + 2), mode = s[pos + 6];
                if (mode > 2u || pos + 7 + L > len) {  // (:600-603), and the payload inside the stream (:614-618)
                    bad = true;
                    break;
                }
                if (payload_crc32c(s + pos + 7, L, cc, s_wsum) != want) {  // (:606-611)
                    bad = true;
                    break;
                }
                pos += 7ull + L;
                left -= left < kHzrBlock ? left : (uint64_t)kHzrBlock;
            }
        }
        if (threadIdx.x == 0) decoded[b] = size | (bad ? kBadBit : 0ull);
    }
}

}  // namespace rspt
