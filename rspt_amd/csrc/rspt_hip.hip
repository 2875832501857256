// rspt_hip.cpp -- C ABI (include/rspt_hip.h) over the gfx950 kernels.
//
// One handle = one reference packer instance: it owns the device workspace
// (what enc_/serialized_ are in signal_packer_base.h:20-21), one HIP stream and
// the persistent nr_bytes_to_compress_ state (signal_packer_xdelta_hzr.cpp:39,66),
// which lives in device memory so that batches chain without a host round trip.
// There is no CPU path: every entry point fails loudly if the device is missing.
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
#include "fir.hip"
#include "median.hip"
#include "peak.hip"
#include "quality.hip"
#include "convert.hip"
#include "bytes.hip"

using namespace rspt;

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

enum Stage { ST_PRE = 0, ST_NB, ST_HIST, ST_TREE, ST_LAYOUT, ST_ENCODE, ST_COUNT };
const char* kStageNames[ST_COUNT] = {"preprocess", "nb_scan", "hzr_hist", "hzr_tree", "layout", "hzr_encode"};

}  // namespace

// ---- owners of HIP resources: move-only, each releases what it holds when destroyed or reset, and nothing when empty ----
template <class T, auto Release>
class Owned {
  public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = o.h_;
            o.h_ = nullptr;
        }
        return *this;
    }
    ~Owned() { reset(); }
    void reset() {
        if (h_) Release(h_);
        h_ = nullptr;
    }
    T* out() {  // for the HIP call that creates the resource
        reset();
        return &h_;
    }
    operator T() const { return h_; }

  private:
    T h_ = nullptr;
};
template <class T> using Dev = Owned<T*, hipFree>;          // device memory
template <class T> using Pinned = Owned<T*, hipHostFree>;   // page-locked host memory
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

// Everything rspt_hip_reserve() sizes; replacing it releases the old workspace as a whole.
struct Workspace {
    size_t cap_blocks = 0;
    size_t cap_slots = 0;     // block slots of four planes each: cap_blocks, or a quarter of it for a bare-stream handle (one plane per buffer)
    Dev<uint8_t> planes;      // [slots][4][plane_stride]
    Dev<int32_t> planar;      // [cap][N] (transform packers, decode)
    Dev<uint32_t> nbuse;      // [cap]
    Dev<uint32_t> dec_nb;     // [cap] decode: planes of each stream (container index entry, else nb_state)
    Dev<uint32_t> big_list;   // [cap*4*nblk] hzr blocks for the workgroup-per-block encoder (filled by k_layout)
    Dev<uint32_t> staging;    // [cap*4*nblk][kStageSlotWords] header + payload of the small hzr blocks (k_tree -> k_encode), 3088 bytes each
    // The per-call zero region [nzflag | needmask | work counters | row sums] exists twice: while a call works in one copy its
    // k_tree zeroes the other for the next call (one store per thread) -- the memset in front of every call was a 9 us launch.
    Dev<uint32_t> zbuf[2];
    size_t zcap_words = 0;
    bool zero_ready[2] = {false, false};  // the copy is known to be all zero
    int zset = 0;                          // the copy the next call works in
    // Clean-block invariant (k_tile_stream's skipped stores): between calls, hzr block j of plane k of block slot b holds
    // zeros everywhere unless its bit in plane_dirty is set (128 bits per plane, bit = j >> dirty_shift).  The streaming
    // front end writes only the 128-byte lines that hold a non-zero byte into a clean block; k_layout sets the bits of
    // the blocks in which data stays behind, and the encoders wipe the non-zero granules of all others right after
    // reading them (light blocks only: block_is_wiped).
    Dev<uint32_t> plane_dirty;  // [cap*4][4]
    bool planes_unknown = false;  // something else (decompress, a diagnostic run) wrote the planes: flag them all
    Dev<uint32_t> hist;      // [cap*4*nblk][264]
    Dev<uint32_t> seghist;   // [cap*4*nblk][16][264] u16: tokens ending in each 4 KiB segment (k_hist -> k_tree)
    Dev<uint32_t> segbase;   // [cap*4*nblk][16] stream bit at which each segment's tokens start (k_tree -> k_encode)
    Dev<uint32_t> lists;     // [cap*4*nblk][16][kListCap] (position << 9 | value) entries of the sparse segments (k_hist -> k_encode)
    Dev<uint2> listinfo;     // [cap*4*nblk][16] {entries or kListNone, position behind the last literal before the segment}
    Dev<uint32_t> cw;        // [cap*4*nblk][264] code | length << 24 per symbol
    Dev<uint32_t> tdesc;     // [..][92]
    Dev<BlockMeta> meta;     // [..]
    Dev<uint64_t> out_off;   // [..]
    Dev<uint8_t> means;      // [cap][hdr_len]
    Dev<int32_t> planar2;    // [cap][N] second int32 buffer (dct output / idct output)
    Dev<uint32_t> txor;      // [cap][ntile] decode scans
    Dev<uint32_t> tsum;      // [cap][ntile]
    Dev<uint32_t> rowrec;    // [cap][N / 256][kRowRec] row tile records of the int32 decode path (k_inv_rows)
    Dev<uint64_t> blk_off;   // [cap*4*nblk] decode: hzr block offsets inside each stream
    Dev<double2> fft_scratch;  // [fft_bpp][nch][n] (dct beyond the dense table)
    size_t fft_bpp = 0;        // blocks per pass (bounds the scratch to ~1 GiB)
    Dev<int32_t> mean_i32;     // [cap][nch]
    // rspt_hip_prdn_batch_dev: [cap][nch] int64 channel sums | [cap][4] per-block accumulators | [cap] u32 flags, each part placed
    // per call right behind the one before it (the first two are zeroed by one memset in front of the call's kernels)
    Dev<unsigned long long> quality;
};

// rspt_hip_compress / rspt_hip_decompress: one block staged on the device
struct HostStaging {
    Dev<uint8_t> src;
    Dev<uint8_t> dst;
    Dev<uint64_t> size;
    size_t dst_cap = 0;
};

// One group of blocks in flight between the host and the device: up, compress (or decompress), down.
struct Slot {
    Dev<uint8_t> d_src;
    Dev<uint8_t> d_dst;
    Dev<uint64_t> d_sizes;
    Pinned<uint64_t> h_sizes;  // [n] stream lengths + [1] the nb_state behind the group (the feed)
    Event ev_up, ev_comp, ev_down;
};

// rspt_hip_compress_many / rspt_hip_decompress_many: two slots of a chunk of blocks each
struct ManyStaging {
    size_t chunk = 0, stride = 0;
    Slot slot[2];
    Dev<uint64_t> idx[2];  // [4 + 2 x chunk] a container header + index over a slot's streams (decompress_many with src_len)
    Pinned<uint64_t> hidx;  // 2 x (4 + 2 x chunk)
};

// rspt_hip_feed_*: a ring of block groups in flight
struct FeedSlot : Slot {
    enum State { FREE, FILLING, COMPRESSING, DOWNLOADING, DONE } state = FREE;
    std::vector<void*> dst_host;
    std::vector<size_t> dst_cap;
    size_t count = 0, delivered = 0, first_seq = 0;
    int error = 0;  // the group's launch failed: every block of it is reported with this status
};
struct Feed {
    size_t G = 0, stride = 0;
    std::vector<FeedSlot> slots;
    size_t head = 0, tail = 0;  // ring positions: oldest slot not yet FREE; the slot being filled / filled next
    size_t next_seq = 0;
};

// rspt_hip_gather_post_*: two slots of sizes (device + page-locked host) and events, on a gather stream of their own
struct LagGather {
    Stream stream;
    Dev<uint64_t> dtotals[2];
    Pinned<uint64_t> htotals[2];
    Event ev_in[2], ev_sizes[2], ev_payload[2];
    bool posted[2] = {false, false};
    int world = 0;
};

// The last call of a windowed stage (FIR, median) that uses a set of the handle's buffers: `done` is recorded behind the call's
// kernels on the caller's stream, and the buffers are refilled, replaced or released only once the device is past it.
struct LastCall {
    Event done;  // made by the first call
    bool used = false;
    bool make_event() { return done || hipEventCreateWithFlags(done.out(), hipEventDisableTiming) == hipSuccess; }
    hipError_t wait() const { return used ? hipEventSynchronize(done) : hipSuccess; }
    // (a failed record leaves nothing to wait on later: the device gets past the buffers now)
    hipError_t record(hipStream_t st) {
        const hipError_t e = hipEventRecord(done, st);
        if (e != hipSuccess) hipStreamSynchronize(st);
        used = e == hipSuccess;
        return e;
    }
};

// rspt_hip_fir_prefilter_batch_dev: the coefficients of the last kSlots calls (the caller's array may go as soon as a call
// returns, so each call copies it into page-locked memory and from there, on the call's stream, to the device), and the halo
// rows of an in-place call.  A slot is refilled only once its last call is past it; the halo is replaced, and the handle
// destroyed, only once the calls of all slots are.  rspt_hip_fir_prefilter_stream_dev adds `head`, the staged K - 1 rows in front
// of a carried-state call, under the same rule.
struct FirStage {
    static constexpr int kSlots = 4;
    struct CoefSlot {
        Pinned<double> host;
        Dev<double> dev;
        size_t cap = 0;
        LastCall last;
    };
    CoefSlot slot[kSlots];
    int next = 0;
    Dev<uint8_t> halo, head;
    size_t halo_cap = 0, head_cap = 0;
    void wait_all() {
        for (CoefSlot& s : slot) s.last.wait();
    }
};

// rspt_hip_median_filter_batch_dev: the halo rows of an in-place short-window call, and the sort buffers of the generic path
// (two key buffers and the ranks of one piece of the batch), all behind the stage's last call.
// rspt_hip_median_filter_stream_dev adds `head`, the staged copy of a carried-state call's old state, under the same rule.
struct MedianStage {
    Dev<uint8_t> halo, head;
    size_t halo_cap = 0, head_cap = 0;
    Dev<uint64_t> keys_a, keys_b;
    Dev<uint32_t> rank;
    size_t key_cap = 0;  // samples of each of the three
    LastCall last;
};

// The members are constructed in the order they are declared and released in the reverse order (rspt_hip_packer_destroy).
struct rspt_hip_packer {
    Geom g{};
    int device = 0;
    int last_hip_error = 0;
    unsigned nb_ctor = 0;
    unsigned nb_host = 0;  // last value of the device nb_state the host has seen (a lower bound: nb only grows)
    int num_cu = 256;
    uint32_t dirty_shift = 0;  // (Workspace::plane_dirty)
    // dct (signal_packer_dct.cpp:60-74)
    double dct_scale0 = 0, dct_scale1 = 0, idct_scale = 0;
    float dct_cs0 = 0;
    // dct beyond the dense table: fp64 FFT path (transforms.hip: k_dctfft_*)
    bool dct_fft = false;
    uint32_t fft_l1 = 0, fft_l2 = 0;   // n = 2^(l1+l2)
    bool dct_real = false;             // forward transform through the real-input FFT (n >= 256)
    uint32_t fftr_la = 0, fftr_lb = 0; // n/2 = 2^(la+lb)
    uint32_t ntile = 0;
    uint32_t Tn_native = 0;  // tile of k_planar_native; 0: one row of all channels does not fit its LDS (more than 8192 channels) -> k_wide_native
    // tile geometry for the front end
    uint32_t T = 0, in_lds = 0;  // k_tile_planar: tile staged in LDS
    uint32_t Tp[5] = {0, 0, 0, 0, 0};  // k_tile_planes: tile length when kcount planes are staged: rows [kcount*nch][Tp+16] + nz flags
    bool wide = false;          // more channels than a 16-sample tile of the front-end kernels holds in LDS: k_wide_planar + k_planar_planes
    uint32_t k1_threads = 256;  // workgroup size of k_tile_planes (RSPT_K1_THREADS)
    uint32_t k1_grid = 0;       // workgroups of k_tile_planes; 0 = by LDS footprint (RSPT_K1_GRID, tuning knob)
    uint32_t hist_grid = 0;     // workgroups of the persistent k_hist / k_encode; 0 = two per CU (a CU's wave slots: one batch at a time)
    uint32_t enc_grid = 0;
    uint32_t ablate = 0;  // RSPT_ABLATE (diagnostic builds only; the product kernels ignore it): timing probes
    uint32_t psel = 0;    // RSPT_PLANESEL (diagnostic builds only): which planes the hzr kernels take; bit 8 / 9: stop behind k_hist / k_tree
    int verify = 0;       // decompress checks the block CRCs (rspt_hip_set_verify)
    int big_endian = 0;   // samples arrive / leave with their bytes reversed (rspt_hip_set_byte_order)
    bool profiling = false;
    bool ev_valid = false;
    bool conv_lds_raised = false;  // rspt_hip_native_to_i32_batch_dev has raised k_tile_planar's dynamic LDS limit

    // ---- per-handle constants (rspt_hip_packer_create) ----
    Stream stream;
    Event ev[ST_COUNT + 1];  // profiling
    Dev<unsigned long long> stamps;  // diagnostic s_memtime stamps: [512 hzr blocks][16 waves][8]
    Dev<CrcConsts> crc;
    Dev<uint32_t> nb_state;  // [4] persistent: [0] = nb; [2] = work counter of the decoder's persistent grid (zeroed by k_dec_frame)
    // dct: COS[x][i] and its transpose, built on the host like the reference ctor; beyond the dense table the FFT twiddles
    Dev<float> cos_tab, cos_tab_t;
    Dev<double2> fft_tw;    // [n] (cos, sin)(2 pi t / n)
    Dev<double2> fft_post;  // [n] (cos, sin)(pi k / 2n)
    // the copy streams of the many-block pipeline and the feed, made by whichever of them comes first
    Stream m_up, m_down;

    // ---- the workspace, and the views into its per-call zero region (set by every compress call) ----
    Workspace ws;
    uint32_t* nzflag = nullptr;    // view: [cap*4*nblk] set by the front end when an hzr block holds a non-zero byte (= zbuf[set of the last call])
    uint32_t* needmask = nullptr;  // view: [cap]
    uint32_t* work_ctr = nullptr;  // view: [16] work counter of the persistent k_hist at 0, the WorkQueues of k_encode from 4 (zeroed per call)
    long long* row_sum = nullptr;  // view: [blocks][nch] channel sums taken by the de-interleave pass (dct at large ns)
    bool have_row_sum = false;     // this call's front end filled row_sum

    // ---- host API staging ----
    HostStaging stage;
    ManyStaging many;
    std::unique_ptr<Feed> feed;  // open between rspt_hip_feed_begin and rspt_hip_feed_end

    // ---- FIR pre-filter stage ----
    FirStage fir;

    // ---- rolling median stage ----
    MedianStage med;

    // ---- gather state ----
    Dev<uint64_t> gat_totals;  // [gat_world]: container lengths of all ranks (rspt_hip_gather_containers)
    int gat_world = 0;
    LagGather lag;
};

#define HIPCHK(p, call)                         \
    do {                                        \
        hipError_t e_ = (call);                 \
        if (e_ != hipSuccess) {                 \
            (p)->last_hip_error = (int)e_;      \
            return RSPT_HIP_ERR_LAUNCH;         \
        }                                       \
    } while (0)

static void stamp(rspt_hip_packer* p, int i, hipStream_t st) {
    if (p->profiling) hipEventRecord(p->ev[i], st);
}

// f(std::integral_constant<int, BPS>()) for the handle's sample width
template <class F>
static auto by_bps(uint32_t bps, F&& f) {
    switch (bps) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        default: return f(std::integral_constant<int, 4>());
    }
}

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
static void launch_fwht_big(rspt_hip_packer* p, uint32_t B, hipStream_t st) {
    const Geom& g = p->g;
    const uint32_t segs = g.ns >> 15;  // 32768-point pieces per row: 4 .. 128
    hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht_seg), hipFuncAttributeMaxDynamicSharedMemorySize, 32768 * 4);
    hipLaunchKernelGGL(k_fwht_seg, dim3(segs, g.nch, B), dim3(1024), 32768 * 4, st, p->ws.planar, g);
    const uint32_t m1 = segs > 64u ? 64u : segs, m2 = segs / m1;
    hipLaunchKernelGGL((k_fwht_cross<FORWARD>), dim3(g.ns / m1 / 256u, g.nch, B), dim3(256), 0, st, p->ws.planar, g, p->ws.means, p->ws.mean_i32, m1, 32768u,
                       m2 == 1u ? 1u : 0u);
    if (m2 > 1u)
        hipLaunchKernelGGL((k_fwht_cross<FORWARD>), dim3(g.ns / m2 / 256u, g.nch, B), dim3(256), 0, st, p->ws.planar, g, p->ws.means, p->ws.mean_i32, m2,
                           32768u * m1, 1u);
}

template <int BPS>
static void launch_fixup(rspt_hip_packer* p, const uint8_t* d_src, size_t nblocks, uint32_t np, hipStream_t st) {
    launch_planes<BPS, true>(p, d_src, nblocks, np, 4 - np, p->ws.nbuse, st);
}


template <int BPS, int NC>
static void launch_iir(rspt_hip_packer* p, uint8_t* buf, uint32_t B, const IirCoef& c, int per_channel, hipStream_t st) {
    const Geom& g = p->g;
    if (g.ns >= kIirChunk && c.init_steps >= NC - 1) {  // the pipelined form: recurrence, feed-forward sums and stores on waves of their own
        const bool al = (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(buf) % BPS) == 0;  // (block_bytes is a multiple of BPS)
        if (per_channel) {
            const uint32_t units = B * g.nch;
            auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((units + 63) / 64), dim3(kIirThreads), 0, st, buf, g.nch, g.ns, (uint64_t)g.block_bytes, c, B, 64u, (IirCarry*)nullptr); };
            if (al) go(&k_iir_pipe<BPS, NC, false, (BPS == 4 || BPS == 2)>);
            else go(&k_iir_pipe<BPS, NC, false, false>);
        } else {
            // shared mode: lane <-> block; few lanes per workgroup so that the blocks' scattered accesses spread over the CUs
            uint32_t lpw = (B + (uint32_t)p->num_cu - 1) / (uint32_t)p->num_cu;
            lpw = lpw < 1 ? 1 : lpw > 64 ? 64 : lpw;
            auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((B + lpw - 1) / lpw), dim3(kIirThreads), 0, st, buf, g.nch, g.ns, (uint64_t)g.block_bytes, c, B, lpw, (IirCarry*)nullptr); };
            if (al) go(&k_iir_pipe<BPS, NC, true, (BPS == 4 || BPS == 2)>);
            else go(&k_iir_pipe<BPS, NC, true, false>);
        }
        return;
    }
    if (per_channel) {
        const uint32_t threads = B * g.nch;
        hipLaunchKernelGGL((k_iir<BPS, NC, false>), dim3((threads + 63) / 64), dim3(64), 0, st, buf, g.nch, g.ns, (uint64_t)g.block_bytes, c, B);
    } else {
        hipLaunchKernelGGL((k_iir<BPS, NC, true>), dim3((B + 63) / 64), dim3(64), 0, st, buf, g.nch, g.ns, (uint64_t)g.block_bytes, c, B);
    }
}
template <int BPS>
static void launch_iir_nc(rspt_hip_packer* p, uint8_t* buf, uint32_t B, const IirCoef& c, int per_channel, hipStream_t st) {
    switch (c.nc) {
        case 2: launch_iir<BPS, 2>(p, buf, B, c, per_channel, st); break;
        case 3: launch_iir<BPS, 3>(p, buf, B, c, per_channel, st); break;
        case 4: launch_iir<BPS, 4>(p, buf, B, c, per_channel, st); break;
        default: launch_iir<BPS, 5>(p, buf, B, c, per_channel, st); break;
    }
}

// The carried form (rspt_hip_iir_prefilter_stream_dev): the call's blocks as one run of `rows` rows, lane <-> channel, the
// filters in `state`.  Whether a channel is fresh is known on the device only, so the route depends on the run's length alone.
template <int BPS, int NC>
static void launch_iir_stream(rspt_hip_packer* p, uint8_t* buf, uint32_t rows, const IirCoef& c, IirCarry* state, hipStream_t st) {
    const Geom& g = p->g;
    const dim3 grid((g.nch + 63) / 64);
    if (rows >= kIirChunk) {
        const bool al = (BPS == 4 || BPS == 2) && (reinterpret_cast<uintptr_t>(buf) % BPS) == 0;
        const uint64_t run_bytes = (uint64_t)rows * g.nch * BPS;
        auto go = [&](auto kern) { hipLaunchKernelGGL(kern, grid, dim3(kIirThreads), 0, st, buf, g.nch, rows, run_bytes, c, 1u, 64u, state); };
        if (al) go(&k_iir_pipe<BPS, NC, false, (BPS == 4 || BPS == 2), true>);
        else go(&k_iir_pipe<BPS, NC, false, false, true>);
        return;
    }
    hipLaunchKernelGGL((k_iir_carry<BPS, NC>), grid, dim3(64), 0, st, buf, g.nch, rows, c, state);
}
template <int BPS>
static void launch_iir_stream_nc(rspt_hip_packer* p, uint8_t* buf, uint32_t rows, const IirCoef& c, IirCarry* state, hipStream_t st) {
    switch (c.nc) {
        case 2: launch_iir_stream<BPS, 2>(p, buf, rows, c, state, st); break;
        case 3: launch_iir_stream<BPS, 3>(p, buf, rows, c, state, st); break;
        case 4: launch_iir_stream<BPS, 4>(p, buf, rows, c, state, st); break;
        default: launch_iir_stream<BPS, 5>(p, buf, rows, c, state, st); break;
    }
}

// The decomposition of a sliding-window stage (WinGeom): channel groups of up to `threads` lanes' channels, runs of `run`
// outputs per lane (kFirThreads / kFirR, kMedThreads / kMedRun), and spans along the time axis until there are about four
// workgroups per CU -- each span at least 4 (K - 1) rows, so that the halo an in-place call stages is at most a quarter of the
// batch.  run_rows != 0 (a carried-state call): the nblocks blocks, back to back, taken as ONE block of run_rows = nblocks * ns rows.
static WinGeom win_geom(const rspt_hip_packer* p, size_t nblocks, uint32_t K, uint32_t threads, uint32_t run, uint32_t run_rows = 0) {
    Geom g = p->g;
    if (run_rows) {
        g.ns = run_rows;
        g.block_bytes = (uint64_t)run_rows * g.nch * g.bps;
        nblocks = 1;
    }
    WinGeom f{};
    f.block_bytes = g.block_bytes;
    f.stride = g.nch * g.bps;  // (window_call_checks checks the chunk's row offsets before a launch)
    f.nch = g.nch;
    f.ns = g.ns;
    f.K = K;
    f.cw = g.nch < threads ? g.nch : threads;
    f.subs = threads / f.cw;
    f.ncg = (g.nch + f.cw - 1) / f.cw;
    const uint32_t C = f.subs * run;
    const uint64_t base_units = (uint64_t)nblocks * f.ncg;
    const uint64_t want = 4ull * (uint64_t)p->num_cu;
    uint64_t nsplit = base_units >= want ? 1 : (want + base_units - 1) / base_units;
    const uint64_t min_span = K > 1 ? 4ull * (K - 1) : 1;
    const uint64_t max_split = g.ns / (min_span > C ? min_span : C);
    nsplit = nsplit > max_split ? max_split : nsplit;
    nsplit = nsplit < 1 ? 1 : nsplit;
    const uint64_t span = ((g.ns + nsplit - 1) / nsplit + C - 1) / C * C;
    f.span = (uint32_t)span;
    f.nsplit = (uint32_t)((g.ns + span - 1) / span);
    f.units = base_units * f.nsplit;
    return f;
}

template <int BPS>
static void launch_fir(const WinGeom& f, const uint8_t* src, uint8_t* dst, const uint8_t* halo, const double* coef, bool aligned, hipStream_t st,
                       const uint8_t* head = nullptr) {
    const uint32_t grid = (uint32_t)(f.units < (1u << 20) ? f.units : (1u << 20));
    if (aligned) hipLaunchKernelGGL((k_fir<BPS, (BPS == 4 || BPS == 2)>), dim3(grid), dim3(kFirThreads), 0, st, src, dst, halo, coef, f, head);
    else hipLaunchKernelGGL((k_fir<BPS, false>), dim3(grid), dim3(kFirThreads), 0, st, src, dst, halo, coef, f, head);
}

template <uint32_t N, int BPS, bool HEAD>
static void launch_med_short(const WinGeom& f, const uint8_t* src, uint8_t* dst, const uint8_t* halo, bool aligned, hipStream_t st, const uint8_t* head) {
    const uint32_t grid = (uint32_t)(f.units < (1u << 20) ? f.units : (1u << 20));
    if (aligned) hipLaunchKernelGGL((k_med_short<N, BPS, (BPS == 4 || BPS == 2), HEAD>), dim3(grid), dim3(kMedThreads), 0, st, src, dst, halo, f, head);
    else hipLaunchKernelGGL((k_med_short<N, BPS, false, HEAD>), dim3(grid), dim3(kMedThreads), 0, st, src, dst, halo, f, head);
}

// k_med_short by its register bucket: the smallest of 4, 8, 16, 32 that holds W.
template <bool HEAD>
static hipError_t launch_med_short_w(uint32_t bps, const WinGeom& f, const void* d_src, void* d_dst, const uint8_t* halo, bool aligned, hipStream_t st,
                                     const uint8_t* head) {
    const uint32_t W = f.K;
    by_bps(bps, [&](auto bb) {
        constexpr int B = decltype(bb)::value;
        if (W <= 4) launch_med_short<4, B, HEAD>(f, (const uint8_t*)d_src, (uint8_t*)d_dst, halo, aligned, st, head);
        else if (W <= 8) launch_med_short<8, B, HEAD>(f, (const uint8_t*)d_src, (uint8_t*)d_dst, halo, aligned, st, head);
        else if (W <= 16) launch_med_short<16, B, HEAD>(f, (const uint8_t*)d_src, (uint8_t*)d_dst, halo, aligned, st, head);
        else launch_med_short<32, B, HEAD>(f, (const uint8_t*)d_src, (uint8_t*)d_dst, halo, aligned, st, head);
    });
    return hipGetLastError();
}

// The generic path on the pairs [pair0, pair0 + npairs) of the batch: sort (tile sort, merge passes), then walk.  STREAM: a pair
// is a (segment, channel) of a carried-state call and f.ns the segment capacity (median.hip).
template <int BPS, bool STREAM = false>
static hipError_t launch_med_generic(rspt_hip_packer* p, const WinGeom& f, const uint8_t* src, uint8_t* dst, uint64_t pair0, uint64_t npairs,
                                     bool aligned, hipStream_t st, const MedSeg& sg = MedSeg{}) {
    MedianStage& ms = p->med;
    const uint32_t ns = f.ns;
    const uint32_t tiles = (ns + kMedTile - 1) / kMedTile;
    uint64_t* a = ms.keys_a;
    uint64_t* b = ms.keys_b;
    uint32_t* rank = ms.rank;
    const bool one_tile = tiles == 1;
    if (aligned) hipLaunchKernelGGL((k_med_tile_sort<BPS, (BPS == 4 || BPS == 2), STREAM>), dim3((uint32_t)(npairs * tiles)), dim3(kMedThreads), 0, st, src,
                                    a, one_tile ? rank : nullptr, f, pair0, sg);
    else hipLaunchKernelGGL((k_med_tile_sort<BPS, false, STREAM>), dim3((uint32_t)(npairs * tiles)), dim3(kMedThreads), 0, st, src, a,
                            one_tile ? rank : nullptr, f, pair0, sg);
    hipError_t e = hipGetLastError();
    const uint64_t total = npairs * ns;
    for (uint32_t width = kMedTile; e == hipSuccess && width < ns; width *= 2) {
        const bool last = (uint64_t)width * 2 >= ns;
        hipLaunchKernelGGL(k_med_merge, dim3((uint32_t)((total + kMedThreads - 1) / kMedThreads)), dim3(kMedThreads), 0, st, a, b, last ? rank : nullptr, ns,
                           width, total);
        e = hipGetLastError();
        std::swap(a, b);
    }
    if (e != hipSuccess) return e;
    const uint32_t spans = ((STREAM ? sg.L : ns) + kMedSpan - 1) / kMedSpan;
    const uint32_t n0 = (ns + 31) / 32;
    const size_t lds = (size_t)(n0 + (n0 + 31) / 32) * sizeof(uint32_t);
    if (aligned) hipLaunchKernelGGL((k_med_walk<BPS, (BPS == 4 || BPS == 2), STREAM>), dim3((uint32_t)(npairs * spans)), dim3(64), lds, st, a, rank, dst, f,
                                    pair0, sg);
    else hipLaunchKernelGGL((k_med_walk<BPS, false, STREAM>), dim3((uint32_t)(npairs * spans)), dim3(64), lds, st, a, rank, dst, f, pair0, sg);
    return hipGetLastError();
}

// The reference's channel limit: convert_native_to_i32 / convert_i32_to_native, which every one of its programs runs first and
// last, count channels with a uint16_t (utils.cpp:57, 129) -- 65536 channels never terminate there.
static constexpr size_t kMaxChannels = 65535;
// The widest handle the filter, median, peak and PRDN stages are verified on (tests/test_gpu_wide_channels.py): beyond it they
// return RSPT_HIP_ERR_UNSUPPORTED before anything is launched.
static constexpr uint32_t kStageMaxChannels = 8191;
static bool stage_too_wide(const rspt_hip_packer* p) { return p->g.nch > kStageMaxChannels; }

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

// The checks both peak entries make, and the kernel arguments from them (all of PeakOffArgs but its workspace): false where
// either entry refuses the call.
static bool peak_args(rspt_hip_packer* p, const void* d_src, size_t nblocks, double sampling_rate, void* d_state, uint32_t* d_count,
                      int32_t* d_index, double* d_value, size_t max_peaks, double* d_sig, double* d_threshold, PeakArgs& a) {
    if (!p || !d_src || !d_count || nblocks == 0) return false;
    if (!std::isfinite(sampling_rate) || sampling_rate <= 0 || sampling_rate > (double)(1 << 20)) return false;
    if (max_peaks > 0 && (!d_index || !d_value)) return false;
    if ((uint64_t)max_peaks > (1ull << 32) || (!d_sig) != (!d_threshold)) return false;
    const Geom& g = p->g;
    if ((uint64_t)nblocks * g.nch >= (1ull << 31)) return false;
    a.src = (const uint8_t*)d_src;
    a.block_bytes = g.block_bytes;
    a.stride = g.nch * g.bps;
    a.nch = g.nch;
    a.ns = g.ns;
    a.nblocks = (uint32_t)nblocks;
    a.lanes = d_state ? g.nch : (uint32_t)(nblocks * g.nch);
    a.state = (uint8_t*)d_state;
    a.count = d_count;
    a.index = d_index;
    a.value = d_value;
    a.max_peaks = max_peaks;
    a.sig = d_sig;
    a.thr = d_threshold;
    return true;
}

// A variant's three filters as the detector's constructor designs them (create_filter_iir(f.d, f.n, ...): numerator -> d), and
// its constants.  (Every design is valid for fs > 0.)
static bool peak_coef(int variant, double sampling_rate, double marker_val, PeakCoef& c) {
    static const struct { int bp_order; double bp_lo, bp_hi; int ig_order; double A; } kVar[3] = {
        {2, 10.0, 20.0, 2, 25.0}, {1, 10.0, 20.0, 1, 25.0}, {1, 15.0, 25.0, 1, 70.0}};
    const auto& v = kVar[variant];
    if (!design_iir(kFiltBandPass, v.bp_order, sampling_rate, v.bp_lo, v.bp_hi, c.bf, c.bb) ||
        !design_iir(kFiltLowPass, v.ig_order, sampling_rate, 3.0, 0.0, c.gf, c.gb) ||
        !design_iir(kFiltLowPass, 2, sampling_rate, 0.15, 0.0, c.tf, c.tb))
        return false;
    c.atten = 1.0 / (1.0 + v.A / sampling_rate);
    c.marker = marker_val;
    c.nslope = (int32_t)((100.0 * sampling_rate) / 1000.0);
    c.hist = 4 * (int32_t)sampling_rate;
    return true;
}

// One lane per detector, 64 to a workgroup, on the caller's stream.
template <class Args, class Coef>
static int peak_launch(rspt_hip_packer* p, void (*kern)(Args, Coef), const Args& a, const Coef& c, void* stream) {
    HIPCHK(p, hipSetDevice(p->device));
    hipLaunchKernelGGL(kern, dim3((a.lanes + 63) / 64), dim3(64), 0, (hipStream_t)stream, a, c);
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
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
    if (kind == RSPT_HIP_KIND_DCT) {
        const double ratio1 = sqrt(2.0 / (double)(int)ns);
        const float cs0 = (float)(1 / sqrt(2));
        p->dct_cs0 = cs0;
        p->dct_scale0 = cs0 * ratio1 / 128.0;   // Cs[0]*ratio1/quality (dct.cpp:84)
        p->dct_scale1 = 1.0f * ratio1 / 128.0;  // Cs[i>0] = 1
        p->idct_scale = ratio1 * 128.0;          // dct.cpp:97
    }
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
    const unsigned nbmax = p->g.kind == RSPT_HIP_KIND_XDELTA_HZR ? 4u : p->nb_ctor;
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
    ok &= hipMalloc(w.quality.out(), max_blocks * ((size_t)g.nch + 5) * sizeof(unsigned long long)) == hipSuccess;
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

// ---- the compress sequence, phase by phase ----------------------------------------------------------------------------------------
// (Round 4 measured whether the phases of TWO batches can overlap -- two whole batches racing on two streams, and an ordered
// schedule with the latency-bound middle of batch i on a second stream beside the front end of batch i+1: neither beats one
// batch at a time on one stream; profiles/r04_notes.md, profiles/r04_pipeline_experiment.patch.)
// front:  zero region, front-end kernel(s), escalation scan / fix-up, list of k_hist's blocks     (HBM-bound)
// hist:   k_hist                                                                                  (vector-issue bound)
// tree:   k_tree + k_layout                                                                       (latency chains, chip mostly idle; the
//                                                                                                  small blocks are encoded under the dense trees)
// encode: k_encode                                                                                (vector-issue bound)
static int phase_front(rspt_hip_packer* p, const uint8_t* src, size_t nblocks, hipStream_t st) {
    const Geom& g = p->g;
    const uint32_t B = (uint32_t)nblocks;
    stamp(p, ST_PRE, st);
    const bool xd = g.kind == RSPT_HIP_KIND_XDELTA_HZR;
    {
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
    }
    if (p->ws.planes_unknown || (p->ablate & ~(3u << 26)) || p->psel) {  // (diagnostic runs skip kernels and stores: never trust the planes they leave; probes 26 / 27 store everything)
        HIPCHK(p, hipMemsetAsync(p->ws.plane_dirty, 0xFF, p->ws.cap_slots * kMaxPlanes * 4 * sizeof(uint32_t), st));
        p->ws.planes_unknown = false;
    }
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
    const uint32_t np = by_bps(g.bps, [&](auto bps) { return launch_front<decltype(bps)::value>(p, src, nblocks, st); });
    if (g.kind == RSPT_HIP_KIND_HADAMARD) {
        // per channel: mean removal, WHT, truncating /n (signal_packer_hadamard.cpp:57-72)
        const uint32_t fw_lds = (g.ns > 32768u ? 32768u : g.ns) * 4u;
        if (g.ns > 65536u) {  // two passes over the planar row (any 2^k the reference's own transform takes, fwht.c:4-28)
            hipLaunchKernelGGL(k_row_means, dim3(g.nch, B), dim3(1024), 0, st, p->ws.planar, g, p->ws.means, p->ws.mean_i32);
            launch_fwht_big<true>(p, B, st);
            hipLaunchKernelGGL((k_planar_planes<false>), dim3((g.N + 4095) / 4096, B), dim3(256), 0, st, p->ws.planar, g, 3u, p->ws.planes, p->nzflag, (uint32_t*)nullptr);
        } else if (g.ns == 65536u) {  // the whole row in registers: read once, and the byte planes written straight from them
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht64k<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
            hipLaunchKernelGGL((k_fwht64k<true, true>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, p->ws.planes, p->nzflag, 3u);
        } else {
            hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
            hipLaunchKernelGGL((k_fwht<true>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means);
            hipLaunchKernelGGL((k_planar_planes<false>), dim3((g.N + 4095) / 4096, B), dim3(256), 0, st, p->ws.planar, g, 3u, p->ws.planes, p->nzflag, (uint32_t*)nullptr);
        }
    } else if (g.kind == RSPT_HIP_KIND_DCT) {
        if (p->dct_fft) {
            if (p->have_row_sum)  // the de-interleave pass summed the channels on its way: no second pass over the planar block
                hipLaunchKernelGGL(k_means_from_sums, dim3((B * g.nch + 255) / 256), dim3(256), 0, st, p->row_sum, g, B, p->ws.means, p->ws.mean_i32);
            else
                hipLaunchKernelGGL(k_row_means, dim3(g.nch, B), dim3(1024), 0, st, p->ws.planar, g, p->ws.means, p->ws.mean_i32);
            launch_dct_fft<true>(p, B, p->ws.planar, p->ws.planar2, st);
        } else {
            hipLaunchKernelGGL((k_dct<true>), dim3((g.ns + 255) / 256, (g.nch + kDctCh - 1) / kDctCh, B), dim3(256), 0, st, p->ws.planar, g, p->ws.means,
                               p->cos_tab, p->dct_scale0, p->dct_scale1, p->dct_cs0, p->ws.planar2);
        }
        hipLaunchKernelGGL((k_planar_planes<true>), dim3((g.N + 4095) / 4096, B), dim3(256), 0, st, p->ws.planar2, g, 2u, p->ws.planes, p->nzflag, (uint32_t*)nullptr);
    }
    HIPCHK(p, hipGetLastError());

    stamp(p, ST_NB, st);
    if (g.kind != RSPT_HIP_KIND_XDELTA_HZR && g.kind != RSPT_HIP_KIND_HZR)  // (k_tile_planes runs the scan in its last workgroup)
        hipLaunchKernelGGL(k_nb_scan, dim3(1), dim3(1024), 0, st, p->needmask, B, p->nb_state, p->ws.nbuse, 0);
    if (xd && np < 4)  // nb may have escalated in this call: add the planes the main pass did not write
        by_bps(g.bps, [&](auto bps) { launch_fixup<decltype(bps)::value>(p, src, nblocks, np, st); });
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
static int compress_batch_serial(rspt_hip_packer* p, const void* d_src, size_t nblocks, void* d_dst, size_t dst_stride, uint64_t* d_sizes, hipStream_t st) {
    int rc = rspt_hip_reserve(p, nblocks);
    if (rc) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    const uint32_t B = (uint32_t)slots_of(p, nblocks);  // what the hzr kernels count in
    if ((rc = phase_front(p, (const uint8_t*)d_src, nblocks, st)) != 0) return rc;
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
    if ((rc = phase_layout(p, B, d_dst, dst_stride, d_sizes, st)) != 0) return rc;

    stamp(p, ST_ENCODE, st);
    if ((rc = phase_encode(p, B, d_dst, dst_stride, st)) != 0) return rc;
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
    s.dst_cap = rspt_hip_max_compressed_size(p) + 64;
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

static int decompress_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, const uint64_t* pidx, size_t packed_len, size_t nblocks,
                          void* d_dst, uint64_t* d_consumed, void* stream);

int rspt_hip_decompress_batch_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, size_t nblocks, void* d_dst, uint64_t* d_consumed,
                                  void* stream) {
    return decompress_dev(p, d_src, src_stride, nullptr, 0, nblocks, d_dst, d_consumed, stream);
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

static int decompress_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, const uint64_t* pidx, size_t packed_len, size_t nblocks,
                          void* d_dst, uint64_t* d_consumed, void* stream) {
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
        const dim3 tg(p->ntile, B);
        // int32 samples of the two hzr packers: the last inverse pass writes the interleaved block itself (k_inv_native)
        const bool direct = (g.kind == RSPT_HIP_KIND_XDELTA_HZR || g.kind == RSPT_HIP_KIND_HZR) && g.bps == 4 && (g.nch & 3) == 0 &&
                            g.ns % kRowTile == 0 && (reinterpret_cast<uintptr_t>(d_dst) & 15) == 0;
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
        if (xd) {
            hipLaunchKernelGGL((k_inv_tile<0, true>), tg, dim3(256), 0, st, p->ws.planes, g, p->ws.dec_nb, p->ntile, p->ws.txor, p->ws.tsum, p->ws.planar);
            hipLaunchKernelGGL((k_inv_scan_tiles<true>), dim3(B), dim3(1024), 0, st, p->ws.txor, p->ntile);
            hipLaunchKernelGGL((k_inv_tile<1, true>), tg, dim3(256), 0, st, p->ws.planes, g, p->ws.dec_nb, p->ntile, p->ws.txor, p->ws.tsum, p->ws.planar);
            hipLaunchKernelGGL((k_inv_scan_tiles<false>), dim3(B), dim3(1024), 0, st, p->ws.tsum, p->ntile);
            hipLaunchKernelGGL((k_inv_tile<2, true>), tg, dim3(256), 0, st, p->ws.planes, g, p->ws.dec_nb, p->ntile, p->ws.txor, p->ws.tsum, p->ws.planar);
        } else {
            hipLaunchKernelGGL((k_inv_tile<2, false>), tg, dim3(256), 0, st, p->ws.planes, g, p->ws.dec_nb, p->ntile, p->ws.txor, p->ws.tsum, p->ws.planar);
        }
        const int32_t* final_planar = p->ws.planar;
        if (g.kind == RSPT_HIP_KIND_HADAMARD) {
            const uint32_t fw_lds = (g.ns > 32768u ? 32768u : g.ns) * 4u;
            if (g.ns > 65536u) {
                launch_fwht_big<false>(p, B, st);
            } else if (g.ns == 65536u) {
                hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht64k<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
                hipLaunchKernelGGL((k_fwht64k<false, false>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means, (uint8_t*)nullptr,
                                   (uint32_t*)nullptr, 0u);
            } else {
                hipFuncSetAttribute(reinterpret_cast<const void*>(&k_fwht<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fw_lds);
                hipLaunchKernelGGL((k_fwht<false>), dim3(g.nch, B), dim3(1024), fw_lds, st, p->ws.planar, g, p->ws.means);
            }
        } else if (g.kind == RSPT_HIP_KIND_DCT) {
            if (p->dct_fft)
                launch_dct_fft<false>(p, B, p->ws.planar, p->ws.planar2, st);
            else
                hipLaunchKernelGGL((k_dct<false>), dim3((g.ns + 255) / 256, (g.nch + kDctCh - 1) / kDctCh, B), dim3(256), 0, st, p->ws.planar, g,
                                   p->ws.means, p->cos_tab_t, 0.0, p->idct_scale, p->dct_cs0, p->ws.planar2);
            final_planar = p->ws.planar2;
        }
        const uint32_t T = min(p->Tn_native, g.ns);
        const uint32_t lds = g.nch * (T + 1) * 4;
        const dim3 ng(T ? (g.ns + T - 1) / T : 0u, B);
        if (T == 0) {  // more channels than k_planar_native holds a row of: 64 x 64 tiles
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

int rspt_hip_iir_prefilter_batch_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, size_t nr_coefficients,
                                     int init_nr_samples, int per_channel, void* stream) {
    if (!p || !d_buf || !n || !d || nblocks == 0 || nblocks > 0x7FFFFFFFu / (p->g.nch ? p->g.nch : 1)) return RSPT_HIP_ERR_ARG;
    if (nr_coefficients < 2 || nr_coefficients > 5 || init_nr_samples < 0 || init_nr_samples > (1 << 28)) return RSPT_HIP_ERR_ARG;  // filter_opt covers 2..5 (iir_filter.cpp:87-103)
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    HIPCHK(p, hipSetDevice(p->device));
    IirCoef c{};
    for (size_t i = 0; i < nr_coefficients; ++i) {
        c.n[i] = n[i];
        c.d[i] = d[i];
    }
    c.nc = (uint32_t)nr_coefficients;
    c.init_steps = 4 * init_nr_samples;
    hipStream_t st = (hipStream_t)stream;
    by_bps(p->g.bps, [&](auto bps) { launch_iir_nc<decltype(bps)::value>(p, (uint8_t*)d_buf, (uint32_t)nblocks, c, per_channel, st); });
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

// A carried-state call takes its blocks as one run of nblocks * ns rows, indexed in 32 bits with a chunk's reach beyond the last
// row: runs of 2^31 - 2^17 rows and more are refused, and the caller splits the call (with a state that split is exact).
static constexpr uint64_t kStreamMaxRows = (1ull << 31) - (1ull << 17);

int rspt_hip_iir_state_bytes(rspt_hip_packer* p, size_t* bytes) {
    if (!p || !bytes) return RSPT_HIP_ERR_ARG;
    *bytes = (size_t)p->g.nch * sizeof(IirCarry);
    return RSPT_HIP_OK;
}

int rspt_hip_iir_prefilter_stream_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, size_t nr_coefficients,
                                      int init_nr_samples, void* d_state, void* stream) {
    if (!p || !d_buf || !n || !d || nblocks == 0 || nblocks > 0x7FFFFFFFu / (p->g.nch ? p->g.nch : 1)) return RSPT_HIP_ERR_ARG;
    if (nr_coefficients < 2 || nr_coefficients > 5 || init_nr_samples < 0 || init_nr_samples > (1 << 28)) return RSPT_HIP_ERR_ARG;
    if (!d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    const uint64_t rows = (uint64_t)nblocks * p->g.ns;
    if (rows >= kStreamMaxRows) return RSPT_HIP_ERR_UNSUPPORTED;
    HIPCHK(p, hipSetDevice(p->device));
    IirCoef c{};
    for (size_t i = 0; i < nr_coefficients; ++i) {
        c.n[i] = n[i];
        c.d[i] = d[i];
    }
    c.nc = (uint32_t)nr_coefficients;
    c.init_steps = 4 * init_nr_samples;
    hipStream_t st = (hipStream_t)stream;
    by_bps(p->g.bps, [&](auto bps) { launch_iir_stream_nc<decltype(bps)::value>(p, (uint8_t*)d_buf, (uint32_t)rows, c, (IirCarry*)d_state, st); });
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

// The checks of both windowed entry points, in the order they return: a null handle or buffer, nblocks == 0 or nblocks * nch
// >= 2^31, and buffers that overlap without being the same (ERR_ARG); then a chunk's row offsets, which k_fir and k_med_short
// compute in 32 bits (ERR_UNSUPPORTED: 2^24 channels and more).  Sets the geometry for the window K and whether the call is in place.
static int window_call_checks(const rspt_hip_packer* p, const void* d_src, const void* d_dst, size_t nblocks, uint32_t K, uint32_t threads,
                              uint32_t run, WinGeom* f, bool* in_place, bool one_run = false) {
    if (!p || !d_src || !d_dst || nblocks == 0 || nblocks > 0x7FFFFFFFu / (p->g.nch ? p->g.nch : 1)) return RSPT_HIP_ERR_ARG;
    const uint64_t bytes = (uint64_t)nblocks * p->g.block_bytes;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
    *in_place = s0 == d0;
    if (!*in_place && s0 < d0 + bytes && d0 < s0 + bytes) return RSPT_HIP_ERR_ARG;  // in place, or apart
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    if (one_run && (uint64_t)nblocks * p->g.ns >= kStreamMaxRows) return RSPT_HIP_ERR_UNSUPPORTED;
    *f = win_geom(p, nblocks, K, threads, run, one_run ? (uint32_t)(nblocks * p->g.ns) : 0u);
    if ((uint64_t)f->subs * run * p->g.nch * p->g.bps >= (1ull << 31)) return RSPT_HIP_ERR_UNSUPPORTED;
    return RSPT_HIP_OK;
}

// The halo of an in-place call with more than one span per block: the K - 1 rows in front of every span but the first,
// nblocks (nsplit - 1) pieces of (K - 1) rows.
static uint64_t halo_pieces(const WinGeom& f, size_t nblocks, bool in_place) {
    return in_place && f.nsplit > 1 ? (uint64_t)nblocks * (f.nsplit - 1) : 0;  // (a carried-state call: one block)
}

static hipError_t launch_halo(const WinGeom& f, const void* d_src, uint8_t* halo, uint64_t pieces, hipStream_t st) {
    const bool words = (reinterpret_cast<uintptr_t>(d_src) % 4) == 0 && (f.block_bytes % 4) == 0 && (f.stride % 4) == 0;
    const uint32_t grid = (uint32_t)(pieces < 65536 ? pieces : 65536);
    if (words) hipLaunchKernelGGL(k_fir_halo<true>, dim3(grid), dim3(256), 0, st, (const uint8_t*)d_src, halo, f, pieces);
    else hipLaunchKernelGGL(k_fir_halo<false>, dim3(grid), dim3(256), 0, st, (const uint8_t*)d_src, halo, f, pieces);
    return hipGetLastError();
}

// The end of a windowed call from the point where it has enqueued work: record `last` behind it, and report the first error.
static int finish_window_call(rspt_hip_packer* p, LastCall& last, hipError_t e, hipStream_t st) {
    const hipError_t er = last.record(st);
    if (e == hipSuccess) e = er;
    if (e != hipSuccess) {
        p->last_hip_error = (int)e;
        return RSPT_HIP_ERR_LAUNCH;
    }
    return RSPT_HIP_OK;
}

// Stage the head of a carried-state call and write the new state (k_fir_carry, fir.hip); the state: [u64 started][K - 1 rows].
static hipError_t launch_fir_carry(const WinGeom& f, const void* d_src, uint8_t* head, void* d_state, hipStream_t st) {
    uint64_t* started = (uint64_t*)d_state;
    uint8_t* rows = (uint8_t*)d_state + 8;
    const uint64_t n = (uint64_t)(f.K - 1) * f.stride;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 4096);
    if (n) hipLaunchKernelGGL(k_fir_carry<false>, dim3(grid), dim3(256), 0, st, (const uint8_t*)d_src, head, started, rows, n, f.stride, f.K, f.ns);
    hipLaunchKernelGGL(k_fir_carry<true>, dim3(grid), dim3(256), 0, st, (const uint8_t*)d_src, head, started, rows, n, f.stride, f.K, f.ns);
    return hipGetLastError();
}

// Both FIR entries: d_state == NULL is the stateless call on nblocks blocks, else the blocks are one run behind the state.
static int fir_call(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, const double* kernel, size_t kernel_size, void* d_state,
                    void* stream) {
    if (!kernel || kernel_size == 0 || kernel_size > kFirMaxTaps) return RSPT_HIP_ERR_ARG;
    WinGeom f;
    bool in_place;
    if (int rc = window_call_checks(p, d_src, d_dst, nblocks, (uint32_t)kernel_size, kFirThreads, kFirR, &f, &in_place, d_state != nullptr)) return rc;
    if (d_state) nblocks = 1;  // (the geometry's one block of nblocks * ns rows)
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    FirStage& fs = p->fir;
    const uint64_t pieces = halo_pieces(f, nblocks, in_place);
    const uint64_t halo_bytes = pieces * (uint64_t)(kernel_size - 1) * f.stride;
    const uint64_t head_bytes = d_state ? (uint64_t)(kernel_size - 1) * f.stride : 0;
    if (halo_bytes > fs.halo_cap || head_bytes > fs.head_cap) {
        fs.wait_all();  // (no earlier call may still read a buffer being replaced)
        if (halo_bytes > fs.halo_cap) {
            fs.halo_cap = 0;
            if (hipMalloc(fs.halo.out(), halo_bytes) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
            fs.halo_cap = halo_bytes;
        }
        if (head_bytes > fs.head_cap) {
            fs.head_cap = 0;
            if (hipMalloc(fs.head.out(), head_bytes) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
            fs.head_cap = head_bytes;
        }
    }
    // the coefficients: the host waits only when kSlots calls are still ahead on the device
    FirStage::CoefSlot& cs = fs.slot[fs.next];
    HIPCHK(p, cs.last.wait());
    if (cs.cap < kernel_size) {
        cs.cap = 0;
        if (hipHostMalloc((void**)cs.host.out(), kernel_size * sizeof(double), hipHostMallocDefault) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
        if (hipMalloc(cs.dev.out(), kernel_size * sizeof(double)) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
        cs.cap = kernel_size;
    }
    if (!cs.last.make_event()) return RSPT_HIP_ERR_ALLOC;
    memcpy(cs.host, kernel, kernel_size * sizeof(double));
    fs.next = (fs.next + 1) % FirStage::kSlots;
    // (from here on every path ends in finish_window_call, which records `last`: the copy below reads the page-locked slot)
    hipError_t e = hipMemcpyAsync(cs.dev, cs.host, kernel_size * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && d_state) e = launch_fir_carry(f, d_src, fs.head, d_state, st);
    if (e == hipSuccess && pieces) e = launch_halo(f, d_src, fs.halo, pieces, st);
    if (e == hipSuccess) {
        const uint32_t bps = p->g.bps;
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
        const bool aligned = (bps == 4 || bps == 2) && s0 % bps == 0 && d0 % bps == 0;  // (block_bytes is a multiple of bps)
        by_bps(bps, [&](auto b) {
            launch_fir<decltype(b)::value>(f, (const uint8_t*)d_src, (uint8_t*)d_dst, pieces ? (const uint8_t*)fs.halo : nullptr, cs.dev, aligned, st,
                                           head_bytes ? (const uint8_t*)fs.head : nullptr);
        });
        e = hipGetLastError();
    }
    return finish_window_call(p, cs.last, e, st);
}

int rspt_hip_fir_prefilter_batch_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, const double* kernel, size_t kernel_size,
                                     void* stream) {
    return fir_call(p, d_src, d_dst, nblocks, kernel, kernel_size, nullptr, stream);
}

int rspt_hip_fir_state_bytes(rspt_hip_packer* p, size_t kernel_size, size_t* bytes) {
    if (!p || !bytes || kernel_size == 0 || kernel_size > kFirMaxTaps) return RSPT_HIP_ERR_ARG;
    *bytes = 8 + (((size_t)(kernel_size - 1) * p->g.nch * p->g.bps + 7) & ~(size_t)7);
    return RSPT_HIP_OK;
}

int rspt_hip_fir_prefilter_stream_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, const double* kernel, size_t kernel_size,
                                      void* d_state, void* stream) {
    if (!d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    return fir_call(p, d_src, d_dst, nblocks, kernel, kernel_size, d_state, stream);
}

// The median stage's buffers for a call: each grows behind the stage's last call, and `last` has its event from here on.
static int median_reserve(MedianStage& ms, uint64_t halo_bytes, uint64_t head_bytes, uint64_t key_samples) {
    if (halo_bytes > ms.halo_cap || head_bytes > ms.head_cap || key_samples > ms.key_cap) {
        ms.last.wait();  // (no earlier call may still use a buffer being replaced)
        if (halo_bytes > ms.halo_cap) {
            ms.halo_cap = 0;
            if (hipMalloc(ms.halo.out(), halo_bytes) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
            ms.halo_cap = halo_bytes;
        }
        if (head_bytes > ms.head_cap) {
            ms.head_cap = 0;
            if (hipMalloc(ms.head.out(), head_bytes) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
            ms.head_cap = head_bytes;
        }
        if (key_samples > ms.key_cap) {
            ms.key_cap = 0;
            ms.rank.reset();
            ms.keys_b.reset();
            if (hipMalloc(ms.keys_a.out(), key_samples * sizeof(uint64_t)) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
            if (hipMalloc(ms.keys_b.out(), key_samples * sizeof(uint64_t)) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
            if (hipMalloc(ms.rank.out(), key_samples * sizeof(uint32_t)) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
            ms.key_cap = key_samples;
        }
    }
    return ms.last.make_event() ? RSPT_HIP_OK : RSPT_HIP_ERR_ALLOC;
}

int rspt_hip_median_filter_batch_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, size_t window, void* stream) {
    if (!p || window == 0) return RSPT_HIP_ERR_ARG;
    const Geom& g = p->g;
    const uint32_t W = (uint32_t)(window < g.ns ? window : g.ns);  // a window of ns or more is the expanding median of the channel
    WinGeom f;
    bool in_place;
    if (int rc = window_call_checks(p, d_src, d_dst, nblocks, W, kMedThreads, kMedRun, &f, &in_place)) return rc;
    if (W > kMedShortMax && g.ns > kMedMaxRanks) return RSPT_HIP_ERR_UNSUPPORTED;  // (the generic path's bitmaps live in LDS)
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    if (W == 1) {  // a copy, sample width kept
        if (in_place) return RSPT_HIP_OK;
        HIPCHK(p, hipMemcpyAsync(d_dst, d_src, (uint64_t)nblocks * g.block_bytes, hipMemcpyDeviceToDevice, st));
        return RSPT_HIP_OK;
    }
    MedianStage& ms = p->med;
    const uint32_t bps = g.bps;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
    const bool aligned = (bps == 4 || bps == 2) && s0 % bps == 0 && d0 % bps == 0;  // (block_bytes is a multiple of bps)
    const uint64_t pairs = (uint64_t)nblocks * g.nch;
    // buffers: the short path's halo, the generic path's keys and ranks for a piece of up to 2^25 samples (or one channel)
    const bool is_short = W <= kMedShortMax;
    const uint64_t pieces = is_short ? halo_pieces(f, nblocks, in_place) : 0;
    const uint64_t halo_bytes = pieces * (uint64_t)(W - 1) * f.stride;
    const uint64_t piece_pairs = is_short ? 0 : std::min<uint64_t>(pairs, std::max<uint64_t>(1, (1ull << 25) / g.ns));
    if (int rc = median_reserve(ms, halo_bytes, 0, piece_pairs * g.ns)) return rc;
    hipError_t e = hipSuccess;
    if (is_short) {
        if (pieces) e = launch_halo(f, d_src, ms.halo, pieces, st);
        if (e == hipSuccess) e = launch_med_short_w<false>(bps, f, d_src, d_dst, pieces ? (const uint8_t*)ms.halo : nullptr, aligned, st, nullptr);
    } else {
        for (uint64_t pair0 = 0; e == hipSuccess && pair0 < pairs; pair0 += piece_pairs) {
            const uint64_t np = std::min(piece_pairs, pairs - pair0);
            e = by_bps(bps, [&](auto bb) {
                return launch_med_generic<decltype(bb)::value>(p, f, (const uint8_t*)d_src, (uint8_t*)d_dst, pair0, np, aligned, st);
            });
        }
    }
    return finish_window_call(p, ms.last, e, st);
}

int rspt_hip_median_state_bytes(rspt_hip_packer* p, size_t window, size_t* bytes) {
    if (!p || !bytes || window == 0) return RSPT_HIP_ERR_ARG;
    if (window > kMedShortMax && window - 1 > kMedMaxCarry) return RSPT_HIP_ERR_UNSUPPORTED;
    *bytes = 8 + (((size_t)(window - 1) * p->g.nch * p->g.bps + 7) & ~(size_t)7);
    return RSPT_HIP_OK;
}

// Stage the old state in the handle's head buffer and write the new one (k_med_carry, median.hip): in words where every
// address and length is a multiple of 4.
static hipError_t launch_med_carry(const WinGeom& f, const void* d_src, uint8_t* head, void* d_state, uint64_t rows, hipStream_t st) {
    uint64_t n = (uint64_t)(f.K - 1) * f.stride, call = rows * f.stride;
    const bool words = reinterpret_cast<uintptr_t>(d_src) % 4 == 0 && f.stride % 4 == 0;
    if (words) n /= 4, call /= 4;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 4096);
    uint8_t* state = (uint8_t*)d_state;
    if (words) {
        hipLaunchKernelGGL((k_med_carry<false, uint32_t>), dim3(grid), dim3(256), 0, st, (const uint32_t*)d_src, head, state, n, call, f.K - 1, rows);
        hipLaunchKernelGGL((k_med_carry<true, uint32_t>), dim3(grid), dim3(256), 0, st, (const uint32_t*)d_src, head, state, n, call, f.K - 1, rows);
    } else {
        hipLaunchKernelGGL((k_med_carry<false, uint8_t>), dim3(grid), dim3(256), 0, st, (const uint8_t*)d_src, head, state, n, call, f.K - 1, rows);
        hipLaunchKernelGGL((k_med_carry<true, uint8_t>), dim3(grid), dim3(256), 0, st, (const uint8_t*)d_src, head, state, n, call, f.K - 1, rows);
    }
    return hipGetLastError();
}

// The segment capacity S = W - 1 + L of a carried-state call of the generic path: 8 (W - 1) rounded up to 2^16, 2^17 or 2^18 --
// at most one row in eight is sorted twice up to W - 1 = 2^15, one in two at the limit W - 1 = 2^17 -- and never more than the
// call needs (one segment of W - 1 + N rows).  2^16 is the channel length the stateless path is measured at:
// shorter segments save merge passes but pay a bitmap clear and W set bits per 1024 outputs more often than they save.
static uint32_t median_segment_rows(uint32_t W, uint64_t rows) {
    const uint64_t want = 8ull * (W - 1);
    const uint64_t S = want <= (1u << 16) ? (1u << 16) : want <= (1u << 17) ? (1u << 17) : kMedMaxRanks;
    return (uint32_t)std::min<uint64_t>(S, (uint64_t)(W - 1) + rows);
}

int rspt_hip_median_filter_stream_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, size_t window, void* d_state, void* stream) {
    if (!p || window == 0 || !d_state || reinterpret_cast<uintptr_t>(d_state) % 8) return RSPT_HIP_ERR_ARG;
    const Geom& g = p->g;
    const uint32_t W = (uint32_t)std::min<size_t>(window, (size_t)kMedMaxCarry + 2);  // (not clamped to ns: the window is the recording's)
    WinGeom f;
    bool in_place;
    if (int rc = window_call_checks(p, d_src, d_dst, nblocks, W, kMedThreads, kMedRun, &f, &in_place, true)) return rc;
    if (W > kMedShortMax && W - 1 > kMedMaxCarry) return RSPT_HIP_ERR_UNSUPPORTED;  // (at least half of every segment is new rows)
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const uint64_t rows = (uint64_t)nblocks * g.ns;  // (below 2^31 - 2^17: window_call_checks)
    if (W == 1) {  // a copy; the state is its header and stays zero
        if (in_place) return RSPT_HIP_OK;
        HIPCHK(p, hipMemcpyAsync(d_dst, d_src, rows * f.stride, hipMemcpyDeviceToDevice, st));
        return RSPT_HIP_OK;
    }
    MedianStage& ms = p->med;
    const uint32_t bps = g.bps;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_src), d0 = reinterpret_cast<uintptr_t>(d_dst);
    const bool aligned = (bps == 4 || bps == 2) && s0 % bps == 0 && d0 % bps == 0;
    const bool is_short = W <= kMedShortMax;
    const uint64_t pieces = is_short ? halo_pieces(f, 1, in_place) : 0;
    const uint64_t halo_bytes = pieces * (uint64_t)(W - 1) * f.stride;
    const uint64_t head_bytes = 8 + (uint64_t)(W - 1) * f.stride;
    // generic: (segment, channel) items of S keys each, in pieces of up to 2^25 keys
    MedSeg sg{};
    WinGeom fg = f;
    uint64_t items = 0, piece_items = 0;
    if (!is_short) {
        const uint32_t S = median_segment_rows(W, rows);
        sg.L = S - (W - 1);
        sg.nseg = (uint32_t)((rows + sg.L - 1) / sg.L);
        sg.N = (uint32_t)rows;
        fg.ns = S;
        items = (uint64_t)sg.nseg * g.nch;
        piece_items = std::min<uint64_t>(items, std::max<uint64_t>(1, (1ull << 25) / S));
    }
    if (int rc = median_reserve(ms, halo_bytes, head_bytes, piece_items * fg.ns)) return rc;
    sg.head = ms.head;
    // the new state is written from d_src before any kernel stores to d_dst
    hipError_t e = launch_med_carry(f, d_src, ms.head, d_state, rows, st);
    if (is_short) {
        if (e == hipSuccess && pieces) e = launch_halo(f, d_src, ms.halo, pieces, st);
        if (e == hipSuccess) e = launch_med_short_w<true>(bps, f, d_src, d_dst, pieces ? (const uint8_t*)ms.halo : nullptr, aligned, st, ms.head);
    } else {
        // from the last segment to the first: a walk writes its segment's new rows, which no segment sorted later reads
        for (uint64_t item0 = 0; e == hipSuccess && item0 < items; item0 += piece_items) {
            const uint64_t ni = std::min(piece_items, items - item0);
            e = by_bps(bps, [&](auto bb) {
                return launch_med_generic<decltype(bb)::value, true>(p, fg, (const uint8_t*)d_src, (uint8_t*)d_dst, item0, ni, aligned, st, sg);
            });
        }
    }
    return finish_window_call(p, ms.last, e, st);
}

// ---- PRDN: the quality figure of the reference's harness (quality.hip) -----------------------------------------------------------
// The decomposition of the two streaming passes for the widest load the buffers' alignment allows.
static QGeom quality_geom(const rspt_hip_packer* p, size_t nblocks, int W) {
    const Geom& g = p->g;
    QGeom q{};
    q.block_bytes = g.block_bytes;
    q.nch = g.nch, q.ns = g.ns, q.be = g.be;
    const uint32_t nw = W == 0 ? 1u : (g.bps == 3 ? 3u : 1u) * (uint32_t)W;
    const uint32_t vs = W == 0 ? 1u : nw * 4u / g.bps;  // samples of a load group
    uint32_t a = g.nch, b = vs;
    while (b) {
        const uint32_t t = a % b;
        a = b, b = t;
    }
    q.rows = vs / a;  // the fewest rows that hold whole groups
    const uint64_t qps = (uint64_t)q.rows * g.nch / vs;
    q.qps = (uint32_t)qps;
    q.nsub = qps < kQThreads ? kQThreads / q.qps : 1u;
    q.ncg = (uint32_t)((qps + kQThreads - 1) / kQThreads);
    q.nsr = g.ns / q.rows;
    const uint64_t sweeps = ((uint64_t)q.nsr + q.nsub - 1) / q.nsub;
    // workgroups: about 4096 in all where the blocks are long enough to give each at least 8 sweeps
    uint64_t nsplit = std::min<uint64_t>(std::max<uint64_t>(1, sweeps / 8), (4096 + nblocks * q.ncg - 1) / (nblocks * q.ncg));
    q.span = (uint32_t)std::max<uint64_t>(1, (sweeps + nsplit - 1) / nsplit) * q.nsub;
    q.nsplit = (uint32_t)std::max<uint64_t>(1, ((uint64_t)q.nsr + q.span - 1) / q.span);
    return q;
}

int rspt_hip_prdn_batch_dev(rspt_hip_packer* p, const void* d_orig, const void* d_dec, size_t nblocks, double* d_prdn, double* d_mse, double* d_ref,
                            uint32_t* d_path, void* stream) {
    if (!p || !d_orig || !d_dec || !d_prdn || nblocks == 0 || nblocks > 0x7FFFFFFFu / (p->g.nch ? p->g.nch : 1)) return RSPT_HIP_ERR_ARG;
    if (p->feed) return RSPT_HIP_ERR_ARG;  // (the feed owns the handle's workspace until rspt_hip_feed_end)
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    const Geom& g = p->g;
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_orig), d0 = reinterpret_cast<uintptr_t>(d_dec);
    auto aligned = [&](uintptr_t m) { return o0 % m == 0 && d0 % m == 0 && (nblocks == 1 || g.block_bytes % m == 0); };
    const int W = aligned(16) ? 4 : aligned(4) ? 1 : 0;
    QGeom q = quality_geom(p, nblocks, W);
    q.aligned4 = aligned(4) ? 1u : 0u;
    const uint64_t units = (uint64_t)nblocks * q.ncg * q.nsplit;
    if (units >= (1ull << 31) || (uint64_t)q.rows * g.nch >= (1ull << 32)) return RSPT_HIP_ERR_UNSUPPORTED;
    if (int rc = rspt_hip_reserve(p, nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = (hipStream_t)stream;
    const uint32_t B = (uint32_t)nblocks;
    unsigned long long* sums = p->ws.quality;
    unsigned long long* acc = sums + (size_t)B * g.nch;
    uint32_t* flag = reinterpret_cast<uint32_t*>(acc + (size_t)B * 4);
    HIPCHK(p, hipMemsetAsync(sums, 0, ((size_t)B * g.nch + (size_t)B * 4) * sizeof(unsigned long long), st));
    const uint8_t* o = (const uint8_t*)d_orig;
    const uint8_t* d = (const uint8_t*)d_dec;
    by_bps(g.bps, [&](auto bb) {
        constexpr int BPS = decltype(bb)::value;
        auto go = [&](auto ww) {
            constexpr int WW = decltype(ww)::value;
            hipLaunchKernelGGL((k_q_sums<BPS, WW>), dim3((uint32_t)units), dim3(kQThreads), 0, st, o, q, sums);
            hipLaunchKernelGGL((k_q_accum<BPS, WW>), dim3((uint32_t)units), dim3(kQThreads), 0, st, o, d, q, (const long long*)sums, acc);
        };
        if (W == 4) go(std::integral_constant<int, 4>());
        else if (W == 1) go(std::integral_constant<int, 1>());
        else go(std::integral_constant<int, 0>());
        hipLaunchKernelGGL(k_q_finish, dim3((B + 255) / 256), dim3(256), 0, st, (const unsigned long long*)acc, B, flag, d_prdn, d_mse, d_ref, d_path);
        hipLaunchKernelGGL(k_q_seq<BPS>, dim3(B), dim3(kQThreads), 0, st, o, d, q, (const long long*)sums, (const unsigned long long*)acc,
                           (const uint32_t*)flag, d_prdn, d_mse, d_ref);
    });
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

// ---- native <-> planar int32 (the reference's convert_native_to_i32 / convert_i32_to_native, utils.cpp:51-191) -------------------
// The checks of both entries.  Nothing of the handle but its shape and byte order is used: no workspace, no allocation.
static int convert_checks(const rspt_hip_packer* p, const void* d_native, const void* d_planar, size_t nblocks) {
    if (!p || !d_native || !d_planar || nblocks == 0 || nblocks > 65535) return RSPT_HIP_ERR_ARG;  // (65535: grid.z, as rspt_hip_reserve)
    const Geom& g = p->g;
    if ((uint64_t)nblocks * g.nch >= (1ull << 31)) return RSPT_HIP_ERR_ARG;
    const uintptr_t n0 = reinterpret_cast<uintptr_t>(d_native), p0 = reinterpret_cast<uintptr_t>(d_planar);
    if (p0 & 3u) return RSPT_HIP_ERR_ARG;
    const uint64_t nbytes = (uint64_t)nblocks * g.block_bytes, pbytes = (uint64_t)nblocks * g.N * sizeof(int32_t);
    if (n0 < p0 + pbytes && p0 < n0 + nbytes) return RSPT_HIP_ERR_ARG;  // the two buffers overlap
    return RSPT_HIP_OK;
}

// Narrow handles with a 16-byte aligned native buffer take the tile kernels of the packers' own front end and inverse; wide ones,
// and native buffers at any other address, the 64 x 64 transposes k_wide_planar / k_wide_native.
static bool convert_i32x4_ok(const Geom& g, const void* d_planar) {
    return g.bps == 4 && (g.nch & 3) == 0 && (g.ns & 3) == 0 && g.nch <= 1024 && (reinterpret_cast<uintptr_t>(d_planar) & 15) == 0;
}

int rspt_hip_native_to_i32_batch_dev(rspt_hip_packer* p, const void* d_native, int32_t* d_planar, size_t nblocks, void* stream) {
    if (int rc = convert_checks(p, d_native, d_planar, nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    const Geom& g = p->g;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t* src = (const uint8_t*)d_native;
    const unsigned B = (unsigned)nblocks;
    if (!p->wide && (reinterpret_cast<uintptr_t>(d_native) & 15) == 0) {
        if (convert_i32x4_ok(g, d_planar)) {
            const uint32_t T4 = tile_i32x4(g);
            hipLaunchKernelGGL(k_tile_planar_i32x4, dim3((g.ns + T4 - 1) / T4, B), dim3(256), g.nch * (T4 + 1) * 4, st, src, g, T4, d_planar,
                               (long long*)nullptr);
        } else {
            by_bps(g.bps, [&](auto bps) {
                constexpr int BPS = decltype(bps)::value;
                if (!p->conv_lds_raised) {  // (once per handle: a handle has one sample width)
                    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tile_planar<BPS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p->in_lds) != hipSuccess) return;
                    p->conv_lds_raised = true;
                }
                hipLaunchKernelGGL((k_tile_planar<BPS>), dim3((g.ns + p->T - 1) / p->T, B), dim3(256), p->in_lds, st, src, g, p->T, d_planar);
            });
        }
    } else {
        by_bps(g.bps, [&](auto bps) {
            hipLaunchKernelGGL(k_wide_planar<decltype(bps)::value>, dim3((g.ns + 63) / 64, (g.nch + 63) / 64, B), dim3(256), 0, st, src, g, d_planar);
        });
    }
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_i32_to_native_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, void* d_native, size_t nblocks, void* stream) {
    if (int rc = convert_checks(p, d_native, d_planar, nblocks)) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    const Geom& g = p->g;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* dst = (uint8_t*)d_native;
    const unsigned B = (unsigned)nblocks;
    // k_planar_native divides per element and stores int8 / int16 / int24 byte by byte: it keeps only the handles of fewer than 32
    // channels, where more than half of k_wide_native's 64-channel tile would be empty.
    const bool narrow = !p->wide && p->Tn_native && (reinterpret_cast<uintptr_t>(d_native) & 15) == 0;
    if (narrow && (convert_i32x4_ok(g, d_planar) || g.nch < 32)) {
        if (convert_i32x4_ok(g, d_planar)) {
            const uint32_t T4 = tile_i32x4(g);
            hipLaunchKernelGGL(k_planar_native_i32x4, dim3((g.ns + T4 - 1) / T4, B), dim3(256), g.nch * (T4 + 1) * 4, st, d_planar, g, T4, dst);
        } else {
            const uint32_t T = min(p->Tn_native, g.ns);
            by_bps(g.bps, [&](auto bps) {
                hipLaunchKernelGGL((k_planar_native<decltype(bps)::value>), dim3((g.ns + T - 1) / T, B), dim3(256), g.nch * (T + 1) * 4, st, d_planar, g, T,
                                   dst);
            });
        }
    } else {
        by_bps(g.bps, [&](auto bps) { launch_wide_native<decltype(bps)::value>(g, d_planar, dst, B, st); });
    }
    HIPCHK(p, hipGetLastError());
    return RSPT_HIP_OK;
}

int rspt_hip_design_iir(int type, int order, double sampling_rate, double cutoff_low, double cutoff_high, double* num, double* den,
                        size_t* nr_coefficients) {
    if (!num || !den || !nr_coefficients) return RSPT_HIP_ERR_ARG;
    double n[5], d[5];
    const int nc = design_iir(type, order, sampling_rate, cutoff_low, cutoff_high, n, d);
    if (nc == 0) return RSPT_HIP_ERR_ARG;
    for (int i = 0; i < nc; ++i) {
        num[i] = n[i];
        den[i] = d[i];
    }
    *nr_coefficients = (size_t)nc;
    return RSPT_HIP_OK;
}

int rspt_hip_peak_state_bytes(rspt_hip_packer* p, size_t* bytes) {
    if (!p || !bytes) return RSPT_HIP_ERR_ARG;
    *bytes = (size_t)p->g.nch * kPeakStateBytesPerChannel;
    return RSPT_HIP_OK;
}

int rspt_hip_peak_detect_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, int variant, double sampling_rate, double marker_val,
                                   void* d_state, uint32_t* d_count, int32_t* d_index, double* d_value, size_t max_peaks, double* d_sig,
                                   double* d_threshold, void* stream) {
    PeakArgs a{};
    PeakCoef c{};
    if (variant < kPeakOnline || variant > kPeakOfflineFw ||
        !peak_args(p, d_src, nblocks, sampling_rate, d_state, d_count, d_index, d_value, max_peaks, d_sig, d_threshold, a) ||
        !peak_coef(variant, sampling_rate, marker_val, c))
        return RSPT_HIP_ERR_ARG;
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    return by_bps(p->g.bps, [&](auto bb) {
        constexpr int B = decltype(bb)::value;
        auto go = [&](auto vv) {
            constexpr int V = decltype(vv)::value;
            return peak_launch(p, d_sig ? &k_peak<B, V, true> : &k_peak<B, V, false>, a, c, stream);
        };
        if (variant == kPeakOnline) return go(std::integral_constant<int, kPeakOnline>());
        if (variant == kPeakOnline1st) return go(std::integral_constant<int, kPeakOnline1st>());
        return go(std::integral_constant<int, kPeakOfflineFw>());
    });
}

int rspt_hip_peak_offline_work_bytes(rspt_hip_packer* p, size_t nblocks, int stateful, size_t* bytes) {
    if (!p || !bytes || nblocks == 0) return RSPT_HIP_ERR_ARG;
    const Geom& g = p->g;
    if ((uint64_t)nblocks * g.nch >= (1ull << 31)) return RSPT_HIP_ERR_ARG;
    const uint64_t lanes = stateful ? g.nch : (uint64_t)nblocks * g.nch;
    *bytes = (size_t)(((lanes + 63) / 64) * kPeakOffSlabBytesPerSample * g.ns);
    return RSPT_HIP_OK;
}

int rspt_hip_peak_detect_offline_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, double sampling_rate, double marker_val,
                                           void* d_state, void* d_work, uint32_t* d_count, int32_t* d_index, double* d_value,
                                           size_t max_peaks, double* d_sig, double* d_threshold, void* stream) {
    PeakOffArgs a{};
    PeakOffCoef k{};
    if (!d_work || ((uintptr_t)d_work % 8) != 0 ||
        !peak_args(p, d_src, nblocks, sampling_rate, d_state, d_count, d_index, d_value, max_peaks, d_sig, d_threshold, a) ||
        !peak_coef(kPeakOfflineFw, sampling_rate, marker_val, k.c))
        return RSPT_HIP_ERR_ARG;
    if (stage_too_wide(p)) return RSPT_HIP_ERR_UNSUPPORTED;
    // the reference's undefined cases: nr_slope_samples 0 (the shift runs every event off the end of the array) and a block
    // shorter than the relocation radius (the unsigned bound len - radius wraps)
    k.radius = (int32_t)((10.0 * sampling_rate) / 1000.0);
    if (k.c.nslope == 0 || (uint64_t)a.ns < (uint64_t)k.radius) return RSPT_HIP_ERR_ARG;
    // peak_detector_offline's constructor adds the baseline: a 0.5 Hz first-order low-pass
    if (!design_iir(kFiltLowPass, 1, sampling_rate, 0.5, 0.0, k.lf, k.lb)) return RSPT_HIP_ERR_ARG;
    a.work = (uint8_t*)d_work;
    return by_bps(p->g.bps, [&](auto bb) {
        constexpr int B = decltype(bb)::value;
        return peak_launch(p, d_sig ? &k_peak_offline<B, true> : &k_peak_offline<B, false>, a, k, stream);
    });
}

// ---- multi-GPU gather over RCCL.  RCCL is bound at run time: a process that never gathers (the C++ drop-in on one
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

}  // extern "C"
