// host_handle.hpp -- the handle behind the C ABI: the owners of its HIP resources, its parts, and the helpers every host file uses.
// Included by rspt_hip.hip behind the kernels.
#pragma once

namespace {
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
    Dev<unsigned long long> quality;  // [cap][quality_words(nch)]: the PRDN entries' scratch, carved up per call by QScratch
    // the lossy packers only (a ladder needs one):
    Dev<uint32_t> idx_choice;   // [cap] the choices of a container's index (k_index_choices -> the ladder kernels of the packed decoders)
    Dev<uint64_t> pack_sizes;   // [cap] rspt_hip_pack_batch_choice_dev: the sizes k_pack_index reads (k_pack_choice_sizes)
    Dev<uint8_t> target_tab;    // rate_work::Tables of [kMaxLadder][cap] cells: the figures of rspt_hip_compress_target_planar_batch_dev
};

// The PRDN scratch of a call on B blocks: [B][nch] int64 channel sums | [B][4] per-block accumulators | [B] u32 flags, each part
// right behind the one before it; the first two (clear_bytes) are zeroed by one memset in front of the call's kernels.
constexpr size_t quality_words(size_t nch) { return nch + 4 + 1; }  // 64-bit words per block (a flag leaves half of its word unused)
struct QScratch {
    unsigned long long *sums, *acc;
    uint32_t* flag;
    size_t clear_bytes;
    QScratch(unsigned long long* base, size_t B, size_t nch)
        : sums(base), acc(base + B * nch), flag(reinterpret_cast<uint32_t*>(acc + B * 4)), clear_bytes(B * (nch + 4) * sizeof(unsigned long long)) {}
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

// A device buffer of a windowed stage (FIR, median) that only grows.  The caller has waited for the stage's last call before
// grow() replaces the buffer; a failed grow() leaves it empty.
namespace {
struct StageBuf {
    Dev<uint8_t> mem;
    size_t cap = 0;
    int grow(size_t bytes) {
        cap = 0;
        if (hipMalloc(mem.out(), bytes) != hipSuccess) return RSPT_HIP_ERR_ALLOC;
        cap = bytes;
        return RSPT_HIP_OK;
    }
    operator uint8_t*() const { return mem; }
};
}  // namespace

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
    StageBuf halo, head;
    void wait_all() {
        for (CoefSlot& s : slot) s.last.wait();
    }
};

// rspt_hip_median_filter_batch_dev: the halo rows of an in-place short-window call, and the sort buffers of the generic path
// (two key buffers and the ranks of one piece of the batch), all behind the stage's last call.
// rspt_hip_median_filter_stream_dev adds `head`, the staged copy of a carried-state call's old state, under the same rule.
// The planar entries (rspt_hip_median_filter_planar_batch_dev / _stream_dev) use the same buffers: `halo` holds the fronts of the
// short path (the W - 1 samples in front of a span, k_firp_front), `head` the staged state, the keys and ranks the generic path's.
struct MedianStage {
    StageBuf halo, head;
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
    // the quantiser of the lossy packers (rspt_hip_set_quantizer): the reference's `quality` constant (signal_packer_dct.cpp:39,
    // signal_packer_hadamard.cpp:37); their plane count, nr_bytes_to_compress_, is nb_host / nb_state.  hadamard other than
    // quality 1 takes the kernels with the fp64 division (transforms.hip: QUANT) by n / quality forward, by quality inverse
    double quality = 0;
    bool had_quant = false;
    double had_div_fwd = 0, had_div_inv = 0;
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
    uint32_t rate_route[3] = {0, 0, 0};  // rspt_hip_debug_set_{target,budget,total}_route (RateRule): 0 = the host's choice, 1 = the general route, 2 = the faster one
    uint32_t qp_form = 0; // RSPT_QP_FORM (diagnostic builds only): planar PRDN form; 0 = the host's choice, 1 = split, 2 = whole rows
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
