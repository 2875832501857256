// hzr_kernels.hip -- the hzr block codec (RLE of zero runs + per-block Huffman,
// LSB-first bit stream, CRC-32C) as gfx950 kernels.  Bit-exact with
// lib_hzr/hzr_encode.c; the parallel formulations are modelled and checked on
// the CPU in tools/kernel_model.py + tests/test_kernel_model.py.
//
//   k_hist    persistent 1024-thread workgroups, one hzr block at a time: zero-run tokenizer
//             (hzr_encode.c:133-173) on 16-byte granules; per-wave 261-bin histograms -> block histogram,
//             per-segment histograms and the zero-run context of every granule (for k_tree / k_encode)
//   k_tree    one wave per hzr block: Fill test (:285-305), Huffman tree with
//             the reference's tie-break (:222-283), codes + pre-order tree
//             description (:177-219), exact payload size -> block mode (:377-469),
//             stream bit at which each 4 KiB segment's tokens start.  A small hzr block (few non-zero
//             segments, tokens, payload bytes) is also encoded here, by the wave that built its code
//             table: header + payload go to the block's staging slot (stage_small_block)
//   k_layout  one workgroup per block: sizes -> stream offsets, stream framing
//             (signal_packer_base.cpp:69-95, hzr_encode.c:521-522), work queue
//   k_encode  persistent 1024-thread workgroups: first the staged small blocks are copied to their
//             place in the streams, then one big hzr block at a time: one pass from
//             lookup to an LDS image of the payload (:410-457), parallel CRC-32C
//             (hzr_crc32c.c:77-84), block header (:475-481), coalesced copy-out
//   k_pack_*  the streams of a batch as one container (rspt_hip_pack_batch_dev)
#include "common.hpp"

namespace rspt {

// ===========================================================================
// shared: load the 4 granules a lane owns and chain the zero runs across the
// workgroup.  Wave w owns bytes [4096w, 4096w+4096) of the hzr block as 4 rows
// of 1 KiB; lane l of row r owns the granule at 4096w + 1024r + 16l, so every
// global load is a fully coalesced 1 KiB wave access.
// ===========================================================================
// threadIdx.x behind an empty asm: inside the persistent loops this keeps everything derived
// from the thread id (lane masks, offsets) loop-VARIANT, so hipcc recomputes it per block instead
// of hoisting it out of the loop and holding it in VGPRs across the register-tight emit pass
// (k_hist: 20 -> 0 bytes of scratch, k_encode: 188 -> ~100).
__device__ __forceinline__ uint32_t thread_id() {
    uint32_t t = threadIdx.x;
    asm volatile("" : "+v"(t));
    return t;
}

// byte i (dynamic) of a granule held in four registers
__device__ __forceinline__ uint32_t granule_byte_dyn(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t i) {
    const uint32_t lo = (i & 8u) ? w2 : w0, hi = (i & 8u) ? w3 : w1;
    return __builtin_amdgcn_perm(hi, lo, 0x0C0C0C00u | (i & 7u));  // byte (i & 7) of {hi,lo}, zero-extended
}

// "Small" hzr blocks -- few non-zero 4 KiB segments -- are tokenized by ONE wave, segment by segment, instead of
// by a 1024-thread workgroup: their histogram is taken inside k_tree (k_hist skips them) and, if they
// also have few tokens and a small payload, the same wave encodes them right there (kModeStaged).
// Clean-block invariant (rspt_hip_packer::plane_dirty): a Huffman block with at most this many tokens has its non-zero
// granules wiped by the encoder that read it; k_layout flags every other block that holds a non-zero byte as dirty.
// (Every small block qualifies: kSmallTokens <= kWipeTokens.)
constexpr uint32_t kWipeTokens = 2048;
__device__ __forceinline__ bool block_is_wiped(const BlockMeta& m) {
    return m.mode == kModeStaged || (m.mode == kModeHuff && m.fill <= kWipeTokens);
}
constexpr uint32_t kSmallSegments = 2;    // non-zero 4 KiB segments (each costs one dependent HBM round trip)
constexpr uint32_t kSmallTokens = 512;    // tokens
constexpr uint32_t kSmallPayload = 3072;  // bytes; the wave's LDS holds the code table, X + payload + read slack
static_assert(kStageSlotWords * 4 >= 7 + kSmallPayload + 4 + 4, "staging slot too small");

struct WorkQueues {
    uint32_t n_big;     // filled by k_layout
    uint32_t next_big;  // consumed by k_encode
};

// Work distribution for k_hist / k_encode.  The hardware places workgroup i on XCD i % 8 and,
// inside the XCD, walks the CUs round-robin; a grid in which heavy (plane 0) and light
// workgroups alternate with a period that divides 256 parks the heavy ones on a fraction of
// the CUs (measured: 117 of 512 slots busy, profiles/r01_notes.md).  So both kernels are
// persistent: 2 workgroups per CU pull hzr-block indices from a counter until none are left.
struct WorkItem {
    uint32_t b, k, j;
};
__device__ __forceinline__ bool next_work(uint32_t* counter, uint32_t total, const Geom& g, uint32_t* s_slot, WorkItem& wi, uint32_t pass) {
    __syncthreads();  // everyone is done with the previous block (and with *s_slot)
    if (threadIdx.x == 0) *s_slot = pass == 0 ? blockIdx.x : gridDim.x + atomicAdd(counter, 1u);  // first item static
    __syncthreads();
    const uint32_t v = *s_slot;
    if (v >= total) return false;
    wi.k = v % kMaxPlanes;  // plane fastest
    wi.j = (v / kMaxPlanes) % g.nblk;
    wi.b = v / (kMaxPlanes * g.nblk);
    return true;
}

constexpr uint32_t kSegHistStride = kEncWaves * kSymStride;  // u16 elements per hzr block (hzr_rows.hip: k_hist)

// ===========================================================================
// shared: sparse data as entry lists -- the tokenizer of k_hist's sparse segments, of k_encode's sparse rows and of k_tree's
// small blocks, and the emit from such entries (k_encode's list blocks, k_tree's staged blocks)
// ===========================================================================
constexpr uint32_t kRunClsEntries = 280;  // lengths 0..278 and ">= 279" (hzr_internal.h:117-121)
__device__ __forceinline__ uint32_t run_class_entry(uint32_t z) {
    const uint32_t sym = run_symbol(z);
    const uint32_t base = sym == 257 ? 3u : sym == 258 ? 7u : sym == 259 ? 23u : sym == 260 ? 279u : z;  // (runs of 1 and 2: no extra bits, value 0)
    return sym | (run_extra_bits(sym) << 12) | (base << 16);
}

// OR a string of `len` <= 64 bits (hi:lo) into the image at bit `pos`.  Two words always; the third only where some lane's
// string reaches into it -- with the usual four codes of ~5.5 bits per string that is no lane of the wave, and the third
// atomic with its shifts and address is one instruction in eight of the dense emit (one wave-wide test instead)
__device__ __forceinline__ void or_bits64(uint32_t* stage, uint32_t pos, uint32_t lo, uint32_t hi, uint32_t len) {
    const uint32_t word = pos >> 5, sh = pos & 31u;
    const uint64_t sv = (((uint64_t)hi << 32) | lo) << sh;
    atomicOr(&stage[word], (uint32_t)sv);
    atomicOr(&stage[(word + 1)], (uint32_t)(sv >> 32));
    if (__builtin_amdgcn_ballot_w64(sh + len > 64u)) atomicOr(&stage[(word + 2)], (hi >> 1) >> (31u - sh));
}

// OR one token (<= 38 bits) into the image at bit `pos`
__device__ __forceinline__ void or_token(uint32_t* stage, uint32_t pos, uint32_t lo, uint32_t hi, uint32_t len) {
    const uint32_t word = pos >> 5, sh = pos & 31u;
    const uint64_t sv = (((uint64_t)hi << 32) | lo) << sh;
    atomicOr(&stage[word], (uint32_t)sv);
    atomicOr(&stage[(word + 1)], (uint32_t)(sv >> 32));
    if (sh + len > 64) atomicOr(&stage[(word + 2)], (hi >> 1) >> (31u - sh));
}

constexpr uint32_t kQueueEntries = 512;  // entries per wave in the sparse-row queue (8 x 64)

// trailing (highest-address) zero bytes of a granule that is not all zero
__device__ __forceinline__ uint32_t trail_zero_bytes(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    return w3 ? ((uint32_t)__clz((int)w3) >> 3) : w2 ? 4u + ((uint32_t)__clz((int)w2) >> 3) : w1 ? 8u + ((uint32_t)__clz((int)w1) >> 3)
                                                                                             : 12u + ((uint32_t)__clz((int)w0) >> 3);
}
__device__ __forceinline__ uint32_t zero_mask16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    return zero_nibble(w0) | (zero_nibble(w1) << 4) | (zero_nibble(w2) << 8) | (zero_nibble(w3) << 12);
}

// full kRunCap tokens in a run of R <= 65536 zeros.  Almost never any: the three compares sit behind one wave-wide test.
__device__ __forceinline__ uint32_t run_caps(uint32_t R) {
    uint32_t q = 0;
    if (__builtin_amdgcn_ballot_w64(R >= kRunCap)) q = (R >= kRunCap) + (R >= 2 * kRunCap) + (R >= 3 * kRunCap);
    return q;
}

__device__ __forceinline__ void hist_run(uint32_t* h, const uint32_t* runcls, uint32_t R) {
    const uint32_t q = run_caps(R);
    const uint32_t rem = R - q * kRunCap;
    if (q) atomicAdd(&h[260], q);
    if (rem) atomicAdd(&h[runcls[min(rem, kRunClsEntries - 1u)] & 0xFFFu], 1u);
}

// The code table of the emit helpers is anything that answers tab[index] with {code, length}: k_encode's uint2 table in LDS,
// or the packed words k_tree keeps (PackedCodes, below).

// the remainder token of a run (0 < rem < 16662) as a bit string
template <class Tab>
__device__ __forceinline__ void run_token(Tab tab, const uint32_t* runcls, uint32_t rem, uint64_t& v, uint32_t& len) {
    const uint32_t e = runcls[min(rem, kRunClsEntries - 1u)];
    const uint2 cw = tab[e & 0xFFFu];
    v = (uint64_t)cw.x | ((uint64_t)(rem - (e >> 16)) << cw.y);
    len = cw.y + ((e >> 12) & 0xFu);
}

// OR the tokens of a zero run into the image at bit `pos`; returns the bits written
template <class Tab>
__device__ __forceinline__ uint32_t emit_run(uint32_t* stage, Tab tab, const uint32_t* runcls, uint32_t pos, uint32_t R) {
    const uint32_t q = run_caps(R);
    const uint32_t rem = R - q * kRunCap;
    uint32_t done = 0;
    if (q) {
        const uint2 c = tab[260];
        const uint64_t v = (uint64_t)c.x | ((uint64_t)(kRunCap - 279u) << c.y);
        for (uint32_t i = 0; i < q; ++i) {
            or_token(stage, pos + done, (uint32_t)v, (uint32_t)(v >> 32), c.y + 14u);
            done += c.y + 14u;
        }
    }
    if (rem) {
        uint64_t v;
        uint32_t len;
        run_token(tab, runcls, rem, v, len);
        or_token(stage, pos + done, (uint32_t)v, (uint32_t)(v >> 32), len);
        done += len;
    }
    return done;
}

// what a row needs to know about its surroundings (wave-uniform)
struct RowCtx {
    uint32_t zb0;    // zeros immediately before the row's first byte (cut at the block start)
    uint32_t last;   // 1: the block ends with this row's last valid byte
    uint32_t valid;  // bytes of this row inside the block (0..1024)
    uint32_t rb;     // position of the row's first byte in the block
};

// rotate the rows through W[0] / rc[0]: the row bodies exist once in the instruction stream; four turns put everything back
__device__ __forceinline__ void rotate_rows(uint32_t (&W)[4][4], RowCtx (&rc)[4]) {
    const uint32_t t0 = W[0][0], t1 = W[0][1], t2 = W[0][2], t3 = W[0][3];
    const RowCtx tc = rc[0];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        W[q][0] = W[q + 1][0];
        W[q][1] = W[q + 1][1];
        W[q][2] = W[q + 1][2];
        W[q][3] = W[q + 1][3];
        rc[q] = rc[q + 1];
    }
    W[3][0] = t0;
    W[3][1] = t1;
    W[3][2] = t2;
    W[3][3] = t3;
    rc[3] = tc;
}

// Sparse rows: the row's literals, in order, as (position, value) entries in a per-wave queue; the wave then takes the
// queue 64 entries at a time -- the run in front of a literal is the gap to the entry before it, so nothing has to be
// chained from lane to lane.  A row that ends the block appends a virtual entry at in_size (the run that reaches the end).
constexpr uint32_t kNoLit = 0x100u;

// the lane's non-zero bytes (bit i = byte i) -- bytes behind the block end were masked to zero at the load
__device__ __forceinline__ uint32_t lane_lits(const uint32_t (&w)[4]) { return ~zero_mask16(w[0], w[1], w[2], w[3]) & 0xFFFFu; }

// fills the queue; returns the number of entries (0: nothing ends in this row)
__device__ __forceinline__ uint32_t sparse_queue(const uint32_t (&w)[4], const RowCtx& rc, uint32_t in_size, uint32_t lits, uint32_t* queue,
                                                 bool& queued) {
    const uint32_t l = lane_id();
    const uint32_t n = (uint32_t)__popc(lits);
    const uint32_t incl = wave_scan_add(n);
    const uint32_t T = read_lane(incl, 63) + (rc.last ? 1u : 0u);
    queued = queue != nullptr && T <= kQueueEntries;
    if (T == 0 || !queued) return T;
    uint32_t k = incl - n, t = lits;
    const uint32_t pos0 = rc.rb + 16u * l;
    while (t) {
        const uint32_t i = (uint32_t)__builtin_ctz(t);
        t &= t - 1;
        queue[k++] = ((pos0 + i) << 9) | granule_byte_dyn(w[0], w[1], w[2], w[3], i);
    }
    if (rc.last && l == 0) queue[T - 1u] = (in_size << 9) | kNoLit;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return T;
}

// entry k of the queue and the zeros in front of it
__device__ __forceinline__ void queue_entry(const uint32_t* queue, const RowCtx& rc, uint32_t k, uint32_t T, uint32_t& R, uint32_t& lit) {
    R = 0;
    lit = kNoLit;
    if (k < T) {
        const uint32_t e = queue[k];
        const uint32_t before = k ? (queue[k - 1u] >> 9) + 1u : rc.rb - rc.zb0;  // position behind the literal before this one
        lit = e & 0x1FFu;
        R = (e >> 9) - before;
    }
}

// without a queue: f(R, lit) for the lane's own entries, in stream order (the gap to the literal of a lower lane comes from a scan)
template <class F>
__device__ __forceinline__ void lane_entries(const uint32_t (&w)[4], const RowCtx& rc, uint32_t in_size, uint32_t lits, F f) {
    const uint32_t l = lane_id();
    const uint32_t pos0 = rc.rb + 16u * l;
    const uint32_t mine = lits ? pos0 + (32u - (uint32_t)__clz((int)lits)) : 0u;  // position behind this lane's last literal
    const uint32_t incl = wave_scan_incl(mine, 0u, [](uint32_t a, uint32_t b) { return a > b ? a : b; });
    uint32_t before = dpp<0x138>(0u, incl);  // wave_shr:1: behind the last literal of the lanes below
    before = max(l ? before : 0u, rc.rb - rc.zb0);
    uint32_t t = lits;
    while (t) {
        const uint32_t i = (uint32_t)__builtin_ctz(t);
        t &= t - 1;
        f(pos0 + i - before, granule_byte_dyn(w[0], w[1], w[2], w[3], i));
        before = pos0 + i + 1u;
    }
    if (rc.last && l == 63u) f(in_size - max(read_lane(incl, 63), rc.rb - rc.zb0), kNoLit);  // the run that reaches the block end
}

// The entries of a wave's sparse rows, kept for the encoder: a block of k_hist's whose sixteen segments all fit their list is
// encoded by k_encode from the lists alone -- no second pass over its 64 KiB of mostly zeros (entry lists) -- and a
// small block of k_tree's from its one list.
constexpr uint32_t kListCap = 512;             // entries per list (k_hist: per 4 KiB segment; k_tree: per small block)
constexpr uint32_t kListNone = 0xFFFFFFFFu;    // list info: no list (a dense row, or too many entries)
struct ListSink {
    uint32_t* dst;  // this wave's list
    uint32_t n;     // entries so far, or kListNone
};

__device__ __forceinline__ void hist_row_sparse(const uint32_t (&w)[4], const RowCtx& rc, uint32_t in_size, uint32_t* h, const uint32_t* runcls,
                                                uint32_t* queue, ListSink& sink) {
    if (rc.valid == 0u) return;
    if (!rc.last && !__ballot((w[0] | w[1] | w[2] | w[3]) != 0u)) return;  // nothing but zeros, and the block goes on: no token ends here
    const uint32_t lits = lane_lits(w);
    bool queued;
    const uint32_t T = sparse_queue(w, rc, in_size, lits, queue, queued);
    if (T == 0) return;
    if (queued && sink.n != kListNone && sink.n + T <= kListCap) {
        for (uint32_t c = lane_id(); c < T; c += 64) sink.dst[sink.n + c] = queue[c];
        sink.n += T;
    } else {
        sink.n = kListNone;
    }
    if (queued) {
        const uint32_t l = lane_id();
        for (uint32_t c = 0; c < T; c += 64) {
            uint32_t R, lit;
            queue_entry(queue, rc, c + l, T, R, lit);
            if (R) hist_run(h, runcls, R);
            if (lit < 256u) atomicAdd(&h[lit], 1u);
        }
        __builtin_amdgcn_wave_barrier();  // the queue is reused by the next row
    } else {
        lane_entries(w, rc, in_size, lits, [&](uint32_t R, uint32_t lit) {
            if (R) hist_run(h, runcls, R);
            if (lit < 256u) atomicAdd(&h[lit], 1u);
        });
    }
}

// one entry per lane (R zeros, then the literal unless lit == kNoLit; R = 0 and no literal: nothing), in lane order
template <class Tab>
__device__ __forceinline__ void emit_entries(uint32_t R, uint32_t lit, Tab tab, const uint32_t* runcls, uint32_t* stage, uint32_t& base) {
    const uint32_t q = run_caps(R);
    const uint32_t rem = R - q * kRunCap;
    uint64_t rv = 0;
    uint32_t rl = 0;
    if (rem) run_token(tab, runcls, rem, rv, rl);
    const uint2 lc = tab[lit < 256u ? lit : 261u];
    const uint64_t V = rv | ((uint64_t)lc.x << rl);  // <= 38 + 24 bits
    const uint32_t vlen = rl + lc.y;
    const uint32_t caplen = q ? q * (tab[260].y + 14u) : 0u;
    const uint32_t len = caplen + vlen;
    const uint32_t inc = wave_scan_add(len);
    uint32_t pos = base + inc - len;
    base += read_lane(inc, 63);
    if (q) pos += emit_run(stage, tab, runcls, pos, q * kRunCap);
    if (vlen) or_bits64(stage, pos, (uint32_t)V, (uint32_t)(V >> 32), vlen);
}

// A wave whose four rows are all sparse (the segments of the "medium" blocks: every 4 KiB non-zero, a few literals per row)
// takes them as ONE queue, and the queue is the segment's entry list as it stands.  Between sparse rows nothing special
// happens at a row boundary: the zeros in front of a row's first literal are the gap to the entry before it, whichever row
// that one came from; only entry 0 looks outside the segment (rc[0].zb0).
//
// Such a segment rarely holds more than 64 granules that are not all zero (planes 1-2 of the xdelta planes: 16 to 32 of 256 on
// average, tools/sparse_census.py), so those granules are first compacted into ONE row, in position order: a lane that holds
// one hands its four words and its block position to lane (granules of the rows before) + (granules of lower lanes of its
// row), through the wave's own queue words -- five columns of 64 words, read back before the first entry is written there.
// One lane_lits, one scan and one entry loop then do what took four of each, with most lanes idle in every one of them.
// Zero granules between compacted neighbours are the position gap, as they are between rows.  False: more than 64 such
// granules, or too many entries for the queue -- the caller goes row by row (the same entries in the same order; keeping the
// four-row body beside the compacted one for the first case cost k_hist 16 bytes of scratch).  W is never written here.
constexpr uint32_t kCompactWords = 5u * 64u;  // the compaction's columns: w0..w3 and the position
static_assert(kCompactWords <= kQueueEntries, "the compaction's scratch stays inside the wave's own queue slot (k_hist's and k_encode's own-count queues alike)");

__device__ __forceinline__ bool hist_segment_sparse(const uint32_t (&W)[4][4], const RowCtx (&rc)[4], uint32_t in_size, uint32_t* h,
                                                    const uint32_t* runcls, uint32_t* queue, ListSink& sink) {
    const uint32_t l = lane_id();
    const uint32_t last = rc[0].last | rc[1].last | rc[2].last | rc[3].last;  // the block ends in this segment: the run that reaches its end
    unsigned long long nzg[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) nzg[r] = __ballot((W[r][0] | W[r][1] | W[r][2] | W[r][3]) != 0u);  // (bytes behind the block end were masked to zero at the load)
    const uint32_t g1 = (uint32_t)__popcll(nzg[0]), g2 = g1 + (uint32_t)__popcll(nzg[1]), g3 = g2 + (uint32_t)__popcll(nzg[2]);
    const uint32_t ng = g3 + (uint32_t)__popcll(nzg[3]);
    if (ng > 64u) return false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if ((W[r][0] | W[r][1] | W[r][2] | W[r][3]) != 0u) {
            const uint32_t s = (r == 0 ? 0u : r == 1 ? g1 : r == 2 ? g2 : g3) +
                               __builtin_amdgcn_mbcnt_hi((uint32_t)(nzg[r] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nzg[r], 0u));
            queue[s] = W[r][0];
            queue[64u + s] = W[r][1];
            queue[128u + s] = W[r][2];
            queue[192u + s] = W[r][3];
            queue[256u + s] = rc[r].rb + 16u * l;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    uint32_t cg[4] = {0u, 0u, 0u, 0u};
    uint32_t pos0 = 0;
    if (l < ng) {
        cg[0] = queue[l];
        cg[1] = queue[64u + l];
        cg[2] = queue[128u + l];
        cg[3] = queue[192u + l];
        pos0 = queue[256u + l];
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();  // every lane holds its granule: the entries may take the same words
    uint32_t t = lane_lits(cg);
    const uint32_t n = (uint32_t)__popc(t);
    const uint32_t inc = wave_scan_add(n);
    const uint32_t T = read_lane(inc, 63) + (last ? 1u : 0u);
    if (T > kQueueEntries) return false;
    if (T == 0) return true;  // nothing but zeros, and the block goes on
    uint32_t k = inc - n;
    while (t) {
        const uint32_t i = (uint32_t)__builtin_ctz(t);
        t &= t - 1;
        queue[k++] = ((pos0 + i) << 9) | granule_byte_dyn(cg[0], cg[1], cg[2], cg[3], i);
    }
    if (last && l == 0) queue[T - 1u] = (in_size << 9) | kNoLit;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (sink.n != kListNone && sink.n + T <= kListCap) {
        for (uint32_t c = l; c < T; c += 64) sink.dst[sink.n + c] = queue[c];
        sink.n += T;
    } else {
        sink.n = kListNone;
    }
    const uint32_t before0 = rc[0].rb - rc[0].zb0;
    for (uint32_t c = 0; c < T; c += 64) {
        const uint32_t k = c + l;
        if (k < T) {
            const uint32_t e = queue[k];
            const uint32_t before = k ? (queue[k - 1u] >> 9) + 1u : before0;  // position behind the literal before this one
            const uint32_t R = (e >> 9) - before, lit = e & 0x1FFu;
            if (R) hist_run(h, runcls, R);
            if (lit < 256u) atomicAdd(&h[lit], 1u);
        }
    }
    __builtin_amdgcn_wave_barrier();  // the queue is reused by the next block
    return true;
}

// ===========================================================================
// k_tree: one wave per hzr block, 4 waves per workgroup
// ===========================================================================
constexpr int kTreeWaves = 4;
constexpr uint32_t kKeyMax = 0xFFFFFFFFu;

// (5084 bytes per tree and 1120 for the workgroup's run-class table: seven 4-wave workgroups = 28 trees per CU by LDS, and the
//  same seven by registers -- 67 VGPRs with the small blocks' tokenizer and encoder, held there by the launch bound (89 and five
//  workgroups without it).  The kernel
//  is a latency chain per wave -- one dense tree alone takes 0.045 ms -- so trees in flight are what it lives on; 32 against 24
//  measured no different: profiles/r03_notes.md 1f.  The small blocks' CRC reads its shift tables from global memory: 4 KiB of
//  LDS per workgroup for CRC tables meant 24 trees per CU and measured 0.081 ms against 0.079, profiles/small_blocks_notes.md.)
struct TreeLds {
    uint32_t key[kSymStride];     // leaf keys: count<<10 | (1023 - index); index order = creation order
    uint32_t lcnt[kNumSym];       // leaves in the subtree of each node, two u16 counts per word (LDS per wave decides how many
                                  // trees a CU builds at once, and the merge loop is a chain of dependent reductions)
    uint32_t up[2 * kNumSym];     // parent | isB<<10 | sibling<<11 (sibling = child_a, kept for child_b only).  Until the merges start
                                  // its first 264 words hold the block's token histogram (lhist(): dead once the counts are in registers)
    uint16_t leafsym[kSymStride];
    uint32_t tdesc[kTdescWords];
    __device__ __forceinline__ uint32_t* lhist() { return up; }
};

// The merge loop with the live keys kept SORTED (descending) across lanes and registers: element e lives in lane e % 64 of
// register e / 64, the n live ones are elements 0 .. n-1, so the two smallest keys -- the reference's `<=` scan picks exactly
// them (hzr_encode.c:251-260: count ascending, node index descending = key ascending) -- are simply elements n-1 and n-2: two
// v_readlane instead of two wave-wide reductions.  Popping them is n -= 2 (nothing moves); the parent's key goes to its place
// among the rest by ONE lane shift of the elements below it:
//     new[e] = old[e] > nk ? old[e] : (old[e-1] > nk ? nk : old[e-1])            (old[-1] = +inf)
// (what lies at or beyond n is stale and never read again: n only shrinks).  k_tree is bound by vector issue, not by latency
// (profiles/r03_notes.md: 0.9 vector instructions per cycle and CU, nearly all of them the reductions' half-rate DPP steps):
// per merge this is 2 + 5 per live register instructions against the 54 .. 76 of round 2's form (the live keys unordered in
// ceil(S/64) registers, two DPP wave-min extractions per merge).  The sort in front (rank = number of greater keys, keys are
// unique) costs ~7 instructions per leaf.
template <int NR>
__device__ __forceinline__ void sorted_merge_phase(TreeLds& t, uint32_t (&kreg)[5], uint32_t& n, uint32_t& node) {
    const uint32_t l = lane_id();
    while (n > 64u * (NR - 1) && n >= 2u) {
        const uint32_t e1 = n - 1u, e2 = n - 2u;
        uint32_t m1 = 0, m2 = 0;
#pragma unroll
        for (int r = 0; r < NR; ++r) {  // (wave-uniform selects: the two smallest sit in the last one or two live registers)
            if ((e1 >> 6) == (uint32_t)r) m1 = read_lane(kreg[r], e1 & 63u);
            if ((e2 >> 6) == (uint32_t)r) m2 = read_lane(kreg[r], e2 & 63u);
        }
        const uint32_t nk = (((m1 >> 10) + (m2 >> 10)) << 10) | (1023u - node);
        // insert nk among elements 0 .. n-3, from the top register down (a register's lane 0 looks at the OLD lane 63 below it)
#pragma unroll
        for (int r = NR - 1; r >= 0; --r) {
            const uint32_t below = r ? read_lane(kreg[r ? r - 1 : 0], 63u) : kKeyMax;
            const uint32_t prev = dpp<0x138>(below, kreg[r]);  // wave_shr:1 -- lane l sees lane l-1, lane 0 keeps `below`
            kreg[r] = kreg[r] > nk ? kreg[r] : (prev > nk ? nk : prev);
        }
        const uint32_t i1 = 1023u - (m1 & 1023u), i2 = 1023u - (m2 & 1023u);
        if (l == 0) {
            t.up[i1] = node;                             // child_a: code bit 0, described right after the branch bit
            t.up[i2] = node | (1u << 10) | (i1 << 11);  // child_b: code bit 1, described after child_a's subtree
        }
        ++node;
        --n;
    }
}

__device__ __forceinline__ void sorted_merge(TreeLds& t, uint32_t S) {
    const uint32_t l = lane_id();
    const uint32_t nreg = (S + 63u) >> 6;
    // ---- sort: every key's rank = the number of keys greater than it (unique keys: a permutation) ----
    uint32_t mine[5], rank[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        mine[r] = (uint32_t)(r * 64) + l < S ? t.key[r * 64 + l] : kKeyMax;  // (lanes past the last leaf take no part)
        rank[r] = 0;
    }
    auto count_greater = [&](uint32_t nr) {
        for (uint32_t j = 0; j < S; ++j) {
            const uint32_t kj = t.key[j];  // (one address for all lanes: a broadcast read)
#pragma unroll
            for (int r = 0; r < 5; ++r)
                if ((uint32_t)r < nr) rank[r] += kj > mine[r] ? 1u : 0u;
        }
    };
    if (nreg <= 1) count_greater(1);
    else if (nreg <= 2) count_greater(2);
    else if (nreg <= 3) count_greater(3);
    else count_greater(5);
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();  // (every lane has read all the keys: they are sorted in place)
#pragma unroll
    for (int r = 0; r < 5; ++r)
        if ((uint32_t)r < nreg && (uint32_t)(r * 64) + l < S) t.key[rank[r]] = mine[r];
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    uint32_t kreg[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) kreg[r] = ((uint32_t)(r * 64) + l < S) ? t.key[r * 64 + l] : 0u;
    // ---- merges, with as many registers as still hold live keys ----
    uint32_t n = S, node = S;
    if (nreg > 4) sorted_merge_phase<5>(t, kreg, n, node);
    if (nreg > 3) sorted_merge_phase<4>(t, kreg, n, node);
    if (nreg > 2) sorted_merge_phase<3>(t, kreg, n, node);
    if (nreg > 1) sorted_merge_phase<2>(t, kreg, n, node);
    sorted_merge_phase<1>(t, kreg, n, node);
}

struct TreeOut {  // wave-uniform
    uint32_t mode, payload_len, tree_bits, ntok, fill;
};

// One wave: token histogram h[0..260] (LDS) of an hzr block of in_size bytes -> Fill test (hzr_encode.c:285-305),
// Huffman tree with the reference's tie-break (:222-283), the pre-order tree description in t.tdesc (:177-219), and the
// block's mode and exact payload size (:377-469).  The code words, code | length << 24, go to cw_out[sym] (global memory) and
// t.key[sym] keeps the symbol's stream bits per token -- or, with cw_out == nullptr (wave-uniform), the code words stay in
// t.key[sym] themselves: the table of a small block's own emit.
__device__ __forceinline__ TreeOut build_tree(TreeLds& t, const uint32_t* h, uint32_t in_size, uint32_t* __restrict__ cw_out) {
    const uint32_t l = lane_id();
    // ---- leaves in ascending symbol order (hzr_encode.c:226-234) ----------
    uint32_t cnt[5], idx[5];
    uint32_t base = 0, nonzero_syms = 0, zero_kind = 0, fillval = 0;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const uint32_t s = r * 64 + l;
        cnt[r] = s < (uint32_t)kNumSym ? h[s] : 0u;
        const unsigned long long bal = __ballot(cnt[r] != 0);
        idx[r] = base + (uint32_t)__popcll(bal & ((1ull << l) - 1ull));
        base += (uint32_t)__popcll(bal);
        // OnlySingleCode (hzr_encode.c:285-305): all zero-type symbols count as one code
        const bool is_zero_kind = (s == 0) || (s >= 256);
        const unsigned long long nzb = __ballot(cnt[r] != 0 && !is_zero_kind);
        nonzero_syms += (uint32_t)__popcll(nzb);
        zero_kind |= __ballot(cnt[r] != 0 && is_zero_kind) ? 1u : 0u;
        if (nzb) fillval = max(fillval, (uint32_t)(r * 64 + (63 - __builtin_clzll(nzb))));
    }
    const uint32_t S = base;
    if (zero_kind + nonzero_syms == 1) return TreeOut{kModeFill, 1u, 0u, 0u, zero_kind ? 0u : fillval};  // EncodeFill (:341-367)

    // ---- node arrays -------------------------------------------------------
    for (uint32_t i = l; i < (uint32_t)kSymStride; i += 64) t.key[i] = kKeyMax;
    for (uint32_t i = l; i < (uint32_t)kNumSym; i += 64) t.lcnt[i] = (2u * i < S ? 1u : 0u) | (2u * i + 1u < S ? 1u << 16 : 0u);
    for (uint32_t i = l; i < (uint32_t)kTdescWords; i += 64) t.tdesc[i] = 0;
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        if (cnt[r]) {
            t.key[idx[r]] = (cnt[r] << 10) | (1023u - idx[r]);
            t.leafsym[idx[r]] = (uint16_t)(r * 64 + l);
        }
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();

    const uint32_t nnodes = 2 * S - 1;
#if defined(TREE_PROBE) && TREE_PROBE == 2  // timing probes (never in the product)
    return TreeOut{kModeFill, 1u, 0u, 0u, 0u};
#endif
    sorted_merge(t, S);
#if defined(TREE_PROBE) && TREE_PROBE == 1
    return TreeOut{kModeFill, 1u, 0u, 0u, 0u};
#endif
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();

    // ---- leaves under every internal node: each leaf credits its ancestors ----
    const uint32_t root = nnodes - 1;
    for (uint32_t i = l; i < S; i += 64) {
        uint32_t cur = i, guard = 0;
        while (cur != root && guard++ < 64) {  // depth <= 22 for <= 65536 tokens; the bound only guards against a corrupted link
            cur = t.up[cur] & 1023u;
            atomicAdd(&t.lcnt[cur >> 1], 1u << ((cur & 1u) * 16u));
        }
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();

    // ---- per-leaf walk to the root: code, length, description offset -------
    // a subtree with L leaves is described in 10 L + (L - 1) bits (leaf = '1' + 9-bit symbol, branch = '0')
    const uint32_t tree_bits = 11u * S - 1u;
    uint32_t bits_sum = 0;
    for (uint32_t i = l; i < S; i += 64) {
        uint32_t cur = i, code = 0, len = 0, off = 0;
        while (cur != root && len < 64) {
            const uint32_t u = t.up[cur];
            const uint32_t is_b = (u >> 10) & 1u;
            code = (code << 1) | is_b;
            off += is_b ? 11u * ((t.lcnt[u >> 12] >> (((u >> 11) & 1u) * 16u)) & 0xFFFFu) : 1u;  // '0' of the branch (+ all of child_a's subtree: 1 + 11 L - 1)
            ++len;
            cur = u & 1023u;
        }
        const uint32_t sym = t.leafsym[i];
        const uint32_t packed = code | (len << 24);
        if (cw_out) cw_out[sym] = packed;
        t.key[sym] = cw_out ? len + run_extra_bits(sym) : packed;  // (the key slots are free now)
        // description: '1' then the 9-bit symbol, LSB first (hzr_encode.c:184-191)
        const uint32_t v = 1u | (sym << 1);
        const uint32_t wi = off >> 5, sh = off & 31u;
        atomicOr(&t.tdesc[wi], v << sh);
        if (sh > 22) atomicOr(&t.tdesc[wi + 1], v >> (32 - sh));
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    // payload bits of the codes: every symbol's count (still in this lane's registers: the histogram's LDS words were taken over
    // by the tree's links) times its stream bits per token
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const uint32_t s2 = r * 64 + l;
        const uint32_t kept = t.key[s2 < (uint32_t)kNumSym ? s2 : 0u];
        if (cnt[r]) bits_sum += cnt[r] * (cw_out ? kept : (kept >> 24) + run_extra_bits(s2));
    }
    bits_sum = wave_add_u32(bits_sum);
    const uint32_t ntok = wave_add_u32(cnt[0] + cnt[1] + cnt[2] + cnt[3] + cnt[4]);
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    const uint32_t total_bits = tree_bits + bits_sum;
    const uint32_t nbytes = (total_bits + 7) >> 3;
    // Huffman iff the payload fits in in_size bytes and is < 65536 (hzr_encode.c:377-382,463-469)
    const bool huff = nbytes <= in_size && nbytes < kHzrBlock;
    if (huff) return TreeOut{kModeHuff, nbytes, tree_bits, ntok, 0u};  // (ntok travels in BlockMeta::fill in this mode)
    return TreeOut{kModeCopy, in_size, 0u, 0u, 0u};
}

// ---------------------------------------------------------------------------------------------
// Small blocks: one wave of k_tree tokenizes the block ONCE, with the compacted-row tokenizer of k_hist's sparse segments
// (hist_segment_sparse and its fall-backs), counts the tokens into its histogram and keeps the entries -- position << 9 |
// literal, in stream order, the run that reaches the block end as a last entry at in_size -- as one list in the block's own
// staging slot (free until the block's header + payload go there; nothing else reads the slot of a block that is not staged).
// After the tree the same wave encodes the block from that list alone, 64 entries per pass (emit_entries, as k_encode does
// for its list blocks): a zero run is the gap between two entries, so all-zero segments, rows and granules cost nothing.
// A staged block has at most kSmallTokens tokens and every entry yields at least one, so its list always fits kListCap; a
// block whose list overflows is by the same count not staged and goes to k_encode as before.
// The tree's LDS is dead by the emit except for the description: the code table stays where build_tree left it (the key
// slots), the image (X || payload + read slack) goes over the node arrays behind them.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kSlotImage = 826;  // words of X || payload (+ slack)
static_assert(kSlotImage * 4 >= kSmallPayload + 4 + 72, "small-block image too small");
static_assert(offsetof(TreeLds, key) == 0 && offsetof(TreeLds, lcnt) == kSymStride * 4, "the code table takes the key slots, the image starts behind them");
static_assert((kSymStride + kSlotImage) * 4 <= offsetof(TreeLds, tdesc), "the image must leave the tree description alone");
static_assert(kQueueEntries * 4 <= offsetof(TreeLds, up), "the tokenizer's queue takes the key and lcnt words (build_tree initialises them afterwards); the histogram sits in up");
static_assert(kListCap <= kStageSlotWords, "a small block's entry list waits in its staging slot");

// Token histogram h and entry list of a small block by one wave; returns the number of entries, or kListNone.  Zero 4 KiB
// segments are skipped without a read.  The tokenizer never sees the block end (RowCtx::last = 0): the run that reaches it
// is counted and listed here, whichever segment the block's last literal lies in.
__device__ __forceinline__ uint32_t small_block_tokens(const uint8_t* __restrict__ in, uint32_t in_size, uint32_t segmask, uint32_t* h,
                                                       const uint32_t* runcls, uint32_t* queue, uint32_t* list) {
    const uint32_t l = lane_id();
    ListSink sink{list, 0u};
    uint32_t behind = 0;  // position behind the block's last literal so far (wave-uniform)
    for (uint32_t m = segmask; m; m &= m - 1u) {
        const uint32_t seg_base = (uint32_t)__builtin_ctz(m) << 12;
        uint32_t W[4][4];
        RowCtx rc[4];
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {  // the segment's four rows in one round trip
            const uint32_t pos = seg_base + (r << 10) + 16u * l;
            uint4 v = make_uint4(0, 0, 0, 0);
            if (pos < in_size) v = *reinterpret_cast<const uint4*>(in + pos);  // plane rows are padded: a partial granule may over-read
            W[r][0] = v.x;
            W[r][1] = v.y;
            W[r][2] = v.z;
            W[r][3] = v.w;
            if (pos + 16u > in_size && pos < in_size) {  // the block's last, partial granule: bytes behind it read as zero
                const uint32_t nv = in_size - pos;
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const uint32_t lo = q * 4u;
                    W[r][q] = nv >= lo + 4u ? W[r][q] : nv <= lo ? 0u : (W[r][q] & ((1u << ((nv - lo) * 8u)) - 1u));
                }
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < 4; ++r) {
            const uint32_t rb = seg_base + (r << 10);
            rc[r].rb = rb;
            rc[r].valid = rb >= in_size ? 0u : min(1024u, in_size - rb);
            rc[r].last = 0u;
            rc[r].zb0 = rb - behind;
            const unsigned long long nzg = __ballot((W[r][0] | W[r][1] | W[r][2] | W[r][3]) != 0u);
            if (nzg) {
                const uint32_t ph = 63u - (uint32_t)__builtin_clzll(nzg);
                behind = rb + 16u * ph + 16u - read_lane(trail_zero_bytes(W[r][0], W[r][1], W[r][2], W[r][3]), ph);
            }
        }
        if (!hist_segment_sparse(W, rc, in_size, h, runcls, queue, sink)) {  // more than 64 non-zero granules or 512 entries: row by row
#pragma unroll 1
            for (int r = 0; r < 4; ++r) {
                hist_row_sparse(W[0], rc[0], in_size, h, runcls, queue, sink);
                rotate_rows(W, rc);
            }
        }
    }
    const uint32_t R = in_size - behind;  // the run that reaches the block end
    if (R) {
        if (l == 0) hist_run(h, runcls, R);
        if (sink.n < kListCap) {  // (kListNone is not)
            if (l == 0) list[sink.n] = (in_size << 9) | kNoLit;
            ++sink.n;
        } else {
            sink.n = kListNone;
        }
    }
    return sink.n;
}

struct PackedCodes {  // k_tree's code table as the emit helpers read it: code | length << 24 per symbol
    const uint32_t* w;
    __device__ __forceinline__ uint2 operator[](uint32_t i) const {
        const uint32_t c = w[i];
        return make_uint2(c & 0x00FFFFFFu, c >> 24);
    }
};

// One wave: emit the block from its n entries (list: global memory, written by this wave) with the code words in cwt and the
// tree description in tdesc_lds (both LDS) into img, checksum it, and store [7-byte block header][payload] to the block's staging
// slot -- over the list, which is in registers by then; k_encode copies it to its stream offset, which only k_layout knows.
// The literals' granules are wiped on the way (clean-block invariant: block_is_wiped).  Work follows the payload: the image is
// zeroed as far as the payload and the CRC's read slack reach, and the CRC-32C goes by words across the lanes.
__device__ __forceinline__ void stage_small_block(uint32_t* cwt, uint32_t* img, const uint32_t* tdesc_lds, const uint32_t* runcls,
                                                  const uint32_t* list, uint32_t n, uint8_t* __restrict__ in, uint32_t in_size, uint32_t L, uint32_t tree_bits,
                                                  const CrcConsts* __restrict__ cc, uint32_t* slot) {
    const uint32_t l = lane_id();
    const uint32_t zwords = min(((L + 4u) >> 2) + 4u, kSlotImage);  // X + payload, the word the CRC reads behind them, or_bits64's reach
    for (uint32_t i = l; i < zwords; i += 64) img[i] = 0;
    if (l < 3u) cwt[(uint32_t)kNumSym + l] = 0u;  // index 261: {0, 0}, what an entry without a literal looks up; 263: the zero word in front of the image
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the list's stores (issued before the tree was built) are done before it is read back
    if (l == 0) img[0] = cc->prefix;
    const uint32_t twords = (tree_bits + 31) >> 5;
    for (uint32_t i = l; i < twords; i += 64) atomicOr(&img[1 + i], tdesc_lds[i]);

    // the entries come back past the L1 (another lane stored them), the next pass's load in flight during this one's emit
    auto entry = [&](uint32_t k) -> uint32_t { return k < n ? __hip_atomic_load(&list[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u; };
    uint32_t base = 32u + tree_bits;  // next stream bit (wave-uniform): the payload starts at image byte 4
    uint32_t carry = 0;               // the entry in front of lane 0's (wave-uniform)
    uint32_t e_next = entry(l);
    for (uint32_t c = 0; c < n; c += 64) {
        const uint32_t e = e_next, kq = c + l;
        e_next = entry(kq + 64u);
        const uint32_t prev = dpp<0x138>(carry, e);  // wave_shr:1 -- lane l sees lane l-1's entry, lane 0 the pass before
        uint32_t R = 0, lit = kNoLit;
        if (kq < n) {
            const uint32_t before = kq ? (prev >> 9) + 1u : 0u;  // position behind the literal before this one
            lit = e & 0x1FFu;
            R = (e >> 9) - before;
            // clean-block invariant: a staged block leaves zeros behind (the granule of every literal)
            if (lit < 256u && (e >> 9) < in_size) *reinterpret_cast<uint4*>(in + ((e >> 9) & ~15u)) = make_uint4(0, 0, 0, 0);
        }
        emit_entries(R, lit, PackedCodes{cwt}, runcls, img, base);
        carry = read_lane(e, 63);
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();

    // CRC-32C of V = X || payload (Lv = L + 4 bytes from image byte 0) as 4-byte virtual words counted from its END: lane l owns
    // the words l, l + 64, ... -- Horner over them with x^(8*256) per step (CrcConsts::shift[59]), then x^(8*4*(l+1)) to the end
    // of V and a wave XOR: ceil(words / 64) steps, as k_encode's per-wave group (tools/kernel_model.py: crc_wave_words).
    // Virtual word r = image words a and a + 1 joined at byte (Lv & 3), a = (Lv >> 2) - 1 - r; a = -1 is the zero word cwt[263].
    const int32_t Lv = (int32_t)L + 4;
    const uint32_t nvw = (uint32_t)(Lv + 3) >> 2;
    const uint32_t K = (nvw + 63u) >> 6;  // steps of the fullest lane
    const uint32_t sh = (uint32_t)Lv & 3u;
    auto vword = [&](int32_t a) -> uint32_t { return __builtin_amdgcn_alignbyte(img[a + 1], img[a], sh); };
    uint32_t c = 0;
    if (l < nvw) {
        int32_t a = (Lv >> 2) - 1 - (int32_t)(l + 64u * (K - 1u));
        if (K > 1u) {
            c = a >= -1 ? vword(max(a, -1)) : 0u;  // (the top word: there for the low lanes only)
            c = gf_shift(cc, 59u, c);
            for (uint32_t kk = K - 2u; kk >= 1u; --kk) {
                a += 64;
                c ^= vword(a);
                c = gf_shift(cc, 59u, c);
            }
            a += 64;
        }
        c ^= vword(a);
    }
    const uint32_t crc = ~wave_xor_u32(gf_shift4(cc, l, c));

    // slot byte s = stream byte s of the encoded block: [L-1 u16][crc u32][mode], then payload byte s - 7 = image byte s - 3
    const uint32_t nw = (7u + L + 3u) >> 2;
    for (uint32_t w = l; w < nw; w += 64) {
        uint32_t v;
        if (w == 0) v = ((L - 1u) & 0xFFFFu) | (crc << 16);
        else if (w == 1) v = (crc >> 16) | (kModeHuff << 16) | (img[1] << 24);
        else v = __builtin_amdgcn_alignbyte(img[w], img[w - 1u], 1u);
        slot[w] = v;
    }
}

// k_tree: one wave per hzr block, 4 waves per workgroup.  Small blocks (<= kSmallSegments non-zero 4 KiB segments) take their
// own histogram here -- and, if they also have few tokens and a small payload, are encoded here too, into their staging slot
// (BlockMeta::mode = kModeStaged: the one mark k_layout and k_encode go by); for the others k_hist left the block histogram and
// the per-segment histograms, which -- times the code lengths -- give the stream bit at which each 4 KiB segment's tokens start
// (k_encode then needs no bit-count pass).
__global__ __launch_bounds__(kTreeWaves * 64, 7) void k_tree(const uint32_t* __restrict__ hist, uint8_t* __restrict__ planes, Geom g,
                                                         const uint32_t* __restrict__ nbuse, const uint32_t* __restrict__ nzflag,
                                                         uint32_t nhb_total, uint32_t* __restrict__ cw, uint32_t* __restrict__ tdesc,
                                                         BlockMeta* __restrict__ meta, const uint32_t* __restrict__ seghist,
                                                         uint32_t* __restrict__ segbase, uint32_t* __restrict__ zero_next, uint32_t zero_words,
                                                         const CrcConsts* __restrict__ cc, uint32_t* __restrict__ staging, uint32_t psel_arg) {
    const uint32_t psel = RSPT_DIAG_ONLY(psel_arg);  // timing probes (diagnostic builds only): no tree for plane 0 (bit 4) / planes >= 1 (bit 5)
    __shared__ TreeLds s_t[kTreeWaves];
    __shared__ uint32_t s_runcls[kRunClsEntries];  // run length -> symbol, extra bits, base: the small blocks' tokenizer and emit
    static_assert((sizeof(TreeLds) * kTreeWaves + sizeof(uint32_t) * kRunClsEntries) * 7 <= 160 * 1024, "seven k_tree workgroups (28 trees) per CU");
    const uint32_t l = lane_id();
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (wave-uniform: the block's index, size and addresses stay in scalar registers)
    // the other copy of the per-call zero region, for the next call (rspt_hip.hip: zbuf)
    for (uint32_t i = blockIdx.x * (kTreeWaves * 64u) + threadIdx.x; i < zero_words; i += gridDim.x * (kTreeWaves * 64u)) zero_next[i] = 0;
    for (uint32_t i = threadIdx.x; i < kRunClsEntries; i += kTreeWaves * 64u) s_runcls[i] = run_class_entry(i);
    __syncthreads();  // (the only one: from here on every wave is on its own)
    // wave -> hzr block, plane-major: all the blocks of plane 0 (the dense, expensive ones) are dispatched first and
    // next to each other, so they spread over every CU; in (b, k, j) order they recur with a period that the
    // dispatcher's round-robin maps onto a quarter of the CUs (profiles/r01_notes.md: placement resonance)
    const uint32_t v = blockIdx.x * kTreeWaves + wv;
    if (v >= nhb_total) return;
    const uint32_t per_plane = nhb_total / kMaxPlanes;  // = blocks * nblk
    const uint32_t k = v / per_plane, rest = v - k * per_plane;
    const uint32_t b = rest / g.nblk, j = rest - b * g.nblk;
    const uint32_t hb = hb_index(g, b, k, j);
    TreeLds& t = s_t[threadIdx.x >> 6];  // (the wave's LDS through a vector register, as the merge loop's lane-0 stores want it: a scalar base costs them four moves per merge)
    if (k >= nbuse[b]) {
        if (l == 0) meta[hb] = BlockMeta{kModeSkip, 0, 0, 0};
        return;
    }
    const uint32_t segmask =  // (one word per wave: in a scalar register, so that what hangs on it is a scalar branch)
        (uint32_t)__builtin_amdgcn_readfirstlane((int)((psel && ((k == 0 && (psel & 16u)) || (k >= 1 && (psel & 32u)))) ? 0u : nzflag[hb]));
    if (!segmask) {  // all-zero block (flagged by the front end): EncodeFill with value 0
        if (l == 0) meta[hb] = BlockMeta{kModeFill, 1u, 0u, 0u};
        return;
    }
    const uint32_t in_size = min(kHzrBlock, g.N - j * kHzrBlock);
    uint32_t* h = t.lhist();
    uint8_t* in = planes + ((size_t)b * kMaxPlanes + k) * g.plane_stride + (size_t)j * kHzrBlock;
    const bool own_hist = (uint32_t)__popc(segmask) <= kSmallSegments;
    if (l == 0) segbase[(size_t)hb * kEncWaves] = 0xFFFFFFFFu;  // "no segment offsets" unless set below
    uint32_t* lds = reinterpret_cast<uint32_t*>(&t);
    uint32_t* slot = staging + (size_t)hb * kStageSlotWords;
    uint32_t nlist = kListNone;  // entries of the small block's list
    if (own_hist) {  // small block: this wave takes the histogram itself, and keeps the entries
        for (uint32_t i = l; i < (uint32_t)kSymStride; i += 64) h[i] = 0;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        const uint32_t nseg = (in_size + 4095u) >> 12;
        nlist = small_block_tokens(in, in_size, segmask & ((1u << nseg) - 1u), h, s_runcls, lds, slot);
    } else {
        for (uint32_t i = l; i < (uint32_t)kSymStride; i += 64) h[i] = hist[(size_t)hb * kSymStride + i];
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    // The code words: k_encode reads them from cw[]; a small block's stay in this wave's LDS (t.key), for its own emit -- they
    // leave for cw[] only if the block turns out too big to be staged.
    uint32_t* cwo = cw + (size_t)hb * kSymStride;
    const TreeOut r = build_tree(t, h, in_size, own_hist ? nullptr : cwo);
    // small enough for this wave to encode it right here?  (wave-uniform; the same mark decides in k_layout and k_encode.  The
    // list is there whenever the tokens are few enough -- see above; the test only keeps a read of a list that is not in bounds.)
    const bool staged = own_hist && r.mode == kModeHuff && r.payload_len <= kSmallPayload && r.ntok <= kSmallTokens && nlist != kListNone;
    if (l == 0) meta[hb] = BlockMeta{staged ? kModeStaged : r.mode, r.payload_len, r.tree_bits, r.mode == kModeHuff ? r.ntok : r.fill};
    if (r.mode != kModeHuff) return;
    if (staged) {
        stage_small_block(lds, lds + kSymStride, t.tdesc, s_runcls, slot, nlist, in, in_size, r.payload_len, r.tree_bits, cc, slot);
        return;
    }
    if (own_hist)  // k_encode takes the block (own_bits), untouched: it needs the code words after all
        for (uint32_t i = l; i < (uint32_t)kNumSym; i += 64) cwo[i] = t.key[i];
    uint32_t* tdo = tdesc + (size_t)hb * kTdescWords;
    for (uint32_t i = l; i < (uint32_t)kTdescWords; i += 64) tdo[i] = t.tdesc[i];
    if (own_hist) return;
    // (bins 261..263 of k_hist's histograms count the zero bytes that end no token: they cost nothing)
    if (l < 3u) t.key[(uint32_t)kNumSym + l] = 0u;
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();

    // ---- stream bit at which the tokens of each 4 KiB segment start (k_hist's per-segment histograms x code lengths) ----
    // lane l: segment l / 4, every fourth of its 132 u16 pairs from pair l % 4 on (the four lanes of a segment read 16
    // consecutive bytes: a wave load touches 16 lines, not 64)
    {
        const uint32_t seg = l >> 2, part = l & 3u;
        const uint32_t* sh = seghist + (size_t)hb * (kSegHistStride / 2) + seg * (kSymStride / 2) + part;
        uint32_t pr[33];
#pragma unroll
        for (int i = 0; i < 33; ++i) pr[i] = sh[4 * i];
        uint32_t acc = 0;
#pragma unroll
        for (int i = 0; i < 33; ++i) {
            const uint32_t s0 = 2u * (4u * (uint32_t)i + part);
            // unused symbols have count 0: whatever their cost slots hold is multiplied away
            acc += (pr[i] & 0xFFFFu) * t.key[s0];
            acc += (pr[i] >> 16) * t.key[s0 + 1u];
        }
        acc += dpp<0xB1>(0u, acc);  // quad_perm [1,0,3,2]
        acc += dpp<0x4E>(0u, acc);  // quad_perm [2,3,0,1]: every lane of the quad holds the segment's bits
        // exclusive prefix over the 16 segments (one value per quad): scan with the quad's bits counted once
        const uint32_t mine = part == 0 ? acc : 0u;
        const uint32_t incl = wave_scan_add(mine);
        if (part == 0) segbase[(size_t)hb * kEncWaves + seg] = 32u + r.tree_bits + incl - mine;  // the payload starts at image byte 4
    }
}

// ===========================================================================
// k_layout: one workgroup per block.  Stream grammar:
//   [method][means header][ per plane k<nb: u32 len_k, u32 N, hzr blocks... ]
// ===========================================================================
__device__ __forceinline__ void store_le32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}

// It also fills the work queue of k_encode: Fill blocks (8 bytes) are written right here; the small blocks k_tree has
// encoded already (kModeStaged) only need their offset, which k_encode's placing copy reads from out_off; everything
// else goes to the `big` queue (one 1024-thread workgroup per block).


__global__ __launch_bounds__(256) void k_layout(Geom g, const uint32_t* __restrict__ nbuse, const BlockMeta* __restrict__ meta,
                                               const uint8_t* __restrict__ means_hdr, uint8_t* __restrict__ dst, uint64_t dst_stride,
                                               uint64_t* __restrict__ out_off, uint64_t* __restrict__ sizes, const CrcConsts* __restrict__ cc,
                                               const uint32_t* __restrict__ nzflag, WorkQueues* __restrict__ wq,
                                               uint32_t* __restrict__ big_list,
                                               uint32_t* __restrict__ plane_dirty, uint32_t dirty_shift, uint32_t psel_arg) {
    const uint32_t psel = RSPT_DIAG_ONLY(psel_arg);  // timing probes (diagnostic builds only): k_encode gets no plane 0 (bit 2) / planes >= 1 (bit 3)
    __shared__ uint64_t s_part[256];
    __shared__ uint64_t s_plane_end[kMaxPlanes + 1];
    __shared__ uint32_t s_dirty[kMaxPlanes * 4];  // 128 bits per plane: hzr blocks (j >> dirty_shift) that keep their data
    if (threadIdx.x < kMaxPlanes * 4) s_dirty[threadIdx.x] = 0;
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const uint32_t nb = nbuse[b];
    const uint32_t n = nb * g.nblk;  // hzr blocks of this block, (k,j) order
    const uint32_t per = (n + 255) / 256;
    const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
    const uint32_t hb0 = hb_index(g, b, 0, 0);
    auto enc_size = [&](uint32_t q) -> uint64_t {  // q = k*nblk + j
        return 7ull + meta[hb0 + q].payload_len;
    };
    uint64_t sum = 0;
    __syncthreads();  // (s_dirty is zeroed)
    for (uint32_t q = lo; q < hi; ++q) {
        sum += enc_size(q);
        // non-zero data that no encoder wipes (dense Huffman blocks, PlainCopy, constant non-zero blocks) stays behind
        if (nzflag[hb0 + q] && !block_is_wiped(meta[hb0 + q])) {
            const uint32_t k = q / g.nblk, bucket = (q - k * g.nblk) >> dirty_shift;
            atomicOr(&s_dirty[k * 4 + (bucket >> 5)], 1u << (bucket & 31u));
        }
    }
    // exclusive prefix of the 256 partial sums: a scan inside each wave, the four wave totals through LDS (the single-thread
    // loop over 256 LDS words this replaces was most of the kernel's 13 us: ~50 dependent LDS round trips per microsecond)
    uint64_t run;
    {
        const uint32_t l = tid & 63u, wv = tid >> 6;
        uint64_t inc = sum;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            const uint64_t up = (uint64_t)__shfl_up((long long)inc, dd, 64);
            if (l >= (uint32_t)dd) inc += up;
        }
        if (l == 63u) s_part[wv] = inc;
        __syncthreads();
        uint64_t pre = 0;
        for (uint32_t q2 = 0; q2 < wv; ++q2) pre += s_part[q2];
        run = pre + inc - sum;
    }
    // absolute offset of hzr block q: 1 + hdr + 8*(k+1) + sum of the encoded blocks before it
    const uint64_t head = 1ull + g.hdr_len;
    for (uint32_t q = lo; q < hi; ++q) {
        const uint32_t k = q / g.nblk;
        out_off[hb0 + q] = head + 8ull * (k + 1) + run;
        run += enc_size(q);
        if ((q + 1) % g.nblk == 0) s_plane_end[k + 1] = run;  // encoded bytes up to the end of plane k
    }
    if (tid == 0) s_plane_end[0] = 0;
    __syncthreads();
    if (g.kind == kKindBytes) {
        // Bare framing (hzr_encode.c:499-545): every plane of the slot is a buffer of its own and leaves as one libhzr stream --
        // u32 LE size, then the hzr blocks; no method byte, no plane length word -- at dst + (4 b + k) * dst_stride, its length
        // in sizes[4 b + k].  k_encode is launched with four times the stride, so the offsets carry k * dst_stride.
        for (uint32_t q = lo; q < hi; ++q) {
            const uint32_t k = q / g.nblk;
            const bool fits_k = 4ull + (s_plane_end[k + 1] - s_plane_end[k]) <= dst_stride;
            // (out_off holds head + 8 (k + 1) + the encoded bytes in front of the block: back to the offset inside plane k's stream)
            out_off[hb0 + q] = fits_k ? (uint64_t)k * dst_stride + 4ull + (out_off[hb0 + q] - head - 8ull * (k + 1) - s_plane_end[k]) : ~0ull;
        }
        if (tid < nb) {
            const uint64_t total_k = 4ull + (s_plane_end[tid + 1] - s_plane_end[tid]);
            sizes[(size_t)b * kMaxPlanes + tid] = total_k <= dst_stride ? total_k : (total_k | (1ull << 63));
        }
        if (tid < nb * 4) {
            const uint32_t k = tid >> 2;
            const bool fits_k = 4ull + (s_plane_end[k + 1] - s_plane_end[k]) <= dst_stride;
            plane_dirty[(size_t)b * kMaxPlanes * 4 + tid] = fits_k ? s_dirty[tid] : 0xFFFFFFFFu;
        }
        uint8_t* o = dst + (size_t)b * kMaxPlanes * dst_stride;
        for (uint32_t q = lo; q < hi; ++q) {
            const BlockMeta m = meta[hb0 + q];
            const uint64_t off = out_off[hb0 + q];
            if (off == ~0ull) continue;  // the buffer's stream does not fit: nothing of it is written
            if (m.mode == kModeFill) {  // EncodeFill, as below
                uint8_t* f = o + off;
                uint32_t c = 0xFFFFFFFFu ^ m.fill;
                c = ~((c >> 8) ^ cc->table[0][c & 0xFFu]);
                f[0] = 0;
                f[1] = 0;
                f[2] = (uint8_t)c;
                f[3] = (uint8_t)(c >> 8);
                f[4] = (uint8_t)(c >> 16);
                f[5] = (uint8_t)(c >> 24);
                f[6] = (uint8_t)kModeFill;
                f[7] = (uint8_t)m.fill;
            } else if (m.mode == kModeHuff || m.mode == kModeCopy) {
                big_list[atomicAdd(&wq->n_big, 1u)] = hb0 + q;
            }
        }
        if (tid < nb && 4ull + (s_plane_end[tid + 1] - s_plane_end[tid]) <= dst_stride) store_le32(o + (uint64_t)tid * dst_stride, g.N);  // hzr_encode.c:521-522
        return;
    }
    const uint64_t total = head + 8ull * nb + s_plane_end[nb];
    const bool fits = total <= dst_stride;
    if (tid == 0) sizes[b] = fits ? total : (total | (1ull << 63));
    // the planes written in this call: dirty when a dense block stays behind, or when nothing will be encoded (and wiped) at all
    if (tid < nb * 4) plane_dirty[(size_t)b * kMaxPlanes * 4 + tid] = fits ? s_dirty[tid] : 0xFFFFFFFFu;
    if (!fits) {  // tell k_encode to leave this block alone
        for (uint32_t q = lo; q < hi; ++q) out_off[hb0 + q] = ~0ull;
        return;
    }
    uint8_t* o = dst + (size_t)b * dst_stride;
    for (uint32_t q = lo; q < hi; ++q) {
        const BlockMeta m = meta[hb0 + q];
        if (m.mode == kModeFill) {  // EncodeFill (hzr_encode.c:341-367): [00 00][crc32c(value)][02][value]
            uint8_t* f = o + out_off[hb0 + q];
            uint32_t c = 0xFFFFFFFFu ^ m.fill;
            c = ~((c >> 8) ^ cc->table[0][c & 0xFFu]);
            f[0] = 0;
            f[1] = 0;
            f[2] = (uint8_t)c;
            f[3] = (uint8_t)(c >> 8);
            f[4] = (uint8_t)(c >> 16);
            f[5] = (uint8_t)(c >> 24);
            f[6] = (uint8_t)kModeFill;
            f[7] = (uint8_t)m.fill;
        } else if (m.mode == kModeHuff || m.mode == kModeCopy) {
            if (psel && ((q / g.nblk == 0 && (psel & 4u)) || (q / g.nblk >= 1 && (psel & 8u)))) continue;
            big_list[atomicAdd(&wq->n_big, 1u)] = hb0 + q;
        }
    }
    if (tid == 0) o[0] = (uint8_t)g.method;  // signal_packer_base.cpp:83
    for (uint32_t i = tid; i < g.hdr_len; i += 256) o[1 + i] = means_hdr[(size_t)b * g.hdr_len + i];  // :86-91
    if (tid < nb) {
        const uint32_t k = tid;
        const uint64_t pstart = head + 8ull * k + s_plane_end[k];
        const uint64_t plen = 4ull + (s_plane_end[k + 1] - s_plane_end[k]);  // hzr stream = master header + blocks
        store_le32(o + pstart, (uint32_t)plen);                               // base.cpp:78
        store_le32(o + pstart + 4, g.N);                                      // hzr_encode.c:521-522
    }
}

// ===========================================================================
// k_encode
// ===========================================================================
// The payload image lives in LDS as plain consecutive words.  Logical word 0 holds the CRC prefix X, the payload starts at
// byte 4: the image IS the virtual CRC input V = X || payload.  Both access patterns are bank-conflict free without
// padding: consecutive words by consecutive lanes (emit, copy-out), and the CRC reads word-strided -- lane tid owns
// the virtual words tid, tid + 1024, ... counted from the END of V (tools/kernel_model.py:crc_strided).
constexpr uint32_t kStageWords = kHzrBlock / 4 + 32;  // X + payload + read slack
constexpr uint32_t kStagePhys = kStageWords + 2;

constexpr uint32_t kLightPayload = 16384;    // bytes: below it the image words from kTokQueueBase on are free (sparse-row queues)
constexpr uint32_t kTokQueueBase = 4200;     // stage word (> (16384 + 4) / 4 + 24)

// byte q of the image (q = 0..3: X, q >= 4: payload byte q-4)
__device__ __forceinline__ uint32_t stage_byte(const uint32_t* stage, uint32_t q) { return (stage[(q >> 2)] >> ((q & 3u) * 8)) & 0xFFu; }

// ===========================================================================
// container packing (rspt_hip_pack_batch_dev)
// ===========================================================================
constexpr uint64_t kPackMagic = 0x4B43415054505352ull;  // "RSPTPACK"
constexpr uint32_t kPackHead = 32;                      // magic, nblocks, payload bytes, nb | bad << 32
constexpr uint64_t kPackLenMask = (1ull << 56) - 1ull;  // index length word: length | nb << 56 | invalid << 63

// The index is self-describing per stream: nb escalates inside a batch and every rank escalates on its own, so the
// plane count of stream i (nbuse[i], the reference's nr_bytes_to_compress_ at that call) travels in its length word.
// A stream that did not fit dst_stride (bit 63 of sizes[i]: nothing was written) becomes an empty, flagged entry.
__global__ __launch_bounds__(1024) void k_pack_index(const uint64_t* __restrict__ sizes, uint32_t nblocks, const uint32_t* __restrict__ nb_state,
                                                    const uint32_t* __restrict__ nbuse, uint8_t* __restrict__ packed,
                                                    uint64_t* __restrict__ total, uint32_t nb_fixed) {  // nb_fixed != 0: every entry's nb (bare streams: 1)
    __shared__ uint64_t s_w[16];
    __shared__ uint64_t s_carry;
    __shared__ uint32_t s_bad;
    uint64_t* head = reinterpret_cast<uint64_t*>(packed);
    uint64_t* index = head + 4;
    const uint32_t tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    if (tid == 0) {
        s_carry = 0;
        s_bad = 0;
    }
    __syncthreads();
    for (uint32_t base = 0; base < nblocks; base += 1024) {
        const uint32_t i = base + tid;
        const uint64_t sz = i < nblocks ? sizes[i] : 0ull;
        const bool bad = (sz >> 63) != 0;
        const uint64_t len = bad ? 0ull : sz;
        if (bad) atomicAdd(&s_bad, 1u);
        const uint64_t v = (len + 15ull) & ~15ull;
        uint64_t inc = v;
#pragma unroll
        for (int dd = 1; dd < 64; dd <<= 1) {
            const uint64_t o = (uint64_t)__shfl_up((long long)inc, dd, 64);
            if (l >= (uint32_t)dd) inc += o;
        }
        if (l == 63) s_w[w] = inc;
        __syncthreads();
        uint64_t pre = s_carry, tot = s_carry;
        for (uint32_t q = 0; q < 16; ++q) {
            if (q < w) pre += s_w[q];
            tot += s_w[q];
        }
        if (i < nblocks) {
            index[2 * i] = pre + inc - v;
            index[2 * i + 1] = len | ((uint64_t)((nb_fixed ? nb_fixed : nbuse[i]) & 0xFu) << 56) | (bad ? (1ull << 63) : 0ull);
        }
        __syncthreads();
        if (tid == 0) s_carry = tot;
        __syncthreads();
    }
    if (tid == 0) {
        head[0] = kPackMagic;
        head[1] = nblocks;
        head[2] = s_carry;
        head[3] = (uint64_t)*nb_state | ((uint64_t)s_bad << 32);
        *total = kPackHead + 16ull * nblocks + s_carry;
    }
}

// grid (chunks, nblocks): 16-byte units of stream b, strided over the chunk workgroups
__global__ __launch_bounds__(256) void k_pack_copy(const uint8_t* __restrict__ dst, uint64_t dst_stride, uint32_t nblocks,
                                                  uint8_t* __restrict__ packed) {
    const uint32_t b = blockIdx.y;
    const uint64_t* index = reinterpret_cast<const uint64_t*>(packed) + 4;
    const uint64_t off = index[2 * b], len = index[2 * b + 1] & kPackLenMask;  // (0 for a flagged stream: nothing to copy)
    const uint8_t* s = dst + (size_t)b * dst_stride;
    uint8_t* o = packed + kPackHead + 16ull * nblocks + off;
    const uint64_t units = (len + 15) >> 4;
    for (uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (uint64_t)gridDim.x * 256) {
        uint4 v = *reinterpret_cast<const uint4*>(s + u * 16);
        if (u * 16 + 16 > len) {  // zero the padding so that containers are reproducible
            const uint32_t keep = (uint32_t)(len - u * 16);
            uint32_t x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t lo = q * 4;
                x[q] = keep >= lo + 4 ? x[q] : keep <= lo ? 0u : (x[q] & ((1u << ((keep - lo) * 8)) - 1u));
            }
            v = make_uint4(x[0], x[1], x[2], x[3]);
        }
        *reinterpret_cast<uint4*>(o + u * 16) = v;
    }
}

}  // namespace rspt
