/*
 * rspt_hip.h -- C ABI of the MI355X (gfx950) signal_packer hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch
 * types.  The reference has no FFI of its own (it is a single C++ library);
 * the entry points below are what its i_signal_packer factories and
 * compress()/decompress() virtuals (lib_rspt/signal_packer.h:29-73) bind to
 * when the path runs on the GPU -- include/signal_packer.h holds the
 * API-identical C++ classes that call them, INTEGRATION.md shows the
 * reference-side binding.
 *
 * Conventions: every function returns RSPT_HIP_OK (0) or a negative
 * rspt_hip_status; nothing throws across this boundary.  A handle owns its
 * device workspace and one HIP stream and is not thread-safe (one handle per
 * host thread), exactly like a reference packer instance
 * (signal_packer_base.h:20-21 scratch tensors).  There is no CPU fallback: if
 * no gfx950 device is usable, create() fails.
 */
#ifndef RSPT_HIP_H_
#define RSPT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rspt_hip_packer rspt_hip_packer;

/* Factory selector -- NOT the stream's method byte (which is 0,0,1,2).
 * Replaces i_signal_packer::new_hzr / new_xdelta_hzr / new_dct / new_hadamard
 * (lib_rspt/signal_packer.h:59-69). */
enum rspt_hip_kind {
    RSPT_HIP_KIND_HZR = 0,        /* lib_signalpacker/signal_packer_hzr.cpp:34-68        */
    RSPT_HIP_KIND_XDELTA_HZR = 1, /* lib_signalpacker/signal_packer_xdelta_hzr.cpp:34-88 */
    RSPT_HIP_KIND_DCT = 2,        /* lib_signalpacker/signal_packer_dct.cpp:36-156       */
    RSPT_HIP_KIND_HADAMARD = 3,   /* lib_signalpacker/signal_packer_hadamard.cpp:35-107  */
    RSPT_HIP_KIND_BYTES = 4       /* lib_hzr/libhzr.h: hzr_encode / hzr_decode on a raw byte buffer (see below) */
};

/* RSPT_HIP_KIND_BYTES -- libhzr itself (lib_hzr/libhzr.h), without a sample packer around it.
 * Create with rspt_hip_packer_create(&p, RSPT_HIP_KIND_BYTES, bps = 1, nch = 1, ns = in_size, nb (ignored), device),
 * 1 <= in_size < 2^31; any other bps or nch is RSPT_HIP_ERR_ARG.  A handle is bound to ONE buffer size (the fixed-size
 * contract of every handle here).  A block is a buffer of in_size bytes and its stream is exactly what
 * hzr_encode(in, in_size, ...) writes: u32 LE in_size, then the hzr blocks -- no method byte, no plane length word.
 *   rspt_hip_block_bytes = in_size;  rspt_hip_max_compressed_size = rspt_hip_hzr_max_compressed_size(in_size);
 *   rspt_hip_current_nb = 1;  rspt_hip_set_nb = RSPT_HIP_ERR_ARG;  container index entries carry nb = 1.
 * Every entry point that takes a handle keeps its contract: the host calls (RSPT_HIP_ERR_DST_TOO_SMALL stands in for
 * hzr_encode's HZR_FAIL on a short buffer), the _many pipelines, the feed, the device batch calls, the container calls,
 * rspt_hip_set_verify, profiling.  In the device batch form buffer b starts at d_src + b * in_size -- at any byte alignment
 * when in_size is not a multiple of 16; only the batch base keeps the 16-byte rule -- and decodes to d_dst + b * in_size.
 * Decode differs from hzr_decode in five points, the first two because a handle has one size:
 *   - a stream whose master header names another decoded size than in_size is malformed (RSPT_HIP_ERR_CORRUPT, bit 63 of
 *     d_consumed[b]); hzr_decode accepts any size up to out_size;
 *   - d_consumed[b] / *src_len report the bytes the stream spans.  hzr_decode's "decoder reached the end of the input"
 *     test (hzr_decode.c:668) is the caller's comparison of that value with the length it holds.
 *   - a Fill block whose length field is not 1 is malformed.  No encoder writes one; hzr_decode would read the fill byte and
 *     go on right behind it, hzr_verify would step over the whole length, so such a stream has no framing to follow.
 *   - stricter than hzr_decode: a Huffman tree with a code of 32 bits or more is malformed.  hzr_decode walks codes of any
 *     length; no block of 65536 bytes gives an optimal code that long (lengths from 24 up need Fibonacci counts).
 *   - stricter than hzr_decode: a Huffman tree that holds a leaf with a symbol above 260 is malformed, used or not.
 *     hzr_decode fails only when such a symbol is decoded.
 *   (Both hold for the hzr blocks inside every packer kind's streams as well: rspt_hip_decompress_batch_dev.)
 * The filter, median, peak, PRDN and converter stages see such a handle as the shape (bps 1, nch 1, ns in_size). */

/* Test hook, OR-ed into `kind` at create: a dct packer takes the fp64 FFT path also where the bit-exact dense-table path
 * would run (ns = 2^k <= 8192), so that the two can be compared with each other (tests/test_gpu_dct_fft.py). */
#define RSPT_HIP_DCT_FORCE_FFT 0x100

enum rspt_hip_status {
    RSPT_HIP_OK = 0,
    RSPT_HIP_ERR_ARG = -1,         /* bad kind / sizes (bps not 1..4, nb not 1..4, ns not 2^k for hadamard ...) */
    RSPT_HIP_ERR_NO_DEVICE = -2,   /* no usable gfx950 device; there is no CPU path */
    RSPT_HIP_ERR_ALLOC = -3,       /* device or host allocation failed */
    RSPT_HIP_ERR_LAUNCH = -4,      /* a HIP call or kernel launch failed (see rspt_hip_last_hip_error) */
    RSPT_HIP_ERR_DST_TOO_SMALL = -5, /* compressed block does not fit dst_max_len / dst_stride */
    RSPT_HIP_ERR_CORRUPT = -6,     /* decompress: malformed stream */
    RSPT_HIP_ERR_UNSUPPORTED = -7, /* shape outside what the kernels handle (documented in DESIGN.md) */
    RSPT_HIP_ERR_BUSY = -8         /* rspt_hip_feed_push: every slot of the feed is in flight (poll, then push again) */
};

const char* rspt_hip_status_string(int status);
/* hipError_t of the last failing HIP call on this handle (0 if none). */
int rspt_hip_last_hip_error(const rspt_hip_packer* p);

/* Number of gfx950 devices visible to this process (0 if none). */
int rspt_hip_device_count(void);

/* Constructor.  Replaces the packer constructors
 * (signal_packer_xdelta_hzr.cpp:42-50, _hzr.cpp:42-49, _hadamard.cpp:47-55,
 * _dct.cpp:49-58): same meaning of (bytes_per_sample, nr_channels,
 * nr_samples_per_channel, nr_bytes_to_encode); `nb` is read by
 * RSPT_HIP_KIND_XDELTA_HZR only.  `device` is the HIP device ordinal.
 * Shape limits: nch * ns < 2^31 (RSPT_HIP_ERR_ARG: the reference indexes with int); nch <= 65535, the reference's own limit --
 * its converters convert_native_to_i32 / convert_i32_to_native count channels in a uint16_t (utils.cpp:57, 129), so 65536
 * channels never terminate there -- and the ns limits of hadamard and dct: RSPT_HIP_ERR_UNSUPPORTED beyond. */
int rspt_hip_packer_create(rspt_hip_packer** out, int kind, size_t bps, size_t nch, size_t ns, size_t nb, int device);

/* Replaces i_signal_packer::delete_* (signal_packer.h:60-72). */
void rspt_hip_packer_destroy(rspt_hip_packer* p);

/* i_signal_packer::compress (signal_packer.h:44), host buffers.
 * src = bps*nch*ns bytes, interleaved sample-major little-endian.
 * Fails with RSPT_HIP_ERR_DST_TOO_SMALL instead of the reference's undefined
 * result when the stream does not fit dst_max_len. */
int rspt_hip_compress(rspt_hip_packer* p, const void* src_host, void* dst_host, size_t dst_max_len, size_t* dst_len);

/* i_signal_packer::decompress (signal_packer.h:57), host buffers.
 * *src_len is an OUTPUT (bytes consumed), as in the reference. */
int rspt_hip_decompress(rspt_hip_packer* p, const void* src_host, size_t* src_len, void* dst_host);

/* The same for a caller that knows how many bytes are readable at src_host (no counterpart in the reference, whose decompress
 * trusts the stream's own length fields -- as rspt_hip_decompress does, up to the longest stream the format allows, 65536 bytes
 * of payload for every hzr block whatever the block decodes to (another writer's Huffman block may be longer than its output, so
 * this is more than rspt_hip_max_compressed_size where the last block is short): a damaged length field of a stream from an
 * untrusted source can send it past the end of a shorter buffer).  Nothing beyond src_host + src_cap is read; a stream whose
 * framing says otherwise is RSPT_HIP_ERR_CORRUPT. */
int rspt_hip_decompress_bounded(rspt_hip_packer* p, const void* src_host, size_t src_cap, size_t* src_len, void* dst_host);

/* Worst-case stream size of ONE block for this packer, allowing for nb
 * escalation up to 4 (1 + header + nb*(4 + hzr_max_compressed_size(nch*ns)),
 * hzr_encode.c:489-497, signal_packer_base.cpp:83-95). */
size_t rspt_hip_max_compressed_size(const rspt_hip_packer* p);

/* Input bytes per block: bps*nch*ns. */
size_t rspt_hip_block_bytes(const rspt_hip_packer* p);

/* hzr_max_compressed_size (hzr_encode.c:489-497): 4 + n + 7 * ceil(n / 65536); 4 for n = 0.  Host only: no handle, no device. */
size_t rspt_hip_hzr_max_compressed_size(size_t uncompressed_size);

/* Current nr_bytes_to_compress_ (signal_packer_xdelta_hzr.cpp:39,66): the
 * state that mutates on escalation and must match between compressor and
 * decompressor because it is not in the stream.  Synchronises the stream. */
unsigned rspt_hip_current_nb(rspt_hip_packer* p);
/* Set it (a decoder fed streams from another instance needs this). */
int rspt_hip_set_nb(rspt_hip_packer* p, unsigned nb);

/* The quantiser of the two lossy packers: the constants a user of the reference edits and rebuilds with -- `quality`
 * (signal_packer_dct.cpp:39 = 128, signal_packer_hadamard.cpp:37 = 1) and nr_bytes_to_compress_ (2 and 3), the number of
 * low bytes of every stored value that reach the stream.  RSPT_HIP_KIND_DCT and RSPT_HIP_KIND_HADAMARD only; a fresh handle
 * has the reference's constants, and streams and decoded samples equal those of the reference rebuilt with the same two.
 *   hadamard  stores (int)((double)WHT(x - mean)[i] / ((double)n / quality)) and decodes (int)((double)WHT(y)[i] / quality)
 *             + mean (fwht.c:30-40): a LARGER quality is FINER, quality = n stores the raw transform.
 *   dct       scales the forward sum by Cs[i] * sqrt(2/n) / quality and the inverse by sqrt(2/n) * quality
 *             (signal_packer_dct.cpp:84, 97): a LARGER quality is COARSER.
 * Neither number is in the stream: like nb of the xdelta packer they are state that compressor and decompressor must share
 * (rspt_hip_set_nb stays RSPT_HIP_ERR_ARG for these kinds; container index entries carry nb).  The lossy packers never verify or
 * escalate: a value that does not fit nb bytes loses its high bytes, as in the reference.
 * RSPT_HIP_ERR_ARG, and the handle unchanged: another kind, nb outside 1..4, a quality that is not finite and > 0 or that leaves
 * n / quality (hadamard) or one of the three dct scales not finite or zero, an open feed.  Ordered like rspt_hip_set_nb: it
 * synchronises the device, and holds for every call on the handle from then on.  rspt_hip_max_compressed_size follows nb
 * (take buffer sizes and strides from it after the call; a change of nb releases the staging of the _many pipelines, which
 * the next of those calls makes again). */
int rspt_hip_set_quantizer(rspt_hip_packer* p, double quality, unsigned nb);
int rspt_hip_get_quantizer(const rspt_hip_packer* p, double* quality, unsigned* nb);

/* Decompress normally trusts the stream like the reference does (hzr_decode.c:343 skips the block CRCs).  With
 * verify on, every Huffman / PlainCopy block's CRC-32C is recomputed on the device and compared with its header
 * (what hzr_verify does, hzr_decode.c:569-624); a mismatch makes the call return RSPT_HIP_ERR_CORRUPT (batch
 * form: bit 63 of d_consumed[b]).  Off by default. */
int rspt_hip_set_verify(rspt_hip_packer* p, int on);

/* Byte order of the samples (default 0 = little-endian, what every reference packer passes: signal_packer_xdelta_hzr.cpp:54).
 * With big_endian != 0 compress reads samples whose bytes are reversed -- convert_native_to_i32(..., reverse_byte_order =
 * true), lib_signalpacker/utils.cpp:127-137,145-154,162-170 -- and decompress writes them that way (convert_i32_to_native,
 * utils.cpp:57-64,77-85,97-104): a 24-bit ADC feed in network byte order needs no host pass.  The streams are those of the
 * byte-reversed (little-endian) block. */
int rspt_hip_set_byte_order(rspt_hip_packer* p, int big_endian);

/* Page-locked host memory for the host-pointer entry points: with src / dst in such buffers (16-byte aligned source)
 * rspt_hip_compress has no copy phases at all -- the front end reads the samples across the link as it transforms them and the
 * encoders write the stream into the caller's buffer -- and rspt_hip_decompress writes the samples there from its last kernel;
 * the many-block forms move their data by DMA at link rate instead of through the runtime's pageable staging copies
 * (the acquisition front end of the reference, lib_ring_buffer/ring_buffers.h:150-203 io_buffer, would allocate its
 * slots here).  NULL on failure. */
void* rspt_hip_host_alloc(size_t bytes);
void rspt_hip_host_free(void* p);

/* A sequence of blocks from host memory: what a caller of the reference does one compress() call per block
 * (the call itself: lib_rspt_test/rspt_test.cpp:66-72; a packer is made for ONE block shape, signal_packer.h:60-72, so a
 * recording longer than that is a loop of such calls on the same instance).  nblocks consecutive blocks at src_host
 * (rspt_hip_block_bytes apart); stream i goes to dst_host + i * dst_stride, its length to dst_len[i]; the nb
 * state moves from block to block as in repeated compress() calls.  Chunks of blocks pass through
 * upload | compress | download on three HIP streams, so a long sequence runs at the rate of the slowest
 * stage (the upload over PCIe when src_host is page-locked) instead of at the sum of the three.  Blocking.
 * A stream that does not fit dst_stride: dst_len[i] = the size it needs, nothing copied for it, and the call
 * returns RSPT_HIP_ERR_DST_TOO_SMALL after finishing the others. */
int rspt_hip_compress_many(rspt_hip_packer* p, const void* src_host, size_t nblocks, void* dst_host, size_t dst_stride, size_t* dst_len);

/* The inverse: nblocks streams at src_host + i * src_stride (src_stride <= rspt_hip_max_compressed_size rounded up to 256)
 * -> blocks at dst_host + i * rspt_hip_block_bytes, bytes consumed to consumed[i].  As in decompress() a stream's length is
 * not needed; where the caller knows it, src_len[i] (may be NULL) bounds what is uploaded of stream i -- with 16 MiB blocks
 * and a stride sized for the worst case that is a fifth of the bytes.  All streams are decoded with the packer's current nb
 * (rspt_hip_set_nb), like successive decompress() calls.  Same three-stage pipeline; here the download bounds it.  A stream
 * that does not decode: consumed[i] = 0 and the call returns RSPT_HIP_ERR_CORRUPT after finishing the others. */
int rspt_hip_decompress_many(rspt_hip_packer* p, const void* src_host, size_t src_stride, const size_t* src_len, size_t nblocks, void* dst_host,
                             size_t* consumed);

/* ---- a feed of blocks that arrive over time (the acquisition side: lib_ring_buffer/ring_buffers.h:150-203 io_buffer hands
 * a consumer one filled buffer after the other; the consumer's loop is rspt_test.cpp:66-72, one compress() per block) ----------
 * Non-blocking: push a block when it is there, poll for finished streams when convenient.  Behind it the same three-stage
 * pipeline as rspt_hip_compress_many (upload | compress | download on three HIP streams), over a ring of `slots` groups of
 * `blocks_per_launch` blocks; the streams are byte for byte those of successive compress() calls in push order (the nb state
 * moves from block to block).
 *   rspt_hip_feed_begin   allocate the ring (slots >= 2; blocks_per_launch >= 1: 1 = lowest latency, more = higher rate)
 *   rspt_hip_feed_push    queue one block: src_host (rspt_hip_block_bytes() bytes; page-locked memory from rspt_hip_host_alloc
 *                         uploads by DMA) -> its stream will be written to dst_host (dst_cap bytes).  Both must stay valid
 *                         until the block is reported by rspt_hip_feed_poll.  Returns RSPT_HIP_OK, or RSPT_HIP_ERR_BUSY when
 *                         every slot is in flight (poll, then push again) -- it never waits.  A group is launched when it is
 *                         full; rspt_hip_feed_submit launches a partly filled one (when no more blocks are expected soon).
 *   rspt_hip_feed_poll    report ONE finished block, in push order: returns 1 and sets *seq (0, 1, 2, ... in push order),
 *                         *dst_len and *status (RSPT_HIP_OK, or RSPT_HIP_ERR_DST_TOO_SMALL with *dst_len = the size needed
 *                         and nothing copied; or the status of a launch that failed -- rspt_hip_feed_push / _submit returned it
 *                         when it happened -- for every block of that group, with *dst_len = 0); returns 0 when none is
 *                         ready yet; never waits.
 *   rspt_hip_feed_flush   submit what is queued and wait until everything pushed so far can be polled
 *   rspt_hip_feed_end     flush, drop unpolled results, free the ring.
 * One feed per handle; while a feed is open the batch and many-block entry points of the handle return RSPT_HIP_ERR_ARG. */
int rspt_hip_feed_begin(rspt_hip_packer* p, size_t blocks_per_launch, size_t slots);
int rspt_hip_feed_push(rspt_hip_packer* p, const void* src_host, void* dst_host, size_t dst_cap);
int rspt_hip_feed_submit(rspt_hip_packer* p);
int rspt_hip_feed_poll(rspt_hip_packer* p, size_t* seq, size_t* dst_len, int* status);
int rspt_hip_feed_flush(rspt_hip_packer* p);
int rspt_hip_feed_end(rspt_hip_packer* p);

/* ---- device-resident, batched forms (bench, multi-GPU shards) ------------ */

/* Grow the workspace so that up to max_blocks blocks can go through one
 * launch sequence.  Called implicitly by the batch entry points; call it
 * yourself to keep allocation out of a timed region. */
int rspt_hip_reserve(rspt_hip_packer* p, size_t max_blocks);

/* Compress nblocks independent blocks that are resident in device memory.
 * Semantics = nblocks successive compress() calls on one packer instance
 * (including the persistent nb escalation, in block order).
 *   d_src      nblocks * rspt_hip_block_bytes() bytes, blocks back to back
 *   d_dst      block b's stream is written at d_dst + b*dst_stride
 *   d_sizes    nblocks uint64: stream length of block b; if it would not fit
 *              dst_stride nothing is written for that block and bit 63 is set
 *   stream     hipStream_t (as void*) to enqueue on; NULL is the HIP null
 *              stream, as everywhere in HIP.  rspt_hip_stream() returns the
 *              handle's own stream for callers that want that one.
 * Asynchronous: returns after enqueueing.
 * Ordering contract of a handle: it is ONE packer instance (one workspace, one nb state), so successive batch calls on it
 * must be stream-ordered -- the same `stream` for all of them, or each call ordered behind the previous one by an event.
 * (Inside, the per-call scratch that must start from zero exists twice and the kernels of call i zero the copy that call
 * i+1 works in; the small-block encoder runs on a side stream of the handle, forked from and joined to `stream` inside the
 * call.)  Two calls racing on different streams would share planes, counters and that zeroing.  One host word is read
 * without synchronisation, by design: the small-block count a RECENT batch left in page-locked memory only decides whether
 * the side stream is used at all (a batch shape without small blocks skips the fork/join); a stale value costs a few
 * microseconds, never correctness. */
int rspt_hip_compress_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, void* d_dst, size_t dst_stride,
                                uint64_t* d_sizes, void* stream);

/* Decompress nblocks streams resident in device memory (stream b at
 * d_src + b*src_stride) into d_dst (nblocks * rspt_hip_block_bytes() bytes).
 * d_consumed[b] = bytes of stream b used; bit 63 set = malformed stream.
 * Every valid stream decodes, whatever writer made it -- any tree shape, duplicate or unused leaves, any tokenisation, any pad
 * bits -- with two limits that are stricter than hzr_decode (lib_hzr/hzr_decode.c), which takes such streams: a block whose
 * Huffman tree has a code of 32 bits or more, and a block whose tree holds a leaf symbol above 260 even where no code uses
 * it, are malformed here (bit 63).  Neither encoder writes either; tests/test_hzr_foreign.py holds the decoder to both. */
int rspt_hip_decompress_batch_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, size_t nblocks, void* d_dst,
                                  uint64_t* d_consumed, void* stream);

/* ---- a quality ladder and a per-block choice: the lossy packers' quality chosen block by block, on the device ----
 * ladder    host array of nladder = 1..8 qualities.  Every entry is validated as rspt_hip_set_quantizer validates its quality for
 *           the handle's kind and ns (RSPT_HIP_ERR_ARG, nothing launched), and turned into the kernels' quantiser on the host
 *           with the same arithmetic; the entries travel as kernel arguments -- nothing is copied to the device and nothing is
 *           allocated per call.
 * d_choice  device array of nblocks uint32 (4-byte aligned): block b takes ladder[d_choice[b]].
 * Block b's stream, d_sizes[b] and decoded samples are byte for byte what rspt_hip_set_quantizer(p, ladder[d_choice[b]], nb)
 * followed by rspt_hip_compress_batch_dev / rspt_hip_decompress_batch_dev gives for that block, nb being the handle's current
 * one for every block.  An entry of quality 1 on a hadamard handle gives the all-integer kernels' stream: (int)((double)y / n)
 * is the truncating division for n = 2^k.  The handle's own quality is neither read nor changed.  The choice is not in the
 * stream: the decoder must be given the one the encoder had.
 * d_choice[b] >= nladder: nothing is written for block b and d_sizes[b] is exactly bit 63 (compress) / bit 63 is added to
 * d_consumed[b] (decompress); the other blocks are not affected.
 * RSPT_HIP_KIND_HADAMARD at every row length, and RSPT_HIP_KIND_DCT where the dense table runs.  RSPT_HIP_ERR_UNSUPPORTED, before
 * anything is launched: a dct handle on the FFT path (rows beyond the dense table, or RSPT_HIP_DCT_FORCE_FFT) -- the FFT kernels
 * do not read a ladder yet -- and every other kind.  Everything else -- the ordering contract, the refusals, the 16-byte
 * d_src, the workspace of rspt_hip_reserve -- is as in rspt_hip_compress_batch_dev / rspt_hip_decompress_batch_dev; a
 * dst_stride of 2^32 bytes per 65536 samples of a block or more is RSPT_HIP_ERR_ARG (no stream is a thousandth of that). */
int rspt_hip_compress_batch_ladder_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder,
                                       const uint32_t* d_choice, void* d_dst, size_t dst_stride, uint64_t* d_sizes, void* stream);
int rspt_hip_decompress_batch_ladder_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, size_t nblocks, const double* ladder,
                                         size_t nladder, const uint32_t* d_choice, void* d_dst, uint64_t* d_consumed, void* stream);

/* ---- compress to a PRDN target: the smallest stream of a ladder whose PRDN is at most target_prdn, block by block ----
 * The rule.  For block b and ladder entry k: o is the native block, d_k what decompress(compress(o)) gives at ladder[k] and the
 * handle's nb, and (prdn_k, mse_k, path_k) what rspt_hip_prdn_batch_dev(o, d_k) gives.  Entry k MEETS THE TARGET iff
 * path_k == 0 and (mse_k == 0 or prdn_k <= target_prdn): a NaN never meets it, and neither does a candidate whose figure needs
 * the sequential path (an exact sum above 2^53).  d_choice[b] is the first k in ladder order that meets the target -- order
 * the ladder coarse to fine; nothing assumes that PRDN is monotonic in it -- and nladder - 1 if no entry does.  d_prdn[b]
 * (optional) is prdn of the chosen entry, bit for bit rspt_hip_prdn_batch_dev's where its path is 0, and +inf where it is 1.
 * Streams and sizes are then those of rspt_hip_compress_batch_ladder_dev with that d_choice, which is the caller's to keep: the
 * decoder needs it.
 * The candidates run the kernels of a compress and a decompress call without the hzr stage (it changes no value): the front
 * end once, then per entry the forward transform, the cut to nb bytes, the way back, the cut to the sample width and the PRDN
 * kernels against the kept original.
 * target_prdn must be finite and > 0 (RSPT_HIP_ERR_ARG); ladder, kinds and refusals as rspt_hip_compress_batch_ladder_dev;
 * nblocks <= 65535.  Asynchronous on `stream`, no host synchronisation inside (beyond rspt_hip_reserve's when the workspace
 * grows), stream-ordered with every other call on the handle; the handle's own quantiser is neither used nor changed.
 * d_work: device memory, 16-byte aligned, at least the bytes rspt_hip_compress_target_work_bytes names for (nblocks, nladder)
 * -- all scratch beyond the handle's workspace; contents unspecified afterwards. */
int rspt_hip_compress_target_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);
int rspt_hip_compress_target_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder,
                                       double target_prdn, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice,
                                       double* d_prdn, void* d_work, void* stream);
/* The candidates take one of two routes, picked from the handle's shape alone; both give the same d_choice, d_prdn and streams
 * bit for bit.  general: every supported shape, the existing kernels per ladder entry as described above.  fused: hadamard rows
 * of up to 8192 points with nch * ns < 2^22 (under which every reference sum of the PRDN is exact) -- one kernel reads each row
 * once, keeps its mean and its transform in LDS and walks the ladder there, and the PRDN stage's own finishing kernel turns its
 * exact sums into the figures.  For tests: route 0 = the host's choice (default), 1 = general, 2 = fused
 * (RSPT_HIP_ERR_UNSUPPORTED where the fused probe does not run; RSPT_HIP_ERR_ARG for any other value). */
int rspt_hip_debug_set_target_route(rspt_hip_packer* p, int route);

/* ---- compress to a byte budget: the finest entry of a ladder whose stream is at most budget bytes, block by block ----
 * The rule.  For block b and ladder entry k: size_k(b) is the number rspt_hip_compress_batch_ladder_dev writes to d_sizes[b] when
 * d_choice[b] = k and every stream fits the stride -- the length of the stream at ladder[k] and the handle's nb; bit 63 is never
 * set in it.  budget(b) = d_budget ? d_budget[b] : budget_bytes; any value is allowed, 0 included.  d_choice[b] is the HIGHEST
 * index k with size_k(b) <= budget(b) -- order the ladder coarse to fine, as for the PRDN target; nothing assumes that the sizes
 * are sorted in it, and <= is inclusive -- and, if no entry fits, the entry of the smallest size, the lowest index among equals:
 * the caller sees the miss as d_sizes[b] > budget(b).  Streams, d_sizes and (with d_choice) the decoded samples are then byte
 * for byte those of rspt_hip_compress_batch_ladder_dev / rspt_hip_decompress_batch_ladder_dev with that d_choice, which is the
 * caller's to keep: the decoder needs it.  A chosen stream that does not fit dst_stride is flagged as the ladder call flags it
 * (bit 63 of d_sizes[b], nothing written); dst_stride plays no part in the choice.
 * d_cand_sizes (optional): the whole table, size_k(b) at d_cand_sizes[k * nblocks + b].
 * A candidate runs a compress call as far as the Huffman trees, behind which its size is known, and not a step further: no
 * stream of a candidate is laid out or encoded, and the only output buffer is the caller's.
 * budget_bytes is a size_t, which has 64 bits wherever this library is built.  ladder, kinds and refusals as
 * rspt_hip_compress_target_batch_dev: RSPT_HIP_ERR_UNSUPPORTED for every kind and path without a ladder, nothing launched;
 * RSPT_HIP_ERR_ARG for a bad ladder, an open feed, a null pointer, nblocks > 65535, a dst_stride of 2^32 bytes per 65536 samples
 * or more, a d_src or d_work off a 16-byte boundary, a d_choice off a 4-byte one, a d_budget or d_cand_sizes off an 8-byte one.
 * Asynchronous on `stream`, no host synchronisation inside (beyond rspt_hip_reserve's when the workspace grows) and nothing
 * copied to the host; stream-ordered with every other call on the handle; the handle's own quantiser is neither read nor
 * changed.
 * d_work: device memory, 16-byte aligned, at least the bytes rspt_hip_compress_budget_work_bytes names for (nblocks, nladder) --
 * the table of sizes, 8 bytes per (entry, block); contents unspecified afterwards. */
int rspt_hip_compress_budget_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);
int rspt_hip_compress_budget_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder,
                                       size_t budget_bytes, const uint64_t* d_budget, void* d_dst, size_t dst_stride, uint64_t* d_sizes,
                                       uint32_t* d_choice, uint64_t* d_cand_sizes, void* d_work, void* stream);
/* The candidates take one of two routes; both give the same table, d_choice and streams bit for bit.  general: every supported
 * shape, one pass per ladder entry of the kernels of a ladder call whose every choice is that entry, stopped behind the trees.
 * batched: hadamard rows of up to 8192 points with nladder * nblocks <= 65535 -- the handle's workspace grows to
 * nladder * nblocks blocks (rspt_hip_reserve), one kernel reads each row once, keeps its transform in LDS and writes every
 * entry's coefficients, and ONE pass of the plane, histogram and tree kernels runs over all of them.  For tests: route 0 = the
 * host's choice (default), 1 = general, 2 = batched (RSPT_HIP_ERR_UNSUPPORTED where the handle's shape does not take it, and
 * from the two entries above for a call of more than 65535 entry-blocks while it is forced; RSPT_HIP_ERR_ARG for any other
 * value). */
int rspt_hip_debug_set_budget_route(rspt_hip_packer* p, int route);

/* ---- compress a batch to one byte total: the lowest common PRDN level at which the whole batch fits ----
 * A budget arrives for a batch -- a link, a file, a gather buffer has room for total_bytes of it -- and not per block.  The rule
 * is minimax: every block is taken to the same PRDN level T, each at its smallest stream that meets T, and T is the lowest level
 * at which the streams add up to at most total_bytes.  It is exact: no floating-point sum over blocks decides anything, levels
 * compare as doubles that are bit-identical with rspt_hip_prdn_batch_dev's.
 * The rule.  For block b and ladder entry k: size_k(b) is rspt_hip_compress_budget_batch_dev's size_k(b), and (prdn_k(b),
 * mse_k(b), path_k(b)) is rspt_hip_compress_target_batch_dev's triple, what rspt_hip_prdn_batch_dev(o, d_k) gives.
 *   Entry k of block b is RATED iff path_k(b) == 0 and (mse_k(b) == 0 or prdn_k(b) is not a NaN).  A rated entry's FIGURE is
 *   f_k(b) = +0.0 if mse_k(b) == 0, else prdn_k(b); it may be +inf (a constant block with a lossy error) and is never negative.
 *   The figure of an unrated entry is reported as a NaN (0x7FF8000000000000).  A block is rated iff it has a rated entry.
 *   At a level T in [0, +inf], pick_T(b) is the rated entry of smallest size among those with f_k(b) <= T (inclusive), the
 *   lowest index among equal sizes.  An unrated block takes its smallest stream at every level, the lowest index among equals,
 *   and its figures never count.  T is ADMISSIBLE iff every rated block has a pick at T.  cost(T) is the sum over all blocks of
 *   the size of the pick (of the smallest stream, for an unrated block), in 64 bits.  cost is non-increasing in T over
 *   admissible levels and admissibility is monotone in T.
 *   T* is the smallest admissible T with cost(T) <= total_bytes, and +inf -- which is always admissible -- if there is none.
 *   T* is always one of the figures, or +inf; with no rated block at all T* is +0.0, whatever total_bytes.
 * d_choice[b] = pick_T*(b); d_level[0] = T*; d_total[0] = cost(T*).  The caller sees a miss as d_total[0] > total_bytes; a T* of
 * +inf alone is not one.  Any total_bytes is allowed, 0 and 2^64 - 1 included, and nothing assumes that sizes or figures are
 * sorted along the ladder.  Every (block, entry) figure is a level of its own, and passing from one level to the next moves the
 * picks of the blocks that have an entry at exactly that figure: the slack left under total_bytes is at most those blocks' steps.
 * Streams, d_sizes and (with d_choice) the decoded samples are byte for byte those of rspt_hip_compress_batch_ladder_dev /
 * rspt_hip_decompress_batch_ladder_dev with that d_choice, which is the caller's to keep.  A chosen stream that does not fit
 * dst_stride is flagged as the ladder call flags it (bit 63 of d_sizes[b], nothing written); dst_stride plays no part in the rule.
 * d_prdn[b] (optional): the figure of the chosen entry -- so +0.0 where its mse is 0, where the PRDN target entry reports the
 * PRDN stage's own value -- and, as there, +inf where its path is 1.
 * d_cand_sizes, d_cand_figs (optional): the two tables, size_k(b) and the figure of entry k of block b at [k * nblocks + b].
 * d_level, d_total, d_prdn, d_cand_sizes and d_cand_figs are optional (NULL) and, if given, 8-byte aligned.
 * Identity: on a ladder along which every block's sizes ascend strictly and every block's figures descend strictly, d_choice[b]
 * is rspt_hip_compress_target_batch_dev's at target_prdn = T*, for every block that has an entry meeting T*.
 * Kinds, ladder validation, the open feed, nblocks <= 65535, the dst_stride bound and the alignments of d_src, d_work (16 bytes)
 * and d_choice (4 bytes) are refused exactly as rspt_hip_compress_budget_batch_dev refuses them: RSPT_HIP_ERR_UNSUPPORTED where
 * there is no ladder (the FFT dct and every other kind), RSPT_HIP_ERR_ARG for the rest, nothing launched.
 * Asynchronous on `stream`, no host synchronisation inside (beyond rspt_hip_reserve's when the workspace grows) and nothing
 * copied to the host; stream-ordered with every other call on the handle; the handle's own quantiser is neither read nor changed.
 * d_work: device memory, 16-byte aligned, at least the bytes rspt_hip_compress_total_work_bytes names for (nblocks, nladder) and
 * the route a call would take now -- all scratch beyond the handle's workspace; contents unspecified afterwards. */
int rspt_hip_compress_total_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);
int rspt_hip_compress_total_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, const double* ladder, size_t nladder,
                                      size_t total_bytes, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice,
                                      double* d_level, uint64_t* d_total, double* d_prdn, uint64_t* d_cand_sizes, double* d_cand_figs,
                                      void* d_work, void* stream);
/* The tables are filled on one of two routes; both give the same tables, level, choice and streams bit for bit.  general: every
 * supported shape -- per ladder entry the PRDN target entry's general sequence and the byte budget entry's general sequence, into
 * the two tables; its d_work holds the target entry's whole work area (two planar copies of the batch) beside the tables.  fused:
 * hadamard rows of up to 8192 points with nch * ns < 2^22 and nladder * nblocks <= 65535 -- the handle's workspace grows to
 * nladder * nblocks blocks (rspt_hip_reserve), one kernel reads each row once and leaves, per entry, the coefficients for the size
 * table and the exact sums for the figure table, and ONE pass of the plane, histogram and tree kernels runs over all of them; its
 * d_work holds tables alone, 72 bytes per (entry, block).  For tests: route 0 = the host's choice (default), 1 = general, 2 = fused
 * (RSPT_HIP_ERR_UNSUPPORTED where the handle's shape does not take it, and from the two entries above for a call of more than
 * 65535 entry-blocks while it is forced; RSPT_HIP_ERR_ARG for any other value). */
int rspt_hip_debug_set_total_route(rspt_hip_packer* p, int route);   /* 0 host's pick, 1 general, 2 fused */

/* ---- planar int32 in and out: samples that already live in a [nblocks][nch][ns] int32 matrix skip the native block ----
 * d_planar is what rspt_hip_native_to_i32_batch_dev writes and rspt_hip_i32_to_native_batch_dev reads: block b's channel c at
 * d_planar + (b*nch + c)*ns.  It must be 4-byte aligned; 16-byte aligned buffers take the widest accesses.  The contract is two
 * identities with the entries above:
 *
 *   compress_planar(P)  ==  rspt_hip_compress_batch_dev(rspt_hip_i32_to_native_batch_dev(P))
 *       the streams, d_sizes, the bit-63 "did not fit" flag, the per-block nb and the handle's nb state afterwards are the same,
 *       for every sample packer and sample width.  Only the low bps bytes of each value count: they are cut and sign-extended
 *       before anything else, whatever lies above the sample width changes nothing.  rspt_hip_set_byte_order has no effect
 *       (there are no bytes to order).  d_planar is ONLY READ: the transform packers copy it into the workspace first.
 *   decompress_planar(S)  ==  rspt_hip_native_to_i32_batch_dev(rspt_hip_decompress_batch_dev(S))  with a little-endian handle
 *       every value sign-extended from bps bytes; d_consumed and its bit 63 are those of the native entry, a flagged stream is
 *       never followed, rspt_hip_set_verify applies.  The packed form takes each stream's nb from its index entry, as
 *       rspt_hip_decompress_packed_dev does, and checks the container the same way.
 *
 * Native and planar calls may alternate on one handle in any order: they share the nb state and the workspace, under the
 * ordering contract of rspt_hip_compress_batch_dev.  Channel counts up to the create limit work on both sides (there is no
 * native tile here).  RSPT_HIP_ERR_ARG for a NULL handle or pointer, nblocks == 0, a d_planar off its 4-byte alignment, a
 * RSPT_HIP_KIND_BYTES handle or a handle with an open feed; everything rspt_hip_reserve refuses (more than 65535 blocks) is
 * refused as there.  A refused call writes nothing.  The host-pointer forms (compress, _many, the feed) stay native-only. */
int rspt_hip_compress_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, void* d_dst, size_t dst_stride,
                                       uint64_t* d_sizes, void* stream);
int rspt_hip_decompress_planar_batch_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, size_t nblocks, int32_t* d_planar,
                                         uint64_t* d_consumed, void* stream);
int rspt_hip_decompress_packed_planar_dev(rspt_hip_packer* p, const void* d_packed, size_t packed_len, size_t nblocks, int32_t* d_planar,
                                          uint64_t* d_consumed, void* stream);

/* ---- the quality ladder, the PRDN target, the byte budget and the byte total on the planar matrix ----
 * The planar forms of rspt_hip_compress_batch_ladder_dev, rspt_hip_decompress_batch_ladder_dev,
 * rspt_hip_compress_target_batch_dev, rspt_hip_compress_budget_batch_dev and rspt_hip_compress_total_batch_dev, under five
 * identities:
 *
 *   compress_planar_ladder(P, ladder, choice)  ==  rspt_hip_compress_batch_ladder_dev(rspt_hip_i32_to_native_batch_dev(P), ladder, choice)
 *       the streams, d_sizes, and "exactly bit 63, nothing written" for d_choice[b] >= nladder.
 *   decompress_planar_ladder(S, ladder, choice)  ==  rspt_hip_native_to_i32_batch_dev(rspt_hip_decompress_batch_ladder_dev(S, ladder, choice))
 *       for a block whose choice lies outside the ladder no element of its rows in d_planar is written and bit 63 is added to
 *       d_consumed[b]; the other blocks are not affected.
 *   target_planar(P, ...)  ==  rspt_hip_compress_target_batch_dev(rspt_hip_i32_to_native_batch_dev(P), ...)
 *       d_choice and d_prdn bit for bit, the streams byte for byte, d_sizes.  On a handle of bps < 4 the original of the rule is
 *       therefore the matrix CUT TO THE SAMPLE WIDTH -- what the stream can carry, the convention of
 *       rspt_hip_compress_planar_batch_dev: whatever lies above the low bps bytes of a value changes nothing.
 *       (rspt_hip_prdn_planar_batch_dev's "the whole int32 is the sample" does not apply here.)
 *   budget_planar(P, ...)  ==  rspt_hip_compress_budget_batch_dev(rspt_hip_i32_to_native_batch_dev(P), ...)
 *       d_choice, d_sizes (bit 63 included), the whole d_cand_sizes table and the streams byte for byte, and through
 *       rspt_hip_decompress_planar_batch_ladder_dev the decoded matrix.  On a handle of bps < 4 only the low bps bytes of each
 *       value count, as above; rspt_hip_set_byte_order has no effect.
 *   total_planar(P, ...)  ==  rspt_hip_compress_total_batch_dev(rspt_hip_i32_to_native_batch_dev(P), ...)
 *       d_choice, d_level, d_total and d_prdn bit for bit, both tables (d_cand_sizes, d_cand_figs), d_sizes (bit 63 included) and
 *       the streams byte for byte, on either route.  On a handle of bps < 4 only the low bps bytes of each value count, for the
 *       sizes and for the original the figures are taken against, as above; rspt_hip_set_byte_order has no effect.
 *
 * The refusals are the union of the planar entries' and the ladder entries': d_planar and d_choice 4-byte aligned (any 4-byte
 * alignment of the matrix works), RSPT_HIP_ERR_UNSUPPORTED for every kind but hadamard and the dense dct, the dst_stride bound,
 * the ladder's validation, an open feed; the target entry adds the native one's (target_prdn, nblocks <= 65535, d_prdn 8-byte
 * and d_work 16-byte aligned), the budget entry the native one's (nblocks <= 65535, d_budget and d_cand_sizes 8-byte and d_work
 * 16-byte aligned), the total entry the native one's (nblocks <= 65535, d_level, d_total, d_prdn, d_cand_sizes and d_cand_figs
 * 8-byte and d_work 16-byte aligned).  A refused call launches nothing and writes nothing.  d_planar is only read by the compress entries.  Asynchronous on
 * `stream`, no host synchronisation inside beyond rspt_hip_reserve's; the handle's own quantiser is neither read nor changed.
 *
 * The target entry takes the native one's two routes under the same condition, and rspt_hip_debug_set_target_route governs
 * it too; both give the same bits.  fused: the probe reads each row from the caller's matrix, cutting it as it loads -- no
 * converter pass, no copy of the original, no decoded copy.  general: per ladder entry the matrix goes through the planar
 * front end into the workspace; a cut copy of the original for the PRDN step is made only at bps < 4.  The tables of figures
 * lie in the handle's workspace (rspt_hip_reserve), so d_work holds block-sized scratch alone:
 * rspt_hip_compress_target_planar_work_bytes names it for the route a call would take NOW (after a change through
 * rspt_hip_debug_set_target_route, ask again) -- general: one decoded copy, the segment marks, and the cut original at bps < 4,
 * which at bps 4 is rspt_hip_compress_target_work_bytes less one planar copy or more; fused: 16 bytes, so that d_work is a
 * pointer.  Nothing is written behind the bytes it names.
 *
 * The budget entry takes the native one's two routes under the same conditions, and rspt_hip_debug_set_budget_route governs it
 * too; both give the same bits.  batched: the probe reads each row from the caller's matrix, cutting it as it loads -- no
 * converter pass, and no copy of the original in the workspace.  general: per ladder entry, and once more for the chosen streams,
 * the matrix goes through the planar front end.  d_work is the native entry's on either route -- the table of sizes and nothing
 * else: rspt_hip_compress_budget_planar_work_bytes names the bytes rspt_hip_compress_budget_work_bytes names, with its refusals
 * (RSPT_HIP_ERR_UNSUPPORTED for more than 65535 entry-blocks while the batched route is forced).  Native and planar budget calls
 * may alternate on one handle.
 *
 * The total entry takes the native one's two routes under the same conditions, and rspt_hip_debug_set_total_route governs it too
 * (one setting for both forms); both give the same bits.  fused: the probe reads each row from the caller's matrix once, cutting
 * it as it loads -- no converter pass, no copy of the original in the workspace, every slot only written; d_work is the native
 * fused one's, tables alone: rspt_hip_compress_total_planar_work_bytes names exactly rspt_hip_compress_total_work_bytes' bytes.
 * general: per ladder entry the matrix goes through the planar front end in the target entry's sequence and in the budget
 * entry's, and once more for the chosen streams; the original of the figures is the matrix itself at bps 4 -- d_work is the
 * native general one less one nblocks * nch * ns * 4 block rounded up to 256 bytes -- and a cut copy of it inside d_work at
 * bps < 4, where d_work is the native general one's size.  The sizing call answers for the route a call would take NOW and
 * refuses as the native one does (RSPT_HIP_ERR_UNSUPPORTED for more than 65535 entry-blocks while the fused route is forced).
 * Nothing is written behind the bytes it names.  Native and planar total calls may alternate on one handle, and behind either
 * the handle is in the same state. */
int rspt_hip_compress_planar_batch_ladder_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                                              const uint32_t* d_choice, void* d_dst, size_t dst_stride, uint64_t* d_sizes, void* stream);
int rspt_hip_decompress_planar_batch_ladder_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, size_t nblocks, const double* ladder,
                                                size_t nladder, const uint32_t* d_choice, int32_t* d_planar, uint64_t* d_consumed, void* stream);
int rspt_hip_compress_target_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);
int rspt_hip_compress_target_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                                              double target_prdn, void* d_dst, size_t dst_stride, uint64_t* d_sizes, uint32_t* d_choice,
                                              double* d_prdn, void* d_work, void* stream);
int rspt_hip_compress_budget_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);
int rspt_hip_compress_budget_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder, size_t nladder,
                                              size_t budget_bytes, const uint64_t* d_budget, void* d_dst, size_t dst_stride, uint64_t* d_sizes,
                                              uint32_t* d_choice, uint64_t* d_cand_sizes, void* d_work, void* stream);
int rspt_hip_compress_total_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);
int rspt_hip_compress_total_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, const double* ladder,
                                             size_t nladder, size_t total_bytes, void* d_dst, size_t dst_stride, uint64_t* d_sizes,
                                             uint32_t* d_choice, double* d_level, uint64_t* d_total, double* d_prdn,
                                             uint64_t* d_cand_sizes, double* d_cand_figs, void* d_work, void* stream);

/* hzr_verify (hzr_decode.c:569-624) of nblocks libhzr streams resident in device memory, WITHOUT decoding them: the frame walk,
 * the mode byte of every block (<= 2) and the CRC-32C of every block's payload against its header.  Stream b starts at
 * d_src + b*src_stride and has d_src_len[b] bytes (a device array); nothing at or beyond d_src + b*src_stride + d_src_len[b] is read.
 * d_decoded[b] = the decoded size its master header names; bit 63 set exactly where hzr_verify returns HZR_FAIL.  Like
 * hzr_verify it accepts ANY decoded size, not only the handle's, and ignores bytes behind the last block.  No output bytes are
 * produced and the handle's workspace is not touched.  RSPT_HIP_KIND_BYTES handles only (RSPT_HIP_ERR_ARG otherwise).
 * Asynchronous on `stream`. */
int rspt_hip_hzr_verify_batch_dev(rspt_hip_packer* p, const void* d_src, size_t src_stride, const uint64_t* d_src_len, size_t nblocks,
                                  uint64_t* d_decoded, void* stream);

/* ---- container: many streams, back to back (what a multi-GPU gather ships) ---
 * layout (little-endian):
 *   u64 magic 'RSPTPACK' | u64 nblocks | u64 payload_bytes | u64 nb of the LAST stream (low 32 bits), flagged streams (high 32)
 *   nblocks x { u64 offset, u64 length | nb << 56 | invalid << 63 }   offsets relative to the payload, 16-byte aligned
 *   payload                                    stream b at payload + offset[b], zero padded to 16 bytes
 * rspt_hip_pack_bound() bytes always suffice for d_packed.  d_total (device u64)
 * receives the container length.  The reference keeps nb out of the stream
 * (signal_packer_xdelta_hzr.cpp:39,66) and nb escalates inside a batch (and on every rank
 * independently), so each index entry carries the plane count of ITS stream: a container decodes
 * in one call whatever mix of nb it holds.  A stream that did not fit dst_stride at compress time
 * (bit 63 of its d_sizes entry) becomes an empty entry with the invalid bit set and is counted in
 * the header; nothing is copied for it.  d_sizes / nblocks must describe the handle's LAST
 * compress_batch call (that call's per-block nb is what the index records). */
size_t rspt_hip_pack_bound(const rspt_hip_packer* p, size_t nblocks);
int rspt_hip_pack_batch_dev(rspt_hip_packer* p, const void* d_dst, size_t dst_stride, const uint64_t* d_sizes, size_t nblocks, void* d_packed,
                            uint64_t* d_total, void* stream);

/* Decompress the nblocks streams of a container resident in device memory (16-byte aligned, packed_len bytes), as
 * laid out above: the consumer side of the gather.  Every stream is decoded with the nb of its own index entry; the
 * handle's nb state is neither used nor changed.  Header and index are checked against packed_len on the device: a
 * truncated or corrupt container flags its streams (bit 63 of d_consumed[b]) instead of reading out of bounds. */
int rspt_hip_decompress_packed_dev(rspt_hip_packer* p, const void* d_packed, size_t packed_len, size_t nblocks, void* d_dst, uint64_t* d_consumed,
                                   void* stream);

/* ---- the choice of a ladder or target compress in the container: no side channel beside the gathered containers ----
 * The index length word is  length | nb << 56 | choice << 60 | invalid << 63.  Bits 60..62 are zero in what
 * rspt_hip_pack_batch_dev writes, and rspt_hip_decompress_packed_dev / rspt_hip_decompress_packed_planar_dev ignore them: they
 * decode a choice-carrying container as they decode the plain one.  A ladder has at most 8 entries, so three bits are a choice.
 *
 * rspt_hip_pack_batch_choice_dev is rspt_hip_pack_batch_dev with d_choice[b] (device, nblocks uint32, 4-byte aligned: what the
 * ladder or target compress call had or wrote) in bits 60..62 of stream b's word.  Header, offsets, padding and nb bits are
 * unchanged: with every choice 0 the container is byte for byte rspt_hip_pack_batch_dev's.  A block flagged in d_sizes (bit 63)
 * becomes the empty flagged entry it is there, with choice bits 0.  A choice >= nladder (1..8) on a block that is NOT flagged
 * in d_sizes is the caller's error: its entry is written flagged (bit 63, length 0, counted in the header, nothing copied)
 * rather than with a choice that aliases another.  RSPT_HIP_ERR_UNSUPPORTED for every kind but hadamard and the dense dct.
 *
 * The two decoders take each stream's choice from its index entry, on the device:
 *   rspt_hip_decompress_packed_ladder_dev         ==  rspt_hip_decompress_batch_ladder_dev on the same streams and choices
 *   rspt_hip_decompress_packed_planar_ladder_dev  ==  rspt_hip_decompress_planar_batch_ladder_dev on them
 * A stored choice >= nladder flags the block (bit 63 of d_consumed[b]) and writes nothing for it, and so does a flagged entry.
 * The ladder itself stays a decoder argument, as the quality is: the header has no room for it and its format is not touched.
 * The container checks are rspt_hip_decompress_packed_dev's: packed_len < 32 + 16 * nblocks is RSPT_HIP_ERR_CORRUPT before the
 * device reads the index, and nothing at or behind d_packed + packed_len is read.  The choices pass through an array of the
 * handle's workspace (rspt_hip_reserve). */
int rspt_hip_pack_batch_choice_dev(rspt_hip_packer* p, const void* d_dst, size_t dst_stride, const uint64_t* d_sizes, size_t nblocks,
                                   const uint32_t* d_choice, size_t nladder, void* d_packed, uint64_t* d_total, void* stream);
int rspt_hip_decompress_packed_ladder_dev(rspt_hip_packer* p, const void* d_packed, size_t packed_len, size_t nblocks, const double* ladder,
                                          size_t nladder, void* d_dst, uint64_t* d_consumed, void* stream);
int rspt_hip_decompress_packed_planar_ladder_dev(rspt_hip_packer* p, const void* d_packed, size_t packed_len, size_t nblocks, const double* ladder,
                                                 size_t nladder, int32_t* d_planar, uint64_t* d_consumed, void* stream);

/* ---- multi-GPU: gather the containers of all ranks to one rank over RCCL -----------------------------
 * One process (or thread) per GPU, each with its own handle and its own ncclComm_t of one communicator.  The ranks hold
 * contiguous shards of independent blocks (no data-path collective); what travels is the result: the sizes by
 * ncclAllGather, the payload as ONE group of ncclSend / ncclRecv straight from every peer to the root (a gatherv over the
 * direct xGMI links; no ring).  `comm` is the caller's ncclComm_t, passed as void* so that this header needs no RCCL
 * header; the library binds to RCCL at the first call (see below which copy) and fails with RSPT_HIP_ERR_UNSUPPORTED when
 * there is none.
 *
 *   rspt_hip_gather_sizes     d_total (device u64: this rank's container length, as rspt_hip_pack_batch_dev wrote it) ->
 *                             d_totals[world] on every rank, and -- if h_totals is not NULL -- a copy in the caller's
 *                             page-locked host array h_totals[world] (asynchronous: valid once `stream` has got there)
 *   rspt_hip_gather_payload   with the sizes known on the host: root receives rank r's container at
 *                             d_recv + r * recv_stride (its own is copied there too), the others send theirs.
 *                             recv_stride >= the largest container (rspt_hip_pack_bound() always suffices), a multiple of
 *                             16 (rspt_hip_decompress_packed_dev wants 16-byte aligned containers; else RSPT_HIP_ERR_ARG),
 *                             the SAME value on every rank: a container that does not fit makes every rank return
 *                             RSPT_HIP_ERR_DST_TOO_SMALL before anything is posted
 *   rspt_hip_gather_containers  both, with one stream synchronisation in between (the sizes must reach the host before
 *                             the transfers can be posted); h_totals[world] receives the sizes on every rank.
 *                             A caller that gathers every step posts the payload of step i after the sizes of step
 *                             i+1 instead (no synchronisation: see rspt_amd/shard.py LaggedGather for the pattern).
 *   rspt_hip_gather_post_sizes / _post_payload / _wait   the same gather for a caller that gathers EVERY step, without a host
 *                             synchronisation in the step (two slots, 0 and 1, alternate):
 *                               step i:  ... compress + rspt_hip_pack_batch_dev on `stream` ...
 *                                        rspt_hip_gather_post_payload(slot of step i-1)   -- its sizes arrived a step ago
 *                                        rspt_hip_gather_post_sizes(slot of step i, stream)
 *                               at the end: rspt_hip_gather_post_payload(last slot).
 *                             Both run on a gather stream of the handle: post_sizes orders it behind `stream` (the pack),
 *                             the payload of step i-1 is posted in front of that and overlaps the kernels of step i.
 *                             post_payload reads the sizes on the host (waits for them only if they have not arrived),
 *                             copies them to h_totals[world] if that is not NULL, and posts the transfers;
 *                             rspt_hip_gather_wait(slot, stream) makes `stream` wait for the slot's payload (before the
 *                             container buffer of that slot is written again, before d_recv is read).
 * The library binds to the copy of RCCL the process has already mapped (where the caller's ncclComm_t came from); with none
 * mapped it loads librccl.so.1; with two different copies mapped (e.g. a framework's bundled one next to /opt/rocm's) every
 * gather call returns RSPT_HIP_ERR_UNSUPPORTED unless the environment variable RSPT_RCCL_LIB names the one to use.
 * All ranks must make the same calls in the same order.  Asynchronous on `stream` except where said. */
int rspt_hip_gather_sizes(rspt_hip_packer* p, void* comm, int world, const uint64_t* d_total, uint64_t* d_totals, uint64_t* h_totals, void* stream);
int rspt_hip_gather_payload(rspt_hip_packer* p, void* comm, int rank, int world, int root, const void* d_packed, const uint64_t* h_totals,
                            void* d_recv, size_t recv_stride, void* stream);
int rspt_hip_gather_containers(rspt_hip_packer* p, void* comm, int rank, int world, int root, const void* d_packed, const uint64_t* d_total,
                               void* d_recv, size_t recv_stride, uint64_t* h_totals, void* stream);
int rspt_hip_gather_post_sizes(rspt_hip_packer* p, void* comm, int world, const uint64_t* d_total, int slot, void* stream);
int rspt_hip_gather_post_payload(rspt_hip_packer* p, void* comm, int rank, int world, int root, const void* d_packed, int slot, void* d_recv,
                                 size_t recv_stride, uint64_t* h_totals);
int rspt_hip_gather_wait(rspt_hip_packer* p, int slot, void* stream);

/* ---- optional stage in front of compress: the reference's IIR pre-filter ---------------------------------------
 * Replaces the filter step of the reference's own pipeline (lib_rspt_test/rspt_test.cpp:116-136): i_filter::new_iir
 * (n, d, nr_coefficients), init_history_values(first sample of the channel, init_nr_samples), filter_opt on every sample
 * (lib_rspt/lib_filter/iir_filter.cpp:46-116), result truncated to int32 and stored back in the native sample width --
 * nblocks device-resident blocks (interleaved native layout, as for compress), IN PLACE, bit-identical with the reference.
 * Every product and sum is rounded on its own (no fused multiply-add); the truncation is x86-64's: every NaN, +-inf and
 * |y| >= 2^31 becomes INT32_MIN (an unstable filter or non-finite coefficients reach them), and the store keeps the low bps
 * bytes.  Samples are read and written little-endian, whatever rspt_hip_set_byte_order says.
 *   init_nr_samples 0 .. 2^28: filter() runs 4 * init_nr_samples times on the channel's first sample before the channel
 *   nblocks         1 or more; nblocks * nch must stay below 2^31 (else RSPT_HIP_ERR_ARG, as for a bad order or history)
 *   n, d            host arrays of nr_coefficients doubles (2..5): feedback (n[0] unused) and feed-forward coefficients
 *   per_channel     0: one filter object for all channels of a block, its state running on from channel to channel, as
 *                      in the reference's harness (the channels of a block are then a serial chain: one thread per block);
 *                   1: a fresh filter per channel (one i_filter per channel): one thread per channel
 * Handles of more than 8191 channels: this stage, its carried-state form, the FIR and median stages (both forms), both peak
 * stages and the PRDN stage are verified on handles of up to 8191 channels only and return RSPT_HIP_ERR_UNSUPPORTED beyond,
 * before anything is launched (the packers and the two converters take up to 65535).
 * Asynchronous on `stream`. */
int rspt_hip_iir_prefilter_batch_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, size_t nr_coefficients,
                                     int init_nr_samples, int per_channel, void* stream);

/* ---- the IIR pre-filter with a carried state: one i_filter per channel over a recording that arrives in blocks ------
 * The nblocks blocks of a call are consecutive pieces of ONE recording (block b holds its rows b * ns .. (b + 1) * ns - 1) and
 * the next call on the same state continues where this one ended.  Per channel there is one reference object,
 * i_filter::new_iir(n, d, nr_coefficients): on the channel's first sample ever it runs init_history_values(that sample,
 * init_nr_samples), then filter_opt((double)x) on every sample of every block of every call, the rings running on
 * (iir_filter.cpp:81-107); each result is truncated and stored in place as rspt_hip_iir_prefilter_batch_dev does, the rings
 * keep the untruncated doubles -- so a NaN that enters a ring stays there across blocks and calls, as in the reference.
 * Bit-identical with the reference's object driven the same way.  This is the per-channel driving only: one object shared by
 * the channels AND carried over blocks has no counterpart in a use of the reference.
 *   d_state         a caller-owned device buffer of rspt_hip_iir_state_bytes bytes, 8-byte aligned: per channel c, at byte
 *                   88 * c, double x[5] (x_ring_: the last inputs, newest first), double y[5] (y_ring_: the last outputs,
 *                   newest first, untruncated), uint64 started; places past nr_coefficients are not used.  All-zero bytes
 *                   are a fresh object for every channel.  A state belongs to the handle's (bps, nch) and to the
 *                   nr_coefficients that it was first used with; the coefficient VALUES may change from call to call, the
 *                   rings simply run on.  Two states may be used in turn on one handle (two recordings of one shape).
 *   init_nr_samples read only by a channel whose state is fresh (any value 0 .. 2^28 otherwise)
 * RSPT_HIP_ERR_ARG for everything rspt_hip_iir_prefilter_batch_dev refuses, a NULL or misaligned d_state and a NULL bytes;
 * RSPT_HIP_ERR_UNSUPPORTED for a call of 2^31 - 2^17 rows (nblocks * ns) or more: split the call, with a state that is exact.
 * A channel is one serial chain over the whole call and only nch lanes run, so a call takes about the stateless per-channel
 * time of ONE lane over nblocks * ns samples whatever nch <= 64 is (DESIGN.md 4b has the measured figures); calls of fewer
 * than 64 rows take the slower one-thread-per-channel form.  Asynchronous on `stream`; calls on one handle or one state are
 * stream-ordered.  The stage allocates nothing.
 * Handles of more than 8191 channels: RSPT_HIP_ERR_UNSUPPORTED before anything is launched (see rspt_hip_iir_prefilter_batch_dev). */
int rspt_hip_iir_state_bytes(rspt_hip_packer* p, size_t* bytes); /* nch * 88 */
int rspt_hip_iir_prefilter_stream_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, size_t nr_coefficients,
                                      int init_nr_samples, void* d_state, void* stream);

/* ---- a cascade of IIR filters: the reference's objects chained per sample, truncated once ---------------------------
 * The reference's filters return double and its users chain them per sample: lp->filter_opt(hp->filter_opt(x)) for a high-pass
 * in front of a low-pass, three filters in peak_detector.h:89-91.  Two calls of rspt_hip_iir_prefilter_batch_dev do NOT give
 * that answer (the intermediate result would be truncated and stored in the sample width); this stage does.
 * Each channel has S objects f_k = i_filter::new_iir(n_k, d_k, nc_k), k = 0 .. S-1, 1 <= S <= 4; nc_k is 2..5 and may differ per
 * section; n is the feedback side and d the feed-forward side, as in the IIR pre-filter stage.  On the channel's first sample x0
 * every section runs f_k->init_history_values((double)x0, init_nr_samples[k]): every section is initialised with x0, the RAW
 * first sample, not with the section's own input; init_nr_samples[k] = 0 (range 0 .. 2^28) runs nothing and leaves the rings
 * zero, the right start for a section behind a high-pass.  Then, for every sample,
 *     v = (double)x;  for k in 0..S-1:  v = use_filter[k] ? f_k->filter(v) : f_k->filter_opt(v);
 *     y = (int32_t)v, as x86-64 truncates (every NaN, +-inf and |v| >= 2^31 -> INT32_MIN); the low bps bytes are stored in place
 * Every product and sum is rounded on its own (no fused multiply-add); filter_opt sums in the order of rolling_iir_filter_N_
 * (every feed-forward term, then the feedback terms), filter in the order of iir_filter.cpp:72-77 (feed-forward and feedback
 * terms interleaved), so the two round differently.  Intermediate doubles are never truncated: a NaN or inf that leaves section
 * k enters the rings of section k + 1.  Samples are little-endian.  Bit-identical with the reference's objects chained so.
 *   nsections        S, 1..4
 *   n, d             5 * nsections host doubles, section k at 5k; places past nc_k are not read
 *   nr_coefficients  nsections values nc_k, each 2..5
 *   init_nr_samples  nsections values, each 0 .. 2^28
 *   use_filter       nsections bytes, or NULL: filter_opt for every section
 * Stateless form (rspt_hip_iir_cascade_batch_dev): a fresh chain per (block, channel) -- the per-channel driving of the IIR
 * pre-filter stage; there is no shared-object mode.
 * Stream form (rspt_hip_iir_cascade_stream_dev): the blocks of a call are consecutive rows of one recording, one chain per
 * channel lives in d_state and runs on into the next call.  d_state: rspt_hip_iir_cascade_state_bytes bytes, 8-byte aligned, the
 * IIR pre-filter's record (88 bytes: double x[5], double y[5], uint64 started) for channel c, section k at byte
 * 88 * (c * S + k).  All-zero bytes are a fresh chain; `started` of section 0 decides whether a channel initialises, and a call
 * writes all S of them.  With S = 1 the layout is rspt_hip_iir_prefilter_stream_dev's own, and a state may move between the two
 * entries.  init_nr_samples is read only by a channel whose state is fresh.
 * RSPT_HIP_ERR_ARG for nsections outside 1..4, an nc_k outside 2..5, a bad init, NULL arrays (use_filter excepted), a misaligned
 * or NULL state, nblocks = 0 or nblocks * nch >= 2^31; RSPT_HIP_ERR_UNSUPPORTED for more than 8191 channels, before anything is
 * launched, and for a stream call of 2^31 - 2^17 rows (nblocks * ns) or more.  Runs of 32 rows and more (a block; in the
 * stream form a call) take the pipelined kernel -- one recurrence wave per section, so the time per sample is the slowest
 * section's, not the sum --, shorter ones one thread per channel.  Asynchronous on `stream`, stream-ordered per
 * handle and per state; the stage allocates nothing. */
int rspt_hip_iir_cascade_batch_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, size_t nsections, const double* n, const double* d,
                                   const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* stream);
int rspt_hip_iir_cascade_state_bytes(rspt_hip_packer* p, size_t nsections, size_t* bytes); /* nch * nsections * 88 */
int rspt_hip_iir_cascade_stream_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, size_t nsections, const double* n, const double* d,
                                    const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* d_state,
                                    void* stream);

/* ---- the IIR pre-filter and the IIR cascade on the planar int32 matrix: the reference's own filter step ---------------
 * The reference filters samples where they live as int32: convert_native_to_i32 into a [nch][ns] matrix,
 * enc.d2d[j][i] = filter->filter_opt(enc.d2d[j][i]) on that matrix, convert_i32_to_native, the packer
 * (lib_rspt_test/rspt_test.cpp:116-136).  These four entries are that middle step for a caller whose samples are in the
 * converters' matrix, so that native_to_i32 -> IIR -> compress_planar runs without leaving it.  Arguments, arithmetic, driving
 * modes, routes and state are those of the native siblings above (rspt_hip_iir_prefilter_batch_dev / _stream_dev,
 * rspt_hip_iir_cascade_batch_dev / _stream_dev) with int32_t* d_planar in place of void* d_buf:
 *   d_planar   the matrix of rspt_hip_native_to_i32_batch_dev, block b's channel c at d_planar + (b*nch + c)*ns, filtered IN
 *              PLACE; it needs 4-byte alignment only.
 *   samples    the WHOLE int32 value is the sample, as in the reference's matrix loop: the handle's bps and byte order have no
 *              effect.  The result is (int32_t)y as x86-64 truncates (every NaN, +-inf and |y| >= 2^31 -> INT32_MIN), stored
 *              whole and NOT cut to bps.  So  i32_to_native(iir_planar(native_to_i32(X))) == iir_native(X)  for every bps, and
 *              compress_planar(iir_planar(native_to_i32(X))) gives the streams of compress(iir_native(X)), because
 *              compress_planar cuts as rspt_hip_i32_to_native_batch_dev does.
 *   modes      per_channel = 0: one object per block, running on from channel to channel (the harness); 1: a fresh object per
 *              (block, channel).  The cascade is per channel only.
 *   stream     the blocks of a call are consecutive pieces of one recording: channel c's run is P[0][c][:], P[1][c][:], ...
 *              d_state has the native entries' layout and size (rspt_hip_iir_state_bytes, rspt_hip_iir_cascade_state_bytes);
 *              all-zero bytes are a fresh object.  Native and planar calls may alternate on one state, exactly where the native
 *              samples are int32 (a narrower native call cuts what it stores, the rings run on uncut either way); with one
 *              section a state may move between the single and the cascade entries, as for the native ones.
 * Refused as the native sibling refuses it: RSPT_HIP_ERR_ARG for NULL pointers, nblocks = 0, nblocks * nch >= 2^31, an order
 * outside 2..5, init_nr_samples outside 0 .. 2^28, nsections outside 1..4, a NULL or misaligned d_state -- and for a d_planar
 * off its 4-byte alignment; RSPT_HIP_ERR_UNSUPPORTED for more than 8191 channels, before anything is launched, and for a stream
 * call of 2^31 - 2^17 rows or more.  A refused call writes nothing.  Asynchronous on `stream`; the entries allocate nothing.
 * Of the other stages the FIR pre-filter, the median and PRDN have planar forms too (rspt_hip_fir_prefilter_planar_batch_dev,
 * rspt_hip_median_filter_planar_batch_dev, rspt_hip_prdn_planar_batch_dev below), and so has the zero-phase IIR
 * (rspt_hip_iir_zero_phase_planar_batch_dev) and both R-peak detectors (rspt_hip_peak_detect_planar_batch_dev,
 * rspt_hip_peak_detect_offline_planar_batch_dev): every stage has a planar form. */
int rspt_hip_iir_prefilter_planar_batch_dev(rspt_hip_packer* p, int32_t* d_planar, size_t nblocks, const double* n, const double* d,
                                            size_t nr_coefficients, int init_nr_samples, int per_channel, void* stream);
int rspt_hip_iir_prefilter_planar_stream_dev(rspt_hip_packer* p, int32_t* d_planar, size_t nblocks, const double* n, const double* d,
                                             size_t nr_coefficients, int init_nr_samples, void* d_state, void* stream);
int rspt_hip_iir_cascade_planar_batch_dev(rspt_hip_packer* p, int32_t* d_planar, size_t nblocks, size_t nsections, const double* n, const double* d,
                                          const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* stream);
int rspt_hip_iir_cascade_planar_stream_dev(rspt_hip_packer* p, int32_t* d_planar, size_t nblocks, size_t nsections, const double* n, const double* d,
                                           const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* d_state,
                                           void* stream);

/* ---- a zero-phase (forward-backward) IIR filter: one reference object run forward, then backward over its own output ----
 * The reference's offline user runs a filter forward and then backward over the same object (peak_detector_offline::detect,
 * peak_detector.h:309-328), which takes the delay and the phase distortion of a forward pass out again ("filtfilt").  Two calls of
 * rspt_hip_iir_prefilter_batch_dev on a reversed buffer do NOT give that answer: the intermediate result would be truncated to
 * the sample width and the second call would start a fresh object on the wrong sample.  This stage does, for one fresh object
 * per (block, channel) -- there is no carried state: zero-phase filtering is offline by nature --
 *     f = i_filter::new_iir(n, d, nr_coefficients)                         nr_coefficients 2..5
 *     f->init_history_values((double)x[0], init_nr_samples)                0 .. 2^28
 *     for t = 0 .. ns-1:      w[t] = f->filter_opt((double)x[t])
 *     f->init_history_values(w[ns-1], backward_init_nr_samples)            0 .. 2^28
 *     for t = ns-1 .. 0:      w[t] = f->filter_opt(w[t])
 *     y[t] = (int32_t)w[t]
 * The backward pass uses the same object as the forward pass, so the rings run on through the turn, as in detect()'s loops: the
 * y ring holds the forward pass's last outputs and the x ring its last INPUTS (the raw samples x[ns-1], x[ns-2], ...).
 * backward_init_nr_samples = 0 runs nothing before the backward pass (detect()'s way); a positive value runs filter()
 * 4 * backward_init_nr_samples times on the last forward output -- init_history_values does not reset the rings
 * (iir_filter.cpp:109-113), so the x ring then holds w[ns-1] in its first min(4 * backward_init_nr_samples, nr_coefficients)
 * places and the forward pass's older inputs behind them.  w stays double between the passes and is truncated once: a NaN or
 * +-inf that enters a ring stays there, through the turn as well.  The truncation is x86-64's, as in every other stage: every
 * NaN, +-inf and |w| >= 2^31 becomes INT32_MIN, and the low bps bytes are stored IN PLACE, little-endian.  Every product and sum
 * is rounded on its own (no fused multiply-add), in filter_opt's order.  Bit-identical with the reference driven this way.
 *   n, d       host arrays of nr_coefficients doubles: feedback (n[0] unused) and feed-forward coefficients
 *   d_work     a caller-owned device buffer, 8-byte aligned, of at least rspt_hip_iir_zero_phase_work_bytes(p, nblocks) bytes:
 *              one slab double [ns][64] per wave of 64 (block, channel) lanes, ceil(nblocks * nch / 64) * 64 * ns * 8 bytes; it
 *              holds w between the passes, needs no initialisation and nothing of it outlives the call
 *   work_bytes the size of d_work
 * RSPT_HIP_ERR_ARG for everything rspt_hip_iir_prefilter_batch_dev refuses, a backward_init_nr_samples outside 0 .. 2^28, a NULL
 * or misaligned d_work, a work_bytes below the bound and a NULL bytes; RSPT_HIP_ERR_UNSUPPORTED for more than 8191 channels (and
 * for a workspace whose byte count does not fit size_t), before anything is launched.  Blocks of 64 rows and more with
 * init_nr_samples >= nr_coefficients - 1 take the pipelined kernel -- one wave holds the recurrence through both passes, four
 * form the feed-forward sums, one writes --, the others one thread per (block, channel).  Asynchronous on
 * `stream`; the stage allocates nothing. */
int rspt_hip_iir_zero_phase_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t* bytes);
int rspt_hip_iir_zero_phase_batch_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, size_t nr_coefficients,
                                      int init_nr_samples, int backward_init_nr_samples, void* d_work, size_t work_bytes, void* stream);

/* ---- the zero-phase IIR filter on the planar int32 matrix --------------------------------------------------------------
 * rspt_hip_iir_zero_phase_batch_dev with the matrix of the converters in place of the native blocks (see the planar IIR entries
 * above), so that native_to_i32 -> zero-phase IIR -> compress_planar runs without leaving it.  The operation, n, d, both history
 * lengths, the arithmetic, the single truncation and the routes are the native entry's, one fresh object per row of the matrix.
 *   d_planar   the matrix [nblocks][nch][ns], block b's channel c at d_planar + (b*nch + c)*ns; 4-byte alignment is all it needs
 *   d_out      NULL or d_planar itself: the matrix is filtered IN PLACE.  Any other pointer: the result goes there (the same
 *              shape, 4-byte aligned) and d_planar is only read; the two nblocks*nch*ns*4-byte ranges must then not overlap at
 *              all.  Out of place costs nothing: the forward pass only reads the source, the backward pass only writes the
 *              destination.
 *   samples    the WHOLE int32 value is the sample: the handle's bps and byte order have no effect, and the result
 *              (int32_t)w[t] (every NaN, +-inf and |w| >= 2^31 -> INT32_MIN) is stored whole and NOT cut to bps.  So
 *              i32_to_native(zp_planar(native_to_i32(X))) == zp_native(X) for every bps, and
 *              compress_planar(zp_planar(native_to_i32(X))) gives the streams of compress(zp_native(X)).
 *   d_work     the native entry's workspace, sized by rspt_hip_iir_zero_phase_work_bytes(p, nblocks): one slab double [ns][64]
 *              per 64 rows of the matrix (row b*nch + c is the unit); needs no initialisation
 * RSPT_HIP_ERR_ARG for everything rspt_hip_iir_zero_phase_batch_dev refuses, a d_planar or d_out off its 4-byte alignment and
 * matrices that overlap without being the same; RSPT_HIP_ERR_UNSUPPORTED for more than 8191 channels (and a workspace whose
 * byte count does not fit size_t).  Refusals come before anything is launched, and a refused call writes nothing.  Rows of 64
 * samples and more with init_nr_samples >= nr_coefficients - 1 take the pipelined kernel, the others one thread per row.
 * Asynchronous on `stream`; the stage allocates nothing. */
int rspt_hip_iir_zero_phase_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, int32_t* d_out, size_t nblocks, const double* n, const double* d,
                                             size_t nr_coefficients, int init_nr_samples, int backward_init_nr_samples, void* d_work, size_t work_bytes,
                                             void* stream);

/* ---- optional stage in front of compress: the reference's FIR pre-filter ---------------------------------------
 * i_filter::new_fir(kernel, kernel_size), init_history_values(first sample of the channel, n), filter_opt on every sample
 * (lib_rspt/lib_filter/fir_filter.cpp), result truncated to int32 and stored in the native sample width, on nblocks
 * device-resident blocks (interleaved native layout, as for compress), bit-identical with the reference.  With K = kernel_size:
 *     y[c][t] = ((((0.0 + x[c][t-K+1]*k[0]) + x[c][t-K+2]*k[1]) + ...) + x[c][t]*k[K-1]),    x[c][s < 0] = x[c][0]
 * every product and sum rounded on its own (no fused multiply-add), in ascending tap order; the truncation is x86-64's: every
 * NaN, +-inf and |y| >= 2^31 becomes INT32_MIN, and the store keeps the low bps bytes.  Samples are little-endian.
 * One filter object shared by all channels of a block gives the same result as one filter per channel (the history
 * initialisation replaces the whole window), so there is no mode to choose.
 *   d_src, d_dst    nblocks blocks each; d_dst == d_src filters in place, any other overlap is RSPT_HIP_ERR_ARG
 *   kernel          host array of kernel_size doubles, 1 <= kernel_size <= 65536; read before the call returns
 * The handle only supplies the shape (bps, nch, ns); any packer kind will do.  nblocks * nch must stay below 2^31, as for the IIR
 * stage.  Asynchronous on `stream`, with the ordering contract of rspt_hip_compress_batch_dev: successive calls on one handle
 * are stream-ordered.  Device and page-locked memory the stage needs belong to the handle.
 * Handles of more than 8191 channels: RSPT_HIP_ERR_UNSUPPORTED before anything is launched (see rspt_hip_iir_prefilter_batch_dev). */
int rspt_hip_fir_prefilter_batch_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, const double* kernel, size_t kernel_size,
                                     void* stream);

/* ---- the FIR pre-filter with a carried state: one i_filter per channel over a recording that arrives in blocks ------
 * The nblocks blocks of a call are consecutive pieces of ONE recording and the next call on the same state continues where this
 * one ended.  Per channel there is one reference object, i_filter::new_fir(kernel, K): init_history_values(the channel's first
 * sample ever) once, then filter_opt on every sample of every block of every call (fir_filter.cpp:52-60).  With X = the
 * channel's whole recording so far,
 *     y[t] = ((((0.0 + X[t-K+1]*k[0]) + X[t-K+2]*k[1]) + ...) + X[t]*k[K-1]),    X[s < 0] = X[0]
 * rounded, truncated and stored as rspt_hip_fir_prefilter_batch_dev does; in place and out of place as there (out of place
 * d_src is only read).  Bit-identical with the reference's object driven the same way.
 *   d_state         a caller-owned device buffer of rspt_hip_fir_state_bytes(p, kernel_size) bytes, 8-byte aligned: uint64
 *                   started, then the last K - 1 input rows of the recording, oldest first, each row nch samples of bps bytes
 *                   as in a block (the object's ring without its newest place), padded to a multiple of 8 bytes.  All-zero
 *                   bytes are a fresh object for every channel.  K - 1 may exceed ns and may exceed a whole call: the new
 *                   state is the tail of (old state ++ the call's rows).  A state belongs to the handle's (bps, nch) and to
 *                   the kernel_size that sized it; the kernel's VALUES may change from call to call.  Two states may be used
 *                   in turn on one handle.
 * RSPT_HIP_ERR_ARG for everything rspt_hip_fir_prefilter_batch_dev refuses, a NULL or misaligned d_state and a NULL bytes;
 * RSPT_HIP_ERR_UNSUPPORTED for a call of 2^31 - 2^17 rows (nblocks * ns) or more: split the call, with a state that is exact.
 * Every output depends on inputs only, so the stage is as parallel as the stateless one and does the same multiply-add work,
 * plus two copies of K - 1 rows.  Asynchronous on `stream`; calls on one handle or one state are
 * stream-ordered.  The stage allocates nothing per state: the staged copy of the old state belongs to the handle.
 * Handles of more than 8191 channels: RSPT_HIP_ERR_UNSUPPORTED before anything is launched (see rspt_hip_iir_prefilter_batch_dev). */
int rspt_hip_fir_state_bytes(rspt_hip_packer* p, size_t kernel_size, size_t* bytes); /* 8 + ((K - 1) * nch * bps rounded up to 8) */
int rspt_hip_fir_prefilter_stream_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, const double* kernel, size_t kernel_size,
                                      void* d_state, void* stream);

/* ---- the FIR pre-filter on the planar int32 matrix: i_filter::new_fir where the reference runs it ----------------------
 * The other factory of the reference's filter interface on the matrix of the converters (see the planar IIR entries above):
 * rspt_hip_fir_prefilter_batch_dev / _stream_dev with the matrix in place of the native blocks, so that
 * native_to_i32 -> FIR -> compress_planar runs without leaving it.  kernel, kernel_size, the arithmetic, the truncation and the
 * ordering contract are the native entries'.
 *   d_src, d_dst    the matrix [nblocks][nch][ns], block b's channel c at d + (b*nch + c)*ns; 4-byte alignment is all it needs
 *                   (16-byte aligned buffers with ns a multiple of 4 take wider loads and stores).  d_dst == d_src filters in
 *                   place; any other overlap of the two nblocks*nch*ns*4-byte ranges is RSPT_HIP_ERR_ARG; out of place d_src is
 *                   only read.
 *   samples         the WHOLE int32 value is the sample: the handle's bps and byte order have no effect, and the result
 *                   (int32_t)y (every NaN, +-inf and |y| >= 2^31 -> INT32_MIN) is stored whole and NOT cut to bps.  So
 *                   i32_to_native(fir_planar(native_to_i32(X))) == fir_native(X) for every bps, and
 *                   compress_planar(fir_planar(native_to_i32(X))) gives the streams of compress(fir_native(X)).
 *   stream          the blocks of a call are consecutive pieces of one recording: channel c's run is P[0][c][:], P[1][c][:], ...
 *                   and continues into the next call on the same state.  A window near the start of a block reaches into the
 *                   blocks before it and, behind the call's first block, into the state.
 *   d_state         caller-owned, 8-byte aligned, rspt_hip_fir_planar_state_bytes(p, kernel_size) bytes: uint64 started, then the
 *                   last K - 1 input rows of the recording, oldest first, each row nch int32 values, padded to a multiple of 8
 *                   bytes -- the native state's layout at bps = 4.  On a handle with bps = 4 the two sizes are equal and native
 *                   and planar stream calls may alternate on one state; on a narrower handle a planar state is its own object,
 *                   not interchangeable with the native one.  All-zero bytes are a fresh object (X[s < 0] = the channel's first
 *                   sample ever).  K - 1 may exceed ns and may exceed a whole call; the kernel's VALUES may change between
 *                   calls, its size may not; two states may be used in turn on one handle.
 * RSPT_HIP_ERR_ARG for a NULL handle, buffer or kernel, a NULL bytes, nblocks = 0, nblocks * nch >= 2^31, kernel_size outside
 * 1..65536, a matrix off its 4-byte alignment, buffers that overlap without being the same, a NULL or misaligned d_state;
 * RSPT_HIP_ERR_UNSUPPORTED for more than 8191 channels, a stream call of 2^31 - 2^17 rows (nblocks * ns) or more, and a
 * stateless call on rows of that many samples.  Refusals come before anything is launched, and a refused call writes nothing.
 * Asynchronous on `stream`.  What a call stages belongs to the handle and only grows: with span = the samples one workgroup
 * takes of a row and nsplit = ceil(ns / span), the K - 1 samples in front of every span but the first of an
 * in-place call and in front of every row of a stream call,
 *     4 * (K - 1) * nblocks * nch * ((in place ? nsplit - 1 : 0) + (stream ? 1 : 0))  bytes,
 * plus 4 * (K - 1) * nch bytes of a stream call's old state.  nsplit is 1 unless the batch has fewer row groups than four per
 * CU, and a span is at least 4 (K - 1) samples then.  A stateless out-of-place call stages nothing. */
int rspt_hip_fir_prefilter_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, const double* kernel,
                                            size_t kernel_size, void* stream);
int rspt_hip_fir_planar_state_bytes(rspt_hip_packer* p, size_t kernel_size, size_t* bytes); /* 8 + ((K - 1) * nch * 4 rounded up to 8) */
int rspt_hip_fir_prefilter_planar_stream_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, const double* kernel,
                                             size_t kernel_size, void* d_state, void* stream);

/* ---- optional stage in front of compress: the reference's rolling-window median -------------------------------
 * rolling_window_median<double>(window) (lib_rspt/lib_stat/rolling_window_median.h), one fresh object per channel of every
 * block, insert((double)x[c][t]) for t = 0 ... ns - 1, (int32_t) of each return value stored in the native sample width, on
 * nblocks device-resident blocks (interleaved native layout, as for compress), bit-identical with the reference.  With
 * W = window, lo = max(0, t - W + 1), m = t - lo + 1 and s = sorted(x[c][lo .. t]):
 *     y[c][t] = m odd ? s[m / 2] : (int32_t)(((int64_t)s[m / 2 - 1] + s[m / 2]) / 2)      (C division: toward zero)
 * so the first W - 1 outputs of a channel are medians of an expanding window, a window of ns or more is the expanding median
 * of the whole channel, and window = 1 copies the block.  Samples are little-endian, read sign-extended from bps bytes.
 *   d_src, d_dst    nblocks blocks each; d_dst == d_src filters in place, any other overlap is RSPT_HIP_ERR_ARG
 *   window          1 or more (0 is RSPT_HIP_ERR_ARG); windows above 32 need ns <= 2^18 (else RSPT_HIP_ERR_UNSUPPORTED)
 * The handle only supplies the shape (bps, nch, ns); any packer kind will do.  nblocks * nch must stay below 2^31.
 * Asynchronous on `stream`, with the ordering contract of rspt_hip_compress_batch_dev: successive calls on one handle are
 * stream-ordered.  Device memory the stage needs belongs to the handle.
 * Handles of more than 8191 channels: RSPT_HIP_ERR_UNSUPPORTED before anything is launched (see rspt_hip_iir_prefilter_batch_dev). */
int rspt_hip_median_filter_batch_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, size_t window, void* stream);

/* ---- the rolling-window median with a carried state: one object per channel over a recording that arrives in blocks ----
 * The nblocks blocks of a call are consecutive pieces of ONE recording and the next call on the same state continues where this
 * one ended.  Per channel there is one reference object, rolling_window_median<double>(window): insert((double)x) on every
 * sample of every block of every call, (int32_t) of each return value stored as rspt_hip_median_filter_batch_dev stores it.
 * With X = the channel's whole recording so far, T a sample's index in it and W = window,
 *     lo = max(0, T - W + 1),  m = T - lo + 1,  s = sorted(X[lo .. T])
 *     y[T] = m odd ? s[m / 2] : (int32_t)(((int64_t)s[m / 2 - 1] + s[m / 2]) / 2)      (C division: toward zero)
 * W is NOT clamped to ns: it may exceed ns and it may exceed a whole call, and the expanding phase happens once per recording.
 * Bit-identical with the reference's object driven block by block, however the recording is cut into blocks and calls.  In
 * place and out of place as rspt_hip_median_filter_batch_dev (out of place d_src is only read).
 *   d_state         a caller-owned device buffer of rspt_hip_median_state_bytes(p, window) bytes, 8-byte aligned: uint64 fill,
 *                   then W - 1 rows, oldest first, each row nch samples of bps bytes as in a block, padded to a multiple of 8
 *                   bytes.  fill = min(rows of the recording so far, W - 1) is the number of valid rows; they are the LAST fill
 *                   rows of the buffer, and every row in front of them stays zero.  All-zero bytes are a fresh object for every
 *                   channel.  The new state is the tail of (old state ++ the call's rows), so its bytes are a function of the
 *                   recording and W alone, not of how the recording was cut.  A state belongs to the handle's (bps, nch) and to
 *                   the window that sized it.  Two states may be used in turn on one handle.  window = 1 copies the blocks;
 *                   its state is the 8-byte header and stays zero.
 * RSPT_HIP_ERR_ARG for everything rspt_hip_median_filter_batch_dev refuses (window 0, bad buffers, nblocks * nch >= 2^31), a
 * NULL or misaligned d_state and a NULL bytes; RSPT_HIP_ERR_UNSUPPORTED for a call of 2^31 - 2^17 rows (nblocks * ns) or more
 * (split the call: with a state that is exact), and, from both entries, for a window above 32 with W - 1 > 2^17.  Windows up to
 * 32 have no other limit; windows above 32 take any ns and any call length below the row limit (the stateless entry's
 * ns <= 2^18 does not apply: a call is cut into segments of at most 2^18 rows that overlap by W - 1).
 * Asynchronous on `stream`; calls on one handle or one state are stream-ordered.  The stage allocates nothing per state: the
 * staged copy of the old state belongs to the handle.
 * Handles of more than 8191 channels: RSPT_HIP_ERR_UNSUPPORTED before anything is launched (see rspt_hip_iir_prefilter_batch_dev). */
int rspt_hip_median_state_bytes(rspt_hip_packer* p, size_t window, size_t* bytes); /* 8 + ((W - 1) * nch * bps rounded up to 8) */
int rspt_hip_median_filter_stream_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, size_t window, void* d_state,
                                      void* stream);

/* ---- the rolling-window median on the planar int32 matrix ------------------------------------------------------------
 * rspt_hip_median_filter_batch_dev / _stream_dev with the matrix of the converters in place of the native blocks (see the planar
 * IIR and FIR entries above), so that native_to_i32 -> median -> compress_planar runs without leaving it.  The formula, the
 * window rules and the ordering contract are the native entries'.
 *   d_src, d_dst    the matrix [nblocks][nch][ns], block b's channel c at d + (b*nch + c)*ns; 4-byte alignment is all it needs
 *                   (16-byte aligned buffers with ns a multiple of 4 take wider loads and stores).  d_dst == d_src filters in
 *                   place; any other overlap of the two nblocks*nch*ns*4-byte ranges is RSPT_HIP_ERR_ARG; out of place d_src is
 *                   only read.
 *   samples         the WHOLE int32 value is the sample: the handle's bps and byte order have no effect, and the median is
 *                   stored whole and NOT cut to bps.  So i32_to_native(median_planar(native_to_i32(X))) == median_native(X)
 *                   for every bps, and compress_planar(median_planar(native_to_i32(X))) gives the streams of
 *                   compress(median_native(X)).
 *   batch           one fresh rolling_window_median<double>(window) per row: the window is clamped to ns, window = 1 is a device
 *                   copy (nothing is done in place), windows above 32 need ns <= 2^18 (else RSPT_HIP_ERR_UNSUPPORTED).
 *   stream          the blocks of a call are consecutive pieces of one recording: channel c's run is P[0][c][:], P[1][c][:], ...
 *                   and continues into the next call on the same state.  W is not clamped: it may exceed ns and a whole call.
 *   d_state         caller-owned, 8-byte aligned, rspt_hip_median_planar_state_bytes(p, window) bytes: uint64 fill, then W - 1
 *                   rows, oldest first, each row nch int32 values, the valid rows last and zeros in front, padded to a multiple
 *                   of 8 bytes -- the native state's layout at bps = 4.  On a handle with bps = 4 the two sizes are equal and
 *                   native and planar stream calls may alternate on one state; on a narrower handle a planar state is its own
 *                   object, not interchangeable with the native one.  All-zero bytes are a fresh object.  The state's bytes
 *                   after a call are a function of the recording and W alone.  window = 1: the header, which stays zero.
 * RSPT_HIP_ERR_ARG for a NULL handle or buffer, a NULL bytes, window = 0, nblocks = 0, nblocks * nch >= 2^31, a matrix off its
 * 4-byte alignment, buffers that overlap without being the same, a NULL or misaligned d_state; RSPT_HIP_ERR_UNSUPPORTED for more
 * than 8191 channels, a stream call of 2^31 - 2^17 rows (nblocks * ns) or more and a stateless call on rows of that many
 * samples, a stateless window above 32 on rows of more than 2^18 samples, and a stream window above 32 with W - 1 > 2^17.
 * Refusals come before anything is launched, and a refused call writes nothing.  Asynchronous on `stream`, stream-ordered with
 * every other call on the handle.  What a call stages belongs to the handle's median stage and only grows: for windows up to
 * 32, with span = the samples one workgroup takes of a row and nsplit = ceil(ns / span), the W - 1 samples in
 * front of every span but the first of an in-place call and in front of every row of a stream call,
 *     4 * (W - 1) * nblocks * nch * ((in place ? nsplit - 1 : 0) + (stream ? 1 : 0))  bytes,
 * plus 8 + 4 * (W - 1) * nch bytes of a stream call's old state; above 32 the native entries' keys and ranks (20 bytes per key of
 * a piece of up to 2^25 keys).  A stateless out-of-place call of a window up to 32 stages nothing. */
int rspt_hip_median_filter_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, size_t window, void* stream);
int rspt_hip_median_planar_state_bytes(rspt_hip_packer* p, size_t window, size_t* bytes); /* 8 + ((W - 1) * nch * 4 rounded up to 8) */
int rspt_hip_median_filter_planar_stream_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, size_t window, void* d_state,
                                             void* stream);

/* ---- the reference's Butterworth designer (host only: no GPU, no handle) -------------------------------------------
 * create_filter_iir(num, den, butterworth, type, order, sampling_rate, cutoff_low, cutoff_high) of
 * lib_rspt/lib_filter/iir_filter_design.cpp, bit-identical with the reference's x86-64 build (same libm calls, same order of
 * operations, no contraction).  type: high_pass 0, low_pass 1, band_pass 2, band_stop 3 (the reference never reads `kind`).
 *   order 2, low/high pass    3 coefficients (cutoff_low)       order 2, band_pass        5 (4th order, cutoff_low .. high)
 *   order 1, low/high pass    2 coefficients (cutoff_low)       order 1, band_pass        3
 * As in the reference, order 1 band_stop gives the first-order band-pass, order 2 band_stop is refused, and so is every other
 * order, sampling_rate <= 0, cutoff_low <= 0 and (band-pass) cutoff_high <= cutoff_low: RSPT_HIP_ERR_ARG, with num, den and
 * *nr_coefficients untouched (so is a type outside 0..3).  num and den must hold 5 doubles each.  num is the feed-forward
 * side and den (den[0] = 1) the feedback side; i_filter::new_iir(n, d) takes them the other way round, so the IIR stage's
 * call is rspt_hip_iir_prefilter_batch_dev(..., n = den, d = num, nr_coefficients, ...). */
int rspt_hip_design_iir(int type, int order, double sampling_rate, double cutoff_low, double cutoff_high, double* num, double* den,
                        size_t* nr_coefficients);

/* ---- the reference's R-peak detectors ------------------------------------------------------------------------------
 * One detector per (block, channel) of nblocks device-resident blocks (the handle's shape, interleaved native layout; any
 * packer kind; samples little-endian, read sign-extended from bps bytes; d_src is only read), fed (double) of every sample:
 *   variant 0  ONLINE      peak_detector::detect             band-pass order 2 (10-20 Hz, 5 coefficients), integrator
 *                                                            low-pass order 2 (3 Hz), threshold low-pass order 2 (0.15 Hz), A = 25
 *   variant 1  ONLINE_1ST  peak_detector_1st_order::detect   band-pass order 1 (10-20 Hz, 3 coefficients), integrator order 1, A = 25
 *   variant 2  OFFLINE_FW  peak_detector_offline::detect_fw  band-pass order 1 (15-25 Hz), integrator order 1, A = 70
 * bit-identical with the reference's x86-64 build.  Per sample x: s = integrator(bp(x)^2), h = threshold(s), then the
 * reference's state machine with threshold_ratio 1.5, reference_ratio 0.5, peak_attenuation = 1 / (1 + A / fs) and
 * nr_slope_samples = (int)(100 fs / 1000).  Each filter is y0 = d0 x0 + d1 x1 + ... - n1 y1 - n2 y2 ..., left to right, with
 * the designer's numerator as d and its denominator as n (rspt_hip_design_iir), every product and sum rounded on its own.
 * Only the band-pass is initialised: 4 * (int)fs calls of filter(x) -- ONLINE / ONLINE_1ST at the sample where the sample
 * index is 0 (the first sample of a fresh detector), OFFLINE_FW with the first sample of every block, on whatever state the
 * filter holds.  With nr_slope_samples 0 (fs < 10) a detector fires on every sample whose counter is 0; with 1 (10 <= fs < 20)
 * it never fires.
 *   event         a sample at which detect() takes its marker branch, whatever the value: marker_val, or the integrator output
 *                 s where marker_val == -1.0 (so a marker of 0.0 or an s of 0.0 is still an event)
 *   d_count       [nblocks][nch] uint32: the exact number of events of each (block, channel); required
 *   d_index       [nblocks][nch][max_peaks] int32: the sample index within the block (the detect() call, not shifted back) of
 *   d_value       [nblocks][nch][max_peaks] double: ... and the value of the first max_peaks events; later events are counted
 *                 only.  max_peaks = 0 gives counts alone (d_index / d_value may then be NULL; else both are required)
 *   d_sig, d_threshold  optional [nblocks][ns][nch] doubles: s and h of every sample (peak_sample / threshold_sample;
 *                 filt_signal / threshold_signal for OFFLINE_FW); NULL for none (both or neither)
 *   d_state       NULL: a fresh detector per (block, channel).  Else a caller-owned device buffer of
 *                 rspt_hip_peak_state_bytes bytes holding one detector per channel: channel c runs through blocks
 *                 0 .. nblocks - 1 in order and on across calls (OFFLINE_FW: every block is one detect_fw call on the object).
 *                 All-zero bytes are a fresh detector.  A state belongs to the variant and sampling rate that made it.  Only
 *                 nch lanes run in this mode, so it is slower than fresh mode on few channels.  The sample index is the
 *                 reference's int: it wraps after 2^31 samples of a channel, and after 2^32 the band-pass history runs again.
 * RSPT_HIP_ERR_ARG for an unknown variant, a sampling_rate that is not finite, <= 0 or > 2^20, a NULL d_src or d_count,
 * max_peaks > 0 with a NULL d_index or d_value, only one of d_sig / d_threshold, nblocks == 0, nblocks * nch >= 2^31, or
 * max_peaks above 2^32.  Asynchronous on `stream`, with the ordering contract of rspt_hip_compress_batch_dev: successive calls
 * on one handle are stream-ordered.  The stage allocates nothing of its own.
 * Handles of more than 8191 channels: RSPT_HIP_ERR_UNSUPPORTED before anything is launched (see rspt_hip_iir_prefilter_batch_dev). */
int rspt_hip_peak_state_bytes(rspt_hip_packer* p, size_t* bytes); /* one detector per channel: nch * 208 bytes */
int rspt_hip_peak_detect_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, int variant, double sampling_rate, double marker_val,
                                   void* d_state, uint32_t* d_count, int32_t* d_index, double* d_value, size_t max_peaks, double* d_sig,
                                   double* d_threshold, void* stream);

/* ---- the reference's zero-phase offline R-peak detector ------------------------------------------------------------
 * peak_detector_offline::detect of lib_rspt/peak_detector.h, bit-identical with the reference's x86-64 build, one detector per
 * (block, channel) of nblocks device-resident blocks (the handle's shape, interleaved native layout; any packer kind; samples
 * little-endian, read sign-extended from bps bytes; d_src is only read).  Per block, with x = (double) of each sample: the
 * band-pass (order 1, 15-25 Hz) and the baseline (low-pass order 1, 0.5 Hz) each take 4 * (int)fs calls of filter(x[0]) on
 * whatever state they hold; the baseline runs forward and then backward over its own output; the band-pass runs forward
 * (outputs dropped) and then backward over x again; the integrator (low-pass order 1, 3 Hz) runs forward over the squares and
 * backward over its own output (filt_signal); the threshold (low-pass order 2, 0.15 Hz) runs forward over filt_signal (outputs
 * dropped) and backward over it again (threshold_signal).  No filter is reset between passes.  detect_fw's state machine
 * (A = 70, nr_slope_samples = (int)(100 fs / 1000)) then writes peak_signal: marker_val, or filt_signal where marker_val == -1.0,
 * at each firing, 0 elsewhere.  Each non-zero peak_signal[i], i >= nr_slope_samples, ascending, moves to i - nr_slope_samples + 1.
 * Then, with radius = (int)(10 fs / 1000), each non-zero peak_signal[i], radius <= i <= ns - radius - 1, ascending, moves to the
 * index of the largest (strict <, first wins) or the smallest (strict >) of x[j] - baseline[j] over i - radius <= j < i + radius
 * (the largest where max > -min; from -2e6 / 2e6 and index 0, so radius 0 (fs < 100) moves every peak to index 0).  A peak moved
 * ahead is visited again; a peak moved onto another replaces it.  A value is a peak where it is not zero (a NaN is one; 0.0 and
 * -0.0 are not).
 *   d_count       [nblocks][nch] uint32: the exact number of non-zero entries of the final peak_signal; required
 *   d_index       [nblocks][nch][max_peaks] int32 and
 *   d_value       [nblocks][nch][max_peaks] double: the first max_peaks of them in ascending index order (index within the block,
 *                 value); max_peaks = 0 gives counts alone (d_index / d_value may then be NULL; else both are required)
 *   d_sig, d_threshold  optional [nblocks][ns][nch] doubles: filt_signal and threshold_signal as detect() leaves them; NULL for
 *                 none (both or neither)
 *   d_state       NULL: a fresh object per (block, channel).  Else a caller-owned device buffer of rspt_hip_peak_state_bytes
 *                 bytes holding one object per channel: channel c runs through blocks 0 .. nblocks - 1 in order and on across
 *                 calls, carrying the four filters and the state machine.  The layout is OFFLINE_FW's of
 *                 rspt_hip_peak_detect_batch_dev, the baseline filter in band-pass slots OFFLINE_FW never uses, so one state may
 *                 take detect_fw (variant 2) and detect calls in turn, as one reference object can.  All-zero bytes are fresh.
 *   d_work        required: a caller-owned device buffer of at least rspt_hip_peak_offline_work_bytes(p, nblocks, d_state != NULL)
 *                 bytes, 8-byte aligned; the call overwrites it.  The stage allocates nothing of its own.
 * The reference's optional peak_indexes vector is not produced: it is sized by the count of shifted peaks before the
 * relocation, and overflows where a peak sits at nr_slope_samples - 1.  d_count / d_index hold the final peak_signal instead,
 * which is defined in every case.
 * RSPT_HIP_ERR_ARG for everything rspt_hip_peak_detect_batch_dev refuses (sampling_rate not finite, <= 0 or > 2^20, a NULL
 * d_src or d_count, max_peaks > 0 with a NULL d_index or d_value, only one of d_sig / d_threshold, nblocks == 0,
 * nblocks * nch >= 2^31, max_peaks above 2^32), a NULL or misaligned d_work, and the reference's undefined cases: fs < 10
 * (nr_slope_samples 0: its shift runs past the end of the array) and ns < radius (its unsigned loop bound wraps).
 * Asynchronous on `stream`, with the ordering contract of rspt_hip_compress_batch_dev.
 * Handles of more than 8191 channels: RSPT_HIP_ERR_UNSUPPORTED before anything is launched (see rspt_hip_iir_prefilter_batch_dev). */
int rspt_hip_peak_offline_work_bytes(rspt_hip_packer* p, size_t nblocks, int stateful, size_t* bytes);
int rspt_hip_peak_detect_offline_batch_dev(rspt_hip_packer* p, const void* d_src, size_t nblocks, double sampling_rate, double marker_val,
                                           void* d_state, void* d_work, uint32_t* d_count, int32_t* d_index, double* d_value,
                                           size_t max_peaks, double* d_sig, double* d_threshold, void* stream);

/* ---- both R-peak detectors on the planar int32 matrix --------------------------------------------------------------
 * rspt_hip_peak_detect_batch_dev and rspt_hip_peak_detect_offline_batch_dev on the converters' matrix: what the reference's user
 * runs behind the filters (band-pass or zero-phase filter, then detect), without leaving the matrix the planar filters wrote.
 * The reference's loop hands (double) of the int32 matrix element to detect(); so do these entries.  A planar filter stores its
 * result whole and rspt_hip_i32_to_native_batch_dev cuts to the handle's width, so on a handle of bps < 4 the peaks of a filtered
 * recording can be taken on the filter's own values only here.  Everything is the native sibling's, but:
 *   d_planar      int32 [nblocks][nch][ns], block b's channel c at d_planar + (b * nch + c) * ns; 4-byte alignment is all it needs;
 *                 only read.  The WHOLE int32 is the sample: the handle's bps and byte order have no effect.
 *   d_count, d_index, d_value   unchanged (they are [nblocks][nch](...) already).
 *   d_sig, d_threshold  optional [nblocks][nch][ns] doubles: planar as the samples are, row b * nch + c the traces of that row
 *                 of the matrix.
 *   d_state       the native layout and size (rspt_hip_peak_state_bytes); all-zero bytes are fresh detectors.  Channel c runs
 *                 through rows c, nch + c, 2 nch + c, ... and on into the next call.  Native calls on a bps = 4 handle and
 *                 planar calls may alternate on one state, and so may the online / OFFLINE_FW and the offline entries, as
 *                 natively.
 *   d_work        the native workspace and size (rspt_hip_peak_offline_work_bytes); needs no initialisation.
 * Refused as the native sibling refuses it, and RSPT_HIP_ERR_ARG for a d_planar off its 4-byte alignment; more than 8191
 * channels: RSPT_HIP_ERR_UNSUPPORTED.  All refusals come before any launch, and a refused call writes nothing.  Asynchronous on
 * `stream`; the entries allocate nothing. */
int rspt_hip_peak_detect_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, int variant, double sampling_rate,
                                          double marker_val, void* d_state, uint32_t* d_count, int32_t* d_index, double* d_value, size_t max_peaks,
                                          double* d_sig, double* d_threshold, void* stream);
int rspt_hip_peak_detect_offline_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, double sampling_rate,
                                                  double marker_val, void* d_state, void* d_work, uint32_t* d_count, int32_t* d_index,
                                                  double* d_value, size_t max_peaks, double* d_sig, double* d_threshold, void* stream);

/* ---- the reference's quality figure: PRDN[%] of a decoded block against its original ------------------------------
 * What test_packer_ prints behind a round trip (lib_rspt_test/rspt_test.cpp:98-111), the only quality figure the reference
 * publishes for its lossy packers, on nblocks device-resident blocks, bit-identical with the reference's x86-64 build.  Per
 * block, with o the original and d the decoded block, each read into int32 per channel as convert_native_to_i32 does:
 *     mse = 0.0; ref = 0.0                                   one pair of doubles for the WHOLE block
 *     for c in 0 .. nch-1:                                   channel outer, sample inner
 *         mean = (int32)(int64)((uint64)sum(o[c]) / (uint64)ns)      average_32: the division is UNSIGNED, so a negative channel
 *                                                                    sum at an ns that is not a power of two gives a garbage mean
 *         for s in 0 .. ns-1:
 *             t = (double)(int32)(o[c][s] - d[c][s])         the int32 subtraction wraps
 *             mse += t * t                                   double product, double sum, each rounded on its own
 *             r = (int32)((o[c][s] - mean) * (o[c][s] - mean))       int * int: the subtraction and the square WRAP, r may be negative
 *             ref += (double)r
 *     PRDN = sqrt(mse / ref) * 100.0                         correctly rounded divide, square root and product, no contraction
 * ref can be negative or zero: every NaN (the square root of a negative quotient, 0 / 0) is stored as the x86-64 default NaN
 * 0xFFF8000000000000; ref == 0 with mse > 0 gives +inf; d == o gives 0.0 (-0.0 under a negative ref).
 * Every term is an integer, so the sums are taken exactly in integers and in parallel where that provably equals the
 * reference's chain of rounded adds: mse = (double)sum(t^2) where the exact sum(t^2) <= 2^53, and ref = (double)sum(r) where
 * the exact sum(|r|) <= 2^53 (always so for nch * ns < 2^22) -- no partial sum then leaves +-2^53 and every add is exact.  A block
 * that misses a condition takes the sequential path: one workgroup adds that sum's terms in the reference's order (tens of
 * milliseconds per 2^22 samples; the blocks of a batch go side by side).
 *   d_orig, d_dec   nblocks blocks each of the handle's shape, interleaved native layout; only read; may be the same buffer.
 *                   The handle supplies the shape and the byte order (rspt_hip_set_byte_order); any packer kind will do.
 *                   16-byte aligned buffers (and block sizes, for nblocks > 1) are read with the widest loads
 *   d_prdn          [nblocks] doubles; required
 *   d_mse, d_ref    [nblocks] doubles, optional (NULL): the two accumulators as the reference leaves them
 *   d_path          [nblocks] uint32, optional (NULL): 0 where the block took the exact-integer path, 1 where the sequential one
 * RSPT_HIP_ERR_ARG for nblocks == 0, a NULL d_orig, d_dec or d_prdn, and nblocks * nch >= 2^31; more than 65535 blocks are
 * refused as by rspt_hip_reserve.  Asynchronous on `stream`, with the ordering contract of rspt_hip_compress_batch_dev: successive
 * calls on one handle are stream-ordered.  Nothing is allocated per call: the scratch (nblocks x nch channel sums, the per-block
 * accumulators) is part of the workspace that rspt_hip_reserve sizes.
 * Handles of more than 8191 channels: RSPT_HIP_ERR_UNSUPPORTED before anything is launched (see rspt_hip_iir_prefilter_batch_dev). */
int rspt_hip_prdn_batch_dev(rspt_hip_packer* p, const void* d_orig, const void* d_dec, size_t nblocks, double* d_prdn, double* d_mse,
                            double* d_ref, uint32_t* d_path, void* stream);

/* ---- PRDN on the planar int32 matrix ---------------------------------------------------------------------------------
 * The same figure on two [nblocks][nch][ns] int32 matrices, the form the reference itself computes it on (orig.d2d[j][i] and
 * enc.d2d[j][i] are rows of two tensor_i32, rspt_test.cpp:98-111).  One identity with the native entry is the contract:
 *     prdn_planar(O, D) == rspt_hip_prdn_batch_dev on a little-endian bps = 4 handle of the same (nch, ns), given
 *     i32_to_native(O) and i32_to_native(D)
 * in d_prdn, d_mse, d_ref and d_path, bit for bit.  The arithmetic text of rspt_hip_prdn_batch_dev applies word for word: the
 * UNSIGNED division of the mean, t and r that WRAP, the 2^53 conditions of the exact-integer path and the sequential path behind
 * them, every NaN stored as 0xFFF8000000000000, -0.0 under a negative ref.
 *   sample value    the whole int32 is the sample, as in the planar IIR and FIR entries: the handle supplies (nch, ns) and
 *                   nothing else; its bps and byte order have no effect.  On a handle of bps < 4 whose values lie inside the
 *                   sample width the result equals the native entry's on rspt_hip_i32_to_native_batch_dev of the two matrices
 *   d_orig, d_dec   block b's channel c at base + (b * nch + c) * ns; only read; may be the same buffer.  Both must be 4-byte
 *                   aligned (else RSPT_HIP_ERR_ARG); each may sit at any 4-byte offset of its own.  Rows are read with 16-byte
 *                   loads between a head and a tail of up to three samples (a row starts on a 16-byte boundary only where the
 *                   base does and ns % 4 == 0); d_dec is read at d_orig's sample positions, so its loads are 16-byte aligned
 *                   too where the two bases are congruent modulo 16
 *   d_prdn          [nblocks] doubles; required
 *   d_mse, d_ref, d_path   optional (NULL), as in rspt_hip_prdn_batch_dev
 * There is no 8191-channel cap: that is the native tile's, which this entry never touches; every channel count a handle can
 * have (65535) works.  The scratch is the native entry's (part of the workspace that rspt_hip_reserve sizes; nothing is
 * allocated per call), so native and planar calls may alternate on one handle.
 * Two forms, picked by the host (the constants are quality_planar.hip's): rows of up to 1024 samples take a wave
 * each, longer rows a workgroup; where a call has at least 1024 workgroups of whole rows of at most 8192 samples, a row's owner
 * takes the sum, the mean and the terms in one go (the row stays in registers up to 4096 samples, is read twice above); else a
 * pass of row sums and a pass of terms over spans of rows, three reads of the batch.  Measured on an MI355X
 * (tools/prdn_planar_bench.py, profiles/prdn_planar_bench.json): 64 x (64 ch x 65536) 0.552 ms (the native entry on the same
 * values 0.546, from_planar_i32 x 2 + the native entry 1.342); 1024 x (12 ch x 8192) 0.181 ms (0.211, 0.512).
 * RSPT_HIP_ERR_ARG for a NULL handle, d_orig, d_dec or d_prdn, nblocks == 0, nblocks * nch >= 2^31, a handle with an open feed,
 * a misaligned d_orig or d_dec, and a RSPT_HIP_KIND_BYTES handle (as the planar packer entries); more than 65535 blocks are
 * refused as by rspt_hip_reserve.  A refused call writes nothing.  Asynchronous on `stream`, with the ordering contract of
 * rspt_hip_compress_batch_dev: stream-ordered with every other call on the handle. */
int rspt_hip_prdn_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_orig, const int32_t* d_dec, size_t nblocks, double* d_prdn,
                                   double* d_mse, double* d_ref, uint32_t* d_path, void* stream);

/* ---- native <-> planar int32: the reference's convert_native_to_i32 / convert_i32_to_native as stages ---------------
 * What every program of the reference runs first and last (lib_signalpacker/utils.cpp:51-191; rspt_test.cpp:62-64, 92-94,
 * 119-135): the interleaved native block <-> a [channels][samples] int32 matrix, on nblocks device-resident blocks.
 *   d_native   nblocks blocks of the handle's shape in the compress layout (sample-major, bps bytes per sample, in the byte
 *              order of rspt_hip_set_byte_order); any alignment -- 16-byte aligned buffers take the widest accesses
 *   d_planar   [nblocks][nch][ns] int32, 4-byte aligned (16-byte aligned buffers take the widest accesses)
 * native -> i32 sign-extends every sample from bps bytes; i32 -> native keeps the low bps bytes of every value.  Both are
 * bit-identical with the reference's functions for bps 1 - 4 and both values of reverse_byte_order, with one exception: the
 * byte order has no effect on one-byte samples, as everywhere in this library.  The reference's bps == 1 reversed store writes
 * at native + 1 (utils.cpp:115), one byte past the caller's buffer; that is not reproduced.
 * Any packer kind will do: the handle supplies (bps, nch, ns) and the byte order, nothing else of it is used -- the stages
 * allocate nothing and do not touch the workspace.  Handles of up to about a thousand channels with a 16-byte aligned d_native
 * run the tile kernels of the packers' own front end and inverse (i32 -> native: only the common int32 shape and handles of
 * fewer than 32 channels); everything else the 64 x 64 transposes k_wide_planar / k_wide_native.
 * RSPT_HIP_ERR_ARG for a NULL handle or pointer, nblocks == 0, nblocks * nch >= 2^31, a d_planar that is not 4-byte aligned
 * and any overlap of the two buffers; more than 65535 blocks are refused as by rspt_hip_reserve.  A refused call writes
 * nothing.  Asynchronous on `stream`, with the ordering contract of rspt_hip_compress_batch_dev. */
int rspt_hip_native_to_i32_batch_dev(rspt_hip_packer* p, const void* d_native, int32_t* d_planar, size_t nblocks, void* stream);
int rspt_hip_i32_to_native_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, void* d_native, size_t nblocks, void* stream);

/* The handle's own (non-blocking) stream, as a hipStream_t. */
void* rspt_hip_stream(rspt_hip_packer* p);

/* Wait for the handle's own stream. */
int rspt_hip_synchronize(rspt_hip_packer* p);

/* ---- measurement hooks ---------------------------------------------------- */

/* When enabled, every batch call brackets each kernel of the sequence with
 * HIP events on the launch stream.  rspt_hip_stage_times() then synchronises
 * and returns, for the LAST batch call, the per-stage elapsed milliseconds.
 * Stage names are returned by rspt_hip_stage_name(i). */
int rspt_hip_set_profiling(rspt_hip_packer* p, int on);
int rspt_hip_stage_count(const rspt_hip_packer* p);
const char* rspt_hip_stage_name(const rspt_hip_packer* p, int i);
int rspt_hip_stage_times(rspt_hip_packer* p, float* ms, int n);

/* Test hook: copy a workspace buffer of the LAST batch call to the host
 * (synchronises).  which: 0 planes [blocks][4][plane_stride] u8, 1 planar
 * int32 [blocks][N], 2 second int32 buffer (dct), 3 token histograms
 * [blocks*4*nblk][264] u32, 4 block records [..][4] u32 (mode, payload_len,
 * tree_bits, fill), 5 nb per block [blocks] u32, 6 means header bytes.
 * Returns the number of bytes copied (<= cap) or a negative status. */
long long rspt_hip_debug_read(rspt_hip_packer* p, int which, void* host_buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* RSPT_HIP_H_ */
