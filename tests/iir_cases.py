"""The IIR pre-filter stage (filter.hip): seeded inputs for its edges and a numpy restatement that keeps the doubles.

The reference (lib_rspt/lib_filter/iir_filter.cpp driven as rspt_test.cpp:116-136 drives it) runs init_history_values, i.e.
4 * init calls of filter() on the channel's first sample, then filter_opt() on every sample, and truncates each double
result with x86-64's conversion: every NaN, +-inf and every value whose truncation does not fit becomes INT32_MIN; the store
keeps the low bps bytes.  iir_double() restates that recurrence in float64 and returns the results BEFORE the truncation,
so that the tests can see which outputs are in range, finite past 2^31, infinite or NaN, and where each class starts.

The cases feed tests/golden/make_iir_record.py, which records the compiled reference's answers in
tests/golden/iir_record.json: the non-finite cases (an unstable filter whose blow-up starts at a chosen sample, feed-forward
overflow, non-finite coefficients) and a finite matrix over the kernel variants (order, kernel, sample width, shape edges).
"""
import struct

import numpy as np

import cases
from fir_cases import INT32_MIN, crc, i32_to_native, native_to_i32, trunc_i32  # noqa: F401
from iir_model import IirModel

CHUNK_PIPE = 64  # k_iir_pipe: samples per chunk; the 16-sample fast path runs on full chunks only
CHUNK_IIR = 16  # k_iir: samples per chunk, then a tail sample by sample

# one stable set per order, each with a gain above one somewhere, so that full-scale int32 input overflows both ways
STABLE = {
    2: ([1.0, 0.5], [1.0, -1.0]),
    3: cases.IIR_HIGHPASS,
    4: ([1.0, -1.2, 0.5, -0.05], [0.1, 0.2, 0.2, 0.1]),
    5: (cases.IIR_BANDPASS[0], [3.0 * v for v in cases.IIR_BANDPASS[1]]),  # the harness's band-pass at three times its gain
}


def kernel_of(ns, init, nc):
    """which kernel rspt_hip_iir_prefilter_batch_dev runs (launch_iir): the pipelined one needs a full chunk and a history"""
    return "pipe" if ns >= CHUNK_PIPE and 4 * init >= nc - 1 else "iir"


# ---- the restatement ----

def iir_double(native, bps, nch, ns, n, d, init, shared=True, nblocks=1):
    """[nblocks][ns][nch] float64: the reference's outputs before the truncation.  shared: one filter per block, its state
    running on from channel to channel (the harness); else a fresh filter per channel"""
    x = native_to_i32(native, bps, nch, ns * nblocks).reshape(nblocks, ns, nch).astype(np.float64)
    y = np.empty((nblocks, ns, nch), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        if shared:
            # (one block: Python floats, the same IEEE doubles at far less overhead per operation; else a lane per block)
            f = IirModel(n, d, 0.0 if nblocks == 1 else np.zeros(nblocks))
            for c in range(nch):
                col = x[0, :, c].tolist() if nblocks == 1 else list(x[:, :, c].T)
                f.init_history(col[0], 4 * init)
                y[:, :, c] = np.array(f.run(col)).T
        else:
            lanes = x.transpose(1, 0, 2).reshape(ns, nblocks * nch)
            f = IirModel(n, d, np.zeros(nblocks * nch))
            f.init_history(lanes[0], 4 * init)
            y[:] = np.array(f.run(list(lanes))).reshape(ns, nblocks, nch).transpose(1, 0, 2)
    return y


def iir_prefilter(native, bps, nch, ns, n, d, init, shared=True, nblocks=1):
    """the filtered blocks in the native sample width, as rspt_hip_iir_prefilter_batch_dev writes them"""
    return i32_to_native(trunc_i32(iir_double(native, bps, nch, ns, n, d, init, shared, nblocks)), bps)


CLASSES = ("in_range", "past_2^31", "inf", "nan")


def classify(y):
    """class name -> mask over y: in range of int32 after truncation, finite but past it, +-inf, NaN"""
    fits = (y > -2147483649.0) & (y < 2147483648.0)
    return {"in_range": fits, "past_2^31": np.isfinite(y) & ~fits, "inf": np.isinf(y), "nan": np.isnan(y)}


def onset(mask, ch):
    """the first sample of channel ch where a [ns][nch] mask holds, or None"""
    m = np.asarray(mask)[:, ch]
    return int(np.argmax(m)) if m.any() else None


def in_region(region, s, ns):
    """region of sample s that a claim names: strictly inside a full chunk of k_iir_pipe (neither its first nor its last
    sample), in its last partial chunk, strictly inside a 16-sample chunk of k_iir, or in k_iir's tail"""
    if region == "pipe_full":
        return s < ns // CHUNK_PIPE * CHUNK_PIPE and 0 < s % CHUNK_PIPE < CHUNK_PIPE - 1
    if region == "pipe_tail":
        return ns % CHUNK_PIPE != 0 and s >= ns // CHUNK_PIPE * CHUNK_PIPE
    if region == "iir_chunk":
        return s < ns // CHUNK_IIR * CHUNK_IIR and 0 < s % CHUNK_IIR < CHUNK_IIR - 1
    if region == "iir_tail":
        return s >= ns // CHUNK_IIR * CHUNK_IIR
    if region == "start":
        return s == 0
    raise ValueError(region)


# ---- coefficients, exactly (NaN signs included) ----

NAN_NEG = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]  # x86's default NaN: sign bit set
NAN_POS = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]


def to_bits(v):
    return ["%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0] for x in v]


def from_bits(h):
    return [struct.unpack("<d", struct.pack("<Q", int(x, 16)))[0] for x in h]


# ---- inputs ----

def onset_block(nch, ns, bps, seed, onsets, amp):
    """channel c is zero before sample onsets[c] (None: zero throughout) and random within +-amp from there on"""
    x = cases.hash_i32(nch * ns, seed, amp).astype(np.int64).reshape(ns, nch)
    for c, k in enumerate(onsets):
        x[: ns if k is None else k, c] = 0
    lim = 1 << (8 * bps - 1)
    x = ((x + lim) % (2 * lim) - lim).astype(np.int32)
    return np.ascontiguousarray(x.view(np.uint8).reshape(-1, 4)[:, :bps]).reshape(-1)


def unstable(g, nc=3):
    """y = 0.5 x + 0.5 x' + g y' - 0 y'' (...): grows by g per sample once fed, and the zero feedback coefficient turns the
    first +-inf into NaN two samples later (0 * inf), as inf - inf would"""
    return [1.0, -g] + [0.0] * (nc - 2), [0.5, 0.5] + [0.0] * (nc - 2)


def iir_edge_cases():
    """name, bps, nch, ns, n, d, init, data, claims: [(mode, class, channel, region)] -- in that mode, the first output of
    the class in that channel lies in that region of its samples (region None: the channel holds none of the class)"""
    C = []

    def add(name, bps, nch, ns, coef, init, data, claims=()):
        data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).reshape(-1))
        assert data.size == bps * nch * ns, name
        C.append(dict(name=name, bps=bps, nch=nch, ns=ns, n=[float(v) for v in coef[0]], d=[float(v) for v in coef[1]], init=init,
                      data=data, claims=list(claims)))

    both = ("shared", "per_channel")

    def at(cls, ch, region, modes=both):
        return [(m, cls, ch, region) for m in modes]

    def finite(ch):
        return at("past_2^31", ch, None) + at("inf", ch, None) + at("nan", ch, None)

    # -- an unstable filter whose blow-up starts at a chosen place: zeros in front of the onset --
    # channel 0 zero throughout (finite), channel 1 zero up to the onset, channel 2 random: shared mode carries channel 1's
    # NaN through the history initialisation into channel 2, per channel mode blows channel 2 up on its own
    g15 = unstable(1.5)
    add("ex3x3000_i32_unstable_nan_in_full_chunk", 4, 3, 3000, g15, 3, onset_block(3, 3000, 4, 101, [None, 1000, 0], 1000),
        finite(0) + at("inf", 1, "pipe_full") + at("nan", 1, "pipe_full") + at("past_2^31", 1, "pipe_full")
        + [("shared", "nan", 2, "start"), ("per_channel", "inf", 2, "pipe_full")])
    add("ex3x3000_i32_unstable_nan_in_last_chunk", 4, 3, 3000, g15, 3, onset_block(3, 3000, 4, 102, [None, 1215, 0], 1000),
        finite(0) + at("nan", 1, "pipe_tail"))
    g1e3 = unstable(1e3)
    add("onset2x500_i32_k_iir_nan_in_chunk", 4, 2, 500, g1e3, 0, onset_block(2, 500, 4, 103, [None, 300], 1000),
        at("nan", 1, "iir_chunk") + at("inf", 1, "iir_chunk"))
    add("onset2x500_i32_k_iir_nan_in_tail", 4, 2, 500, g1e3, 0, onset_block(2, 500, 4, 104, [None, 393], 1000),
        at("nan", 1, "iir_tail"))
    g4 = unstable(4.0, nc=4)
    add("onset4x700_i32_order3_pipe_shared_onset_in_ch2", 4, 4, 700, g4, 1, onset_block(4, 700, 4, 105, [None, None, 100, 0], 1000),
        finite(0) + finite(1) + at("nan", 2, "pipe_full") + [("shared", "nan", 3, "start"), ("per_channel", "nan", 3, "pipe_full")])
    g2 = unstable(2.0, nc=5)
    add("onset3x1200_i32_order4_pipe_nan_in_full_chunk", 4, 3, 1200, g2, 2, onset_block(3, 1200, 4, 106, [None, 100, 0], 1 << 20),
        at("nan", 1, "pipe_full"))
    # every sample width: the narrow ones pin the low bytes of INT32_MIN and of finite values past their range
    for bps, amp in ((1, 100), (2, 30000), (3, 1 << 22)):
        add("onset3x1500_i%d_unstable" % (8 * bps), bps, 3, 1500, unstable(2.0), 2, onset_block(3, 1500, bps, 110 + bps, [None, 200, 0], amp),
            at("nan", 1, "pipe_full") + at("past_2^31", 1, "pipe_full"))
        add("onset2x300_i%d_k_iir_unstable" % (8 * bps), bps, 2, 300, g1e3, 0, onset_block(2, 300, bps, 120 + bps, [None, 100], amp),
            at("nan", 1, "iir_chunk"))

    # -- feed-forward overflow: products near 1e308 overflow to +-inf, inf - inf is NaN (fir_cases' rand4x2000_i32_inf_nan) --
    add("ff_overflow4x2000_i32", 4, 4, 2000, ([1.0, -0.5, 0.25, 0.0], [1e308, -1e308, 0.5, 1e308]), 2,
        cases._rand_native(4, 2000, 4, 130, 1 << 30), at("nan", 0, "start"))
    for init, kern, region in ((1, "pipe", "pipe_full"), (0, "iir", "iir_chunk")):
        add("ff_overflow3x200_i32_onset_%s" % kern, 4, 3, 200, ([1.0, -0.5, 0.0], [1e300, 1e300, -1e300]), init,
            onset_block(3, 200, 4, 131, [None, 70, 0], 1 << 30), at("inf", 1, region) + at("nan", 1, region))

    # -- non-finite coefficients from the caller, in n and in d, through both kernels; n[0] is never read --
    for vname, v in (("nan", NAN_POS), ("negnan", NAN_NEG), ("inf", float("inf")), ("neginf", float("-inf"))):
        for where in ("n1", "d0", "dlast", "n0"):
            nc = 3 if where in ("n1", "n0") else 4
            n, d = [list(x) for x in STABLE[nc]]
            if where == "n0":
                n[0] = v
            elif where == "n1":
                n[1] = v
            elif where == "d0":
                d[0] = v
            else:
                d[-1] = v
            seed = 140 + len(C)
            for ns, init, kern in ((200, 2, "pipe"), (40, 1, "iir")):
                data = cases._rand_native(3, ns, 4, seed + ns, 1 << 20)
                claims = finite(0) + finite(1) + finite(2) if where == "n0" else at("nan", 0, "start")
                add("coef_%s_%s_%s3x%d_i32" % (where, vname, kern, ns), 4, 3, ns, (n, d), init, data, claims)
    return C


def iir_matrix_cases():
    """finite cases over the kernel variants: every order with its stable set, both kernels, every sample width at up to its
    full scale, the shape edges (ns around the chunk sizes, a clamped last producer set, channel counts around a wave)"""
    C = []

    def add(name, bps, nch, ns, nc, init, amp, seed):
        n, d = STABLE[nc]
        C.append(dict(name=name, bps=bps, nch=nch, ns=ns, n=[float(v) for v in n], d=[float(v) for v in d], init=init,
                      data=cases._rand_native(nch, ns, bps, seed, amp), claims=[]))

    full = {1: 127, 2: 32767, 3: (1 << 23) - 1, 4: (1 << 31) - 1}
    k = 0
    for nc in (2, 3, 4, 5):
        for ns in sorted({1, nc - 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 232}):
            inits = (0, 1 + k % 5) if ns >= CHUNK_PIPE else ((0, 1 + k % 3) if ns <= 17 else (5,))
            for init in inits:
                bps = 1 + k % 4
                amp = full[bps] if k % 3 else max(1, full[bps] >> 6)
                add("m_nc%d_ns%d_init%d_i%d_x3" % (nc, ns, init, 8 * bps), bps, 3, ns, nc, init, amp, 2000 + k)
                k += 1
    # channel counts around one wave (one lane per channel in per channel mode), every order, both kernels
    for i, nch in enumerate((1, 63, 64, 65, 129)):
        bps = 4 - i % 4
        add("w_nc%d_ns100_init2_i%d_x%d" % (2 + i % 4, 8 * bps, nch), bps, nch, 100, 2 + i % 4, 2, full[bps], 2100 + i)
        add("w_nc%d_ns40_init3_i%d_x%d" % (5 - i % 4, 8 * bps, nch), bps, nch, 40, 5 - i % 4, 3, full[bps], 2110 + i)
    # full-scale int32 at a length of many chunks: every order overflows both ways and redoes chunks with INT_MAX
    for nc in (2, 3, 4, 5):
        add("fs_nc%d_ns2000_init50_i32_x3" % nc, 4, 3, 2000, nc, 50, full[4], 2200 + nc)
    return C


def all_cases():
    return iir_edge_cases() + iir_matrix_cases()
