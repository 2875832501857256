"""The FIR pre-filter stage: its test inputs and a numpy restatement of the reference.

The cases feed tests/golden/make_fir_record.py, which records the compiled reference's answers in
tests/golden/fir_record.json.  The tests take the coefficients from that record (stored exactly: kernel_to_record), so they
do not depend on numpy's window functions being bit-stable; the inputs are integer arithmetic or the shipped recordings, and the
record holds their crc32.
"""
import numpy as np

import cases
from casetools import crc  # noqa: F401  (fc.crc: the tests and generators use it beside the sample readers)
from rspt_amd import synth

INT32_MIN = -(1 << 31)


def native_to_i32(native, bps, nch, ns):
    """[ns][nch] int32 from little-endian native samples of bps bytes"""
    b = np.frombuffer(np.ascontiguousarray(native).tobytes(), dtype=np.uint8)[: bps * nch * ns].reshape(ns * nch, bps)
    x = np.zeros(ns * nch, dtype=np.int64)
    for i in range(bps):
        x |= b[:, i].astype(np.int64) << (8 * i)
    sign = np.int64(1) << (8 * bps - 1)
    x = (x ^ sign) - sign
    return x.astype(np.int32).reshape(ns, nch)


def i32_to_native(y, bps):
    """the low bps bytes of every int32, little-endian (convert_i32_to_native)"""
    b = np.ascontiguousarray(y, dtype=np.int32).reshape(-1).view(np.uint8).reshape(-1, 4)[:, :bps]
    return np.ascontiguousarray(b).reshape(-1)


def trunc_i32(y):
    """(int32_t) of a double as the reference's x86-64 build does it (cvttsd2si): NaN, +-inf and every value whose
    truncation does not fit give INT32_MIN"""
    ok = (y > -2147483649.0) & (y < 2147483648.0)  # (False for NaN)
    return np.where(ok, np.trunc(np.where(ok, y, 0.0)), INT32_MIN).astype(np.int64).astype(np.int32)


def fir_i32(x, kernel):
    """y[t][c] = ((((0.0 + x[t-K+1][c] k[0]) + x[t-K+2][c] k[1]) + ...) + x[t][c] k[K-1]), x[s < 0][c] = x[0][c]: the
    double sums of i_filter::filter_opt after init_history_values, every product and sum rounded on its own"""
    k = np.asarray(kernel, dtype=np.float64)
    K = k.size
    ns = x.shape[0]
    xd = x.astype(np.float64)
    pad = np.concatenate([np.repeat(xd[:1], K - 1, axis=0), xd], axis=0)
    y = np.zeros(xd.shape, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(K):
            y = y + pad[i : i + ns] * k[i]
    return y


def fir_prefilter(native, bps, nch, ns, kernel):
    """the filtered block in the native sample width (bytes), as rspt_hip_fir_prefilter_batch_dev writes it"""
    return i32_to_native(trunc_i32(fir_i32(native_to_i32(native, bps, nch, ns), kernel)), bps)


# ---- coefficient sets (made here once; the record keeps them exactly) ----

def windowed_sinc_bandpass(K, lo, hi):
    """linear-phase band-pass, cut-offs as fractions of the sampling rate, Hamming window, unit gain at the centre"""
    n = np.arange(K) - (K - 1) / 2.0
    h = 2 * hi * np.sinc(2 * hi * n) - 2 * lo * np.sinc(2 * lo * n)
    h = h * np.hamming(K) if K > 1 else h
    c = (lo + hi) / 2.0
    g = np.abs(np.sum(h * np.exp(-2j * np.pi * c * np.arange(K))))
    return h / g if g > 0 else h


def windowed_sinc_lowpass(K, fc):
    n = np.arange(K) - (K - 1) / 2.0
    h = 2 * fc * np.sinc(2 * fc * n)
    if K > 1:
        h = h * np.hamming(K)
    return h / np.sum(h)


def _rand_kernel(K, seed, exp):
    """K taps in {-8/2^exp, ..., 7/2^exp}: random, and exactly one hex digit each in the record (kernel_to_record)"""
    return cases.hash_i32(K, seed, 8).astype(np.float64) * 2.0 ** -exp


def kernel_to_record(kernel):
    """the coefficients, exactly: {"hex": [float.hex, ...]}, or -- where every tap is (d - 8) / 2^exp with a hex digit d and one
    exp, as in the long random kernels -- {"digits": "...", "exp": exp}, one character per tap instead of twenty"""
    k = np.asarray(kernel, dtype=np.float64)
    for exp in range(0, 40):
        with np.errstate(over="ignore", invalid="ignore"):
            q = k * 2.0 ** exp
        if k.size > 64 and np.all(q == np.round(q)) and np.all((q >= -8) & (q < 8)):
            return {"digits": "".join("%x" % (int(v) + 8) for v in q), "exp": exp}
    return {"hex": [float.hex(float(v)) for v in k]}


def kernel_from_record(rec):
    if "hex" in rec:
        return np.array([float.fromhex(h) for h in rec["hex"]], dtype=np.float64)
    d = np.frombuffer(rec["digits"].encode(), dtype=np.uint8)
    v = np.where(d >= ord("a"), d - ord("a") + 10, d - ord("0")).astype(np.float64) - 8.0
    return v * 2.0 ** -rec["exp"]


def fir_cases():
    """name, bps, nch, ns, kernel, data (native bytes)"""
    ecg = np.frombuffer(synth.ecg_12ch_i32(), dtype=np.uint8)
    ds = np.frombuffer(synth.data_stream_3ch_i24(), dtype=np.uint8)
    C = []

    def add(name, bps, nch, ns, kernel, data):
        data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).reshape(-1)[: bps * nch * ns])
        assert data.size == bps * nch * ns, name
        C.append(dict(name=name, bps=bps, nch=nch, ns=ns, kernel=[float(v) for v in np.asarray(kernel, dtype=np.float64)], data=data))

    full32 = np.array([(1 << 31) - 1, INT32_MIN], dtype=np.int32)
    add("ecg12x34199_i32_bandpass101", 4, 12, 34199, windowed_sinc_bandpass(101, 0.0005, 0.08), ecg)
    add("ecg12x34199_i32_lowpass1001", 4, 12, 34199, windowed_sinc_lowpass(1001, 0.02), ecg)
    add("ds3x20000_i24_bandpass255", 3, 3, 20000, windowed_sinc_bandpass(255, 0.002, 0.1), ds)
    add("ds3x20000_i24_k1_gain", 3, 3, 20000, [0.75], ds)
    add("synth5x3000_i16_lowpass31", 2, 5, 3000, windowed_sinc_lowpass(31, 0.1), synth.synth_native(5, 3000, 3, bps=2, ecg=True).numpy())
    add("rand7x1001_i8_k2", 1, 7, 1001, [0.5, 0.5], cases._rand_native(7, 1001, 1, 61, 100))
    add("rand7x1001_i8_moving_average31", 1, 7, 1001, [1.0 / 31] * 31, cases._rand_native(7, 1001, 1, 62, 128))
    add("synth4x2500_i32_differentiator", 4, 4, 2500, [1.0, 0.0, -2.0, 0.0, 1.0], synth.synth_native(4, 2500, 4, ecg=True).numpy())
    add("rand1x5000_i32_bandpass101", 4, 1, 5000, windowed_sinc_bandpass(101, 0.01, 0.2), cases._rand_native(1, 5000, 4, 63, 1 << 24, walk=True))
    add("rand1x3000_i16_k4097", 2, 1, 3000, _rand_kernel(4097, 64, 9), cases._rand_native(1, 3000, 2, 71, 1 << 12, walk=True))
    add("rand3x700_i24_k4097", 3, 3, 700, _rand_kernel(4097, 65, 9), cases._rand_native(3, 700, 3, 66, 1 << 22))
    add("rand2x40_i32_k65536", 4, 2, 40, _rand_kernel(65536, 67, 11), cases._rand_native(2, 40, 4, 68, 1 << 22))
    add("full_scale6x3000_i32_gain_overflow", 4, 6, 3000, windowed_sinc_lowpass(31, 0.05) * 1.7,
        np.where(cases.hash_i32(6 * 3000, 69, 4) >= 0, full32[0], full32[1]).astype(np.int32).view(np.uint8))
    # a huge coefficient overflows a product to +-inf; inf + (-inf) is NaN: both truncate to INT32_MIN
    add("rand4x2000_i32_inf_nan", 4, 4, 2000, [1e308, -1e308, 0.5, 1e308], cases._rand_native(4, 2000, 4, 70, 1 << 30))
    return C


BIG = dict(name="synth64x65536_i32_bandpass255", bps=4, nch=64, ns=65536, block=7)


def big_kernel():
    return windowed_sinc_bandpass(255, 0.001, 0.1)


def big_data():
    return synth.synth_native(BIG["nch"], BIG["ns"], BIG["block"], bps=BIG["bps"], ecg=True).numpy()
