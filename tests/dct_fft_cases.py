"""The dct's FFT kernels held to exact values: inputs, a long-double reference of both directions and the comparator.

The FFT kernels (k_dctr_*, k_idctr_*, k_dctfft_* in rspt_amd/csrc/transforms.hip) evaluate the reference's definition
(signal_packer_dct.cpp:76-100) in fp64 through an FFT, so they are not bit-exact with the reference's float32 table -- but
against the SAME definition evaluated in long double they can only differ where a value lies within their own rounding error
of a truncation boundary.  That error is a few eps * max|v| of a row (eps = 2^-52); check_exact allows one count inside a band
of 2^14 eps max|v| around the non-zero integers and nothing anywhere else.  The band is derived, not tuned: scipy's fp64 DCT
errs by about 2 eps max|v| against its long-double DCT on these inputs (tests/golden/dct_fft_exact_record.json keeps the
figure per case), and 2^14 leaves three orders of magnitude over that.

The inputs are chosen so that almost nothing falls into the band (CAP): a case whose long-double reference has more than
1e-3 of its values there tests the inputs, not the kernels.  That is checked on the CPU (tests/test_dct_fft_exact_record.py).
"""
import ctypes as C
import functools
import hashlib

import numpy as np

import lossy_quantizer_cases as lq

EPS = 2.0 ** -52
BAND = 2.0 ** 14 * EPS  # half-width of the band around an integer, in units of a row's max|v|
CAP = 1e-3              # largest share of a case's values that may lie in the band
LD = np.longdouble


# ---- the cases ----------------------------------------------------------------------------------------------------------------

def _case(name, src, k, nch, nblocks, bps=4, q=128.0, nb=2, planar=False, inverse=True, seed=0, forced=None):
    ns = 1 << k
    return dict(name=name, src=src, k=k, ns=ns, nch=nch, nblocks=nblocks, bps=bps, q=float(q), nb=nb, planar=planar, inverse=inverse,
                seed=seed, forced=(k <= 13) if forced is None else forced)


def _shape(k):
    """channels and blocks of the sweep: three channels and two blocks while that is cheap"""
    return (3, 2) if k <= 16 else (2, 1) if k <= 19 else (1, 1)


PLANAR_K = (5, 17, 21)          # also from a planar matrix: odd complex form, lw = 2, lb = 8
FULL_K = (5, 7, 12, 17, 19, 21)  # full-scale input: the (float) cast rounds, four planes
BPS3_K = (9, 17)


def sweep_cases():
    """every k = log2 ns the FFT path takes, 4 .. 22: RSPT_HIP_DCT_FORCE_FFT up to 2^13, the natural route beyond"""
    out = []
    for k in range(4, 23):
        nch, nblocks = _shape(k)
        out.append(_case("noise_k%02d" % k, "noise", k, nch, nblocks, planar=k in PLANAR_K, seed=1000 + k))
    for k in BPS3_K:
        nch, nblocks = _shape(k)
        out.append(_case("noise_i24_k%02d" % k, "noise", k, nch, nblocks, bps=3, seed=1100 + k))
    for k in FULL_K:
        nch, nblocks = _shape(k)
        # no inverse leg: decoded values reach 2^30, where the band is 2^-8 wide and holds 0.8 % of all values -- eight times
        # the cap (the record keeps the measured share of each as inverse_share_not_run)
        out.append(_case("full_k%02d" % k, "full", k, nch, nblocks, nb=4, planar=k in PLANAR_K, inverse=False, seed=1200 + k))
    return out


LARGE_NS = [(4, 3, 16384, 2), (3, 2, 32768, 1), (4, 64, 65536, 1), (4, 2, 262144, 1), (4, 1, 1048576, 1), (4, 1, 4194304, 1)]  # bps, nch, ns, nblocks


def large_ns_cases():
    """the ECG-like blocks of test_gpu_dct_fft.py::test_dct_large_ns (most coefficients truncate to 0: the sparse-plane route of
    the hzr stages behind the transform)"""
    return [_case("ecg_%dx%d_i%d" % (nch, ns, 8 * bps), "ecg", ns.bit_length() - 1, nch, nblocks, bps=bps, inverse=False, seed=11, forced=False)
            for bps, nch, ns, nblocks in LARGE_NS]


MULTIPASS = dict(nch=16, k=20, nblocks=6, checked_block=4, seed=1300)  # 16 ch x 2^20: 256 MiB of FFT scratch a block, four to a pass


def multipass_case():
    """block 4 -- the first of the second pass -- of the batch that needs more than one pass over the FFT scratch"""
    m = MULTIPASS
    return _case("noise_16x1048576_block4", "noise", m["k"], m["nch"], 1, inverse=False, seed=m["seed"] + m["checked_block"], forced=False)


def all_cases():
    return sweep_cases() + large_ns_cases() + [multipass_case()]


def by_name():
    return {c["name"]: c for c in all_cases()}


# ---- the inputs ---------------------------------------------------------------------------------------------------------------

def _channel_means(nch, seed):
    """a mean per channel, alternating in sign"""
    c = np.arange(nch, dtype=np.int64)
    return (((c + seed) & 1) * 2 - 1) * (700 + 37 * c + 11 * (seed % 50))


def block_i32(c, i):
    """block i of a case as int32 [nch, ns]"""
    nch, ns, seed = c["nch"], c["ns"], c["seed"] + i
    if c["src"] == "ecg":
        from rspt_amd import synth

        native = synth.synth_native(nch, ns, block_index=seed, bps=c["bps"], ecg=True).numpy().reshape(-1)
        return lq.native_to_i32(native, c["bps"], nch, ns)
    rng = np.random.default_rng(seed)
    if c["src"] == "noise":
        # sigma 38400: coefficients of sigma 300 at quality 128, > 99.7 % of them non-zero, everything within two planes and
        # within 24 bits (the (float) cast is exact)
        x = np.rint(rng.standard_normal((nch, ns)) * 38400.0).astype(np.int64)
    else:
        x = rng.integers(-(1 << 30), 1 << 30, size=(nch, ns), dtype=np.int64)  # the (float) cast rounds; coefficients reach 2e7
    return np.ascontiguousarray((x + _channel_means(nch, seed)[:, None]).astype(np.int32))


def block_native(c, x):
    return lq.i32_to_native(x, c["bps"])


def new_packer(api, c):
    pk = api.SignalPacker(api.KIND_DCT | (api.DCT_FORCE_FFT if c["forced"] else 0), c["bps"], c["nch"], c["ns"], 2)
    if (c["q"], c["nb"]) != lq.DEFAULTS["dct"]:
        pk.set_quantizer(quality=c["q"], nb=c["nb"])
    return pk


# ---- the long-double reference -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _orc():
    from oracle.oracle import Oracle

    return Oracle()


def _centred(x):
    """(float)(x - mean) of signal_packer_dct.cpp:80,108-109 and the means (average_32, the oracle's)"""
    x = np.ascontiguousarray(x, dtype=np.int32)
    means = np.array([_orc().average_32(row) for row in x], dtype=np.int32)
    return (x.view(np.uint32) - means.view(np.uint32)[:, None]).view(np.int32).astype(np.float32), means


def _forward(s, ns, q, dtype):
    import scipy.fft

    csum = scipy.fft.dct(s.astype(dtype), type=2, axis=1) * dtype(0.5)  # sum_x s[x] cos(pi (2x + 1) i / 2n)
    s0, s1, _ = lq.dct_scales(ns, q)  # Cs[i] * sqrt(2/n) / quality in double, Cs[0] the float 1/sqrt 2: as oracle.dct_big_compress
    scale = np.full(ns, s1, dtype=np.float64)
    scale[0] = s0
    return csum * scale.astype(dtype)[None, :]


def exact_forward(x_i32, ns, q=128.0):
    """transform_dct (signal_packer_dct.cpp:76-87, 102-116) of int32 [nch, ns] in long double -> (v untruncated, means int32)"""
    s, means = _centred(x_i32)
    return _forward(s, ns, q, LD), means


def fp64_forward(x_i32, ns, q=128.0):
    """the same through scipy's fp64 DCT: what oracle.dct_big_compress truncates"""
    s, _ = _centred(x_i32)
    return _forward(s, ns, q, np.float64)


def _inverse(coeffs, ns, q, dtype):
    import scipy.fft

    co = np.ascontiguousarray(coeffs, dtype=np.int32)
    y = co.astype(np.float32).astype(dtype)
    y[:, 0] = (lq.CS0 * co[:, 0].astype(np.float32)).astype(dtype)  # Cs[0] * dct[0], a float product (dct.cpp:95)
    y[:, 1:] *= dtype(0.5)  # scipy's type 3 is Y0 + 2 sum_{x > 0} Y[x] cos(pi (2i + 1) x / 2n)
    return scipy.fft.dct(y, type=3, axis=1) * dtype(lq.dct_scales(ns, q)[2])


def exact_inverse(coeffs, means24, ns, q=128.0):
    """transform_idct (signal_packer_dct.cpp:89-100) of int32 coefficients [nch, ns] in long double, as oracle.dct_big_decompress
    does it in fp64 -> the untruncated values before the mean is added; a decoded sample is trunc(v) + means24 wrapped to int32
    (decoded_minus_mean undoes that)."""
    means24 = np.asarray(means24)
    assert means24.shape == (np.asarray(coeffs).shape[0],) and (np.abs(means24.astype(np.int64)) <= 1 << 23).all()
    return _inverse(coeffs, ns, q, LD)


def fp64_inverse(coeffs, ns, q=128.0):
    return _inverse(coeffs, ns, q, np.float64)


def means24_of(means):
    """what the header keeps of a mean: its low 24 bits, sign-extended"""
    return ((np.asarray(means, dtype=np.int32).astype(np.int64) << 8).astype(np.int32) >> 8).astype(np.int32)


def header_bytes(means):
    return np.ascontiguousarray(np.asarray(means, dtype="<i4")).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()


def decoded_minus_mean(dec_i32, means24):
    return (np.ascontiguousarray(dec_i32, dtype=np.int32).view(np.uint32) - np.asarray(means24, dtype=np.int32).view(np.uint32)[:, None]).view(np.int32)


# ---- the comparator -----------------------------------------------------------------------------------------------------------

def band_of(v):
    """bool [rows, n]: v within BAND * max|v| (of its row) of an integer other than zero -- truncation goes toward zero, so zero
    is no boundary"""
    a = np.abs(v)
    delta = (a.max(axis=1) * LD(BAND))[:, None]
    return (np.abs(v - np.rint(v)) < delta) & (a >= LD(0.5))


def check_exact(got_i32, v, what, stats=None):
    """got == trunc(v) outside the band, |got - trunc(v)| <= 1 inside it -> the band's share of the values.  stats (a dict) is
    given the counts: values, band, flips (values inside the band that differ)."""
    v = np.asarray(v, dtype=LD)
    v = v.reshape(-1, v.shape[-1])
    got = np.asarray(got_i32).reshape(v.shape).astype(np.int64)
    assert (np.abs(v) < LD(2.0 ** 31)).all(), what
    want = np.trunc(v).astype(np.int64)
    band = band_of(v)
    d = got - want
    bad = np.where(band, np.abs(d) > 1, d != 0)
    if stats is not None:
        stats.update(values=int(v.size), band=int(band.sum()), flips=int((band & (d != 0)).sum()))
    if bad.any():
        rows, cols = np.nonzero(bad)
        lines = ["[%d, %d] got %d v %.6f boundary %.3g away, band %.3g" % (r, i, got[r, i], float(v[r, i]), float(abs(v[r, i] - np.rint(v[r, i]))),
                                                                           float(np.abs(v[r]).max() * LD(BAND))) for r, i in list(zip(rows, cols))[:6]]
        raise AssertionError("%s: %d of %d values outside the rule (first: %s)" % (what, int(bad.sum()), v.size, "; ".join(lines)))
    return float(band.mean())


def digest(v):
    """what the record keeps of trunc(v)"""
    return hashlib.sha256(np.ascontiguousarray(np.trunc(v).astype(np.int64).astype("<i4")).tobytes()).hexdigest()[:16]


# ---- coefficients out of a stream ------------------------------------------------------------------------------------------------

def stream_coeffs(orc, stream, c):
    """a dct stream -> (coefficients int32 [nch, ns], header bytes): orc_packer_decompress_coeffs for the reference's own
    quantiser, the stream helpers of lossy_quantizer_cases.py for four planes"""
    nch, ns = c["nch"], c["ns"]
    header = bytes(stream[1:1 + 3 * nch])
    if c["nb"] != lq.DEFAULTS["dct"][1]:
        co, _, used = lq.stream_values(orc, stream, "dct", nch, ns, c["nb"])
        assert used == len(stream)
        return np.ascontiguousarray(co), header
    s = np.frombuffer(bytes(stream) + b"\0" * 16, dtype=np.uint8).copy()
    co, me, used = np.zeros((nch, ns), dtype=np.int32), np.zeros(nch, dtype=np.int32), C.c_size_t(0)
    pk = orc.packer("dct", c["bps"], nch, ns)
    f = orc.lib.orc_packer_decompress_coeffs
    f.restype = C.c_int
    rc = f(C.c_void_p(pk._h), s.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(used), co.ctypes.data_as(C.POINTER(C.c_int32)),
           me.ctypes.data_as(C.POINTER(C.c_int32)))
    pk.close()
    assert rc == 0 and used.value == len(stream)
    assert header_bytes(me) == header
    return co, header


def coeff_mismatch(orc, a, b, bps, nch, ns):
    """two dct streams by their coefficients, decoded by the oracle: (the share that differs, the largest difference)"""
    def coeffs(stream):
        s = np.frombuffer(stream + b"\0" * 16, dtype=np.uint8).copy()
        co = np.zeros((nch, ns), dtype=np.int32)
        me = np.zeros(nch, dtype=np.int32)
        used = C.c_size_t(0)
        pk = orc.packer("dct", bps, nch, ns)
        f = orc.lib.orc_packer_decompress_coeffs
        f.restype = C.c_int
        rc = f(C.c_void_p(pk._h), s.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(used), co.ctypes.data_as(C.POINTER(C.c_int32)),
               me.ctypes.data_as(C.POINTER(C.c_int32)))
        pk.close()
        assert rc == 0
        return co, me

    ca, ma = coeffs(a)
    cb, mb = coeffs(b)
    assert (ma == mb).all()
    d = np.abs(ca.astype(np.int64) - cb.astype(np.int64))
    return float((d != 0).mean()), int(d.max())
