"""The PRDN stage: its test inputs and a numpy restatement of the reference.

What the reference's test_packer_ computes behind a round trip (lib_rspt_test/rspt_test.cpp:98-111), with o the original and d
the decoded block as int32 per channel:
    mse = ref = 0.0
    for c:  mean = (int32)(int64)((uint64)sum(o[c]) / (uint64)ns)            average_32: unsigned division
            for s:  t = (int32)(o - d);  mse += (double)t * (double)t
                    r = (int32)((o - mean) * (o - mean));  ref += (double)r   int * int: wraps
    PRDN = sqrt(mse / ref) * 100.0                                            a NaN is the x86-64 default NaN 0xFFF8000000000000
Every term is an integer: mse is exactly (double)sum(t^2) where that sum is at most 2^53, ref exactly (double)sum(r) where
sum(|r|) is at most 2^53; only outside these conditions does the order of the rounded adds matter (`path` 1: the GPU stage's
sequential path).  The cases feed tests/golden/make_prdn_record.py, which records the compiled reference's PRDN in
tests/golden/prdn_record.json; the inputs are integer arithmetic or the shipped recordings, and the record holds their crc32.
"""
import struct

import numpy as np

import cases
from casetools import _i32, crc  # noqa: F401
from fir_cases import i32_to_native, native_to_i32  # noqa: F401

NAN_BITS = 0xFFF8000000000000  # what the reference's x86-64 build returns for sqrt of a negative and for 0 / 0
EXACT_LIMIT = 1 << 53


def bits(x):
    """the bit pattern of a double as an int; every NaN is the x86-64 default NaN"""
    x = float(x)
    return NAN_BITS if x != x else struct.unpack("<Q", struct.pack("<d", x))[0]


def hexbits(x):
    return "%016x" % bits(x)


def average_32(o):
    """[ns][nch] int32 -> the reference's mean per channel (utils.cpp:30-40: the int64 sum is divided as an unsigned)"""
    s = o.astype(np.int64).sum(axis=0)
    q = s.astype(np.uint64) // np.uint64(o.shape[0])
    return q.astype(np.int64).astype(np.int32)  # (both conversions keep the low bits)


def terms(o, d):
    """[ns][nch] int32 x 2 -> (t, r) int64 arrays holding the reference's int32 values"""
    t = (o.astype(np.int64) - d.astype(np.int64)).astype(np.int32).astype(np.int64)
    dm = (o.astype(np.int64) - average_32(o).astype(np.int64)[None, :]).astype(np.uint32).astype(np.uint64)
    r = ((dm * dm) & np.uint64(0xFFFFFFFF)).astype(np.uint32).astype(np.int32).astype(np.int64)
    return t, r


def _chain(x):
    """the reference's sum: channel outer, sample inner, one rounded add per term (np.cumsum adds in order)"""
    return float(np.cumsum(np.ascontiguousarray(x.T).reshape(-1))[-1])


def finish(mse, ref):
    """sqrt(mse / ref) * 100.0 as IEEE-754 has it, spelled out so that no platform's NaN or warning handling enters"""
    if mse != mse or ref != ref:
        return float("nan")
    if ref == 0.0:
        q = float("nan") if mse == 0.0 else float("inf")
    else:
        q = mse / ref
    if q != q or q < 0.0:
        return float("nan")
    return float(np.sqrt(np.float64(q))) * 100.0  # (sqrt(-0.0) = -0.0, sqrt(inf) = inf)


def prdn_parts(orig, dec, bps, nch, ns):
    """native blocks -> (prdn, mse, ref, path, info): the three doubles as the reference leaves them, path = 1 where a sum
    depends on the order of its adds, info = the exact integer sums and the means"""
    o, d = native_to_i32(orig, bps, nch, ns), native_to_i32(dec, bps, nch, ns)
    t, r = terms(o, d)
    t2 = t * t  # up to 2^62
    s2 = (int((t2 >> 32).sum()) << 32) + int((t2 & 0xFFFFFFFF).sum())
    sr, sa = int(r.sum()), int(np.abs(r).sum())
    need_m, need_r = s2 > EXACT_LIMIT, sa > EXACT_LIMIT
    tf = t.astype(np.float64)
    mse = _chain(tf * tf) if need_m else float(s2)
    ref = _chain(r.astype(np.float64)) if need_r else float(sr)
    info = dict(s2=s2, sr=sr, sa=sa, need_m=need_m, need_r=need_r, mean=average_32(o))
    return finish(mse, ref), mse, ref, int(need_m or need_r), info


def prdn(orig, dec, bps, nch, ns):
    return prdn_parts(orig, dec, bps, nch, ns)[0]


def _noisy(native, bps, nch, ns, seed, amp):
    """the block with a pseudo-random error in [-amp, amp) added to every sample (kept in the sample's width)"""
    x = native_to_i32(native, bps, nch, ns).astype(np.int64) + cases.hash_i32(nch * ns, seed, amp).astype(np.int64).reshape(ns, nch)
    return i32_to_native(x.astype(np.int32), bps)


def synthetic_cases():
    """name, bps, nch, ns, orig, dec (native bytes), group"""
    C = []

    def add(name, bps, nch, ns, orig, dec, group):
        orig = np.ascontiguousarray(np.asarray(orig, dtype=np.uint8).reshape(-1))
        dec = np.ascontiguousarray(np.asarray(dec, dtype=np.uint8).reshape(-1))
        assert orig.size == dec.size == bps * nch * ns, name
        C.append(dict(name=name, bps=bps, nch=nch, ns=ns, orig=orig, dec=dec, group=group))

    # every sample width, ns a power of two and not, odd channel counts
    for bps, nch, ns, amp, err in ((1, 7, 1001, 100, 5), (1, 16, 256, 128, 3), (2, 5, 1000, 1 << 14, 40), (2, 8, 2048, 1 << 15, 300),
                                   (3, 3, 777, 1 << 14, 200), (3, 4, 4096, 1 << 22, 1 << 12), (4, 4, 512, 1 << 15, 1 << 10),
                                   (4, 5, 333, 1 << 20, 100), (4, 12, 8192, 3000, 20)):
        x = cases._rand_native(nch, ns, bps, 1100 + bps * 10 + nch, amp, walk=amp <= 3000)
        add("rand%dx%d_i%d" % (nch, ns, 8 * bps), bps, nch, ns, x, _noisy(x, bps, nch, ns, 1200 + nch, err), "widths")
    # one channel, one sample: the mean is the sample, ref = 0
    add("one_sample_same_i32", 4, 1, 1, _i32([5]), _i32([5]), "zero_over_zero")
    add("one_sample_differs_i32", 4, 1, 1, _i32([5]), _i32([3]), "inf")
    add("one_sample_differs_i8", 1, 1, 1, np.array([250], dtype=np.uint8), np.array([3], dtype=np.uint8), "inf")
    # constant channels: ref = 0 whatever the decoded block holds
    const = np.repeat(np.array([[7, -3, 0]], dtype=np.int32), 64, axis=0)
    add("const3x64_same_i32", 4, 3, 64, _i32(const), _i32(const), "zero_over_zero")
    add("const3x64_differs_i32", 4, 3, 64, _i32(const), _i32(const + 1), "inf")
    # d == o on an ordinary block
    x = cases._rand_native(6, 500, 4, 1301, 1 << 16)
    add("same6x500_i32", 4, 6, 500, x, x, "same")
    # a negative channel sum at an ns that is not a power of two: (uint64)sum / ns is garbage, the squares wrap
    for k, (nch, ns, amp) in enumerate(((3, 100, 500), (2, 37, 1 << 20), (4, 1000, 1 << 28), (1, 7, 50), (5, 99, 30000))):
        neg = (-np.abs(cases.hash_i32(nch * ns, 1400 + k, amp)) - 3).astype(np.int32)
        add("negsum%dx%d_i32" % (nch, ns), 4, nch, ns, _i32(neg), _noisy(_i32(neg), 4, nch, ns, 1450 + k, 9), "negsum")
    x = _i32(-np.abs(cases.hash_i32(3 * 100, 1460, 500)) - 3)
    add("negsum3x100_same_i32", 4, 3, 100, x, x, "negsum")
    neg16 = (-np.abs(cases.hash_i32(4 * 300, 1470, 1 << 14)) - 1).astype(np.int16).view(np.uint8)
    add("negsum4x300_i16", 2, 4, 300, neg16, _noisy(neg16, 2, 4, 300, 1471, 4), "negsum")
    # a difference that wraps int32
    o = np.where(cases.hash_i32(2 * 64, 1500, 2) >= 0, (1 << 31) - 1 - 5, -(1 << 31) + 7).astype(np.int32).reshape(64, 2)
    add("diff_wraps2x64_i32", 4, 2, 64, _i32(o), _i32(-o), "wrap")
    full = cases._rand_native(3, 200, 4, 1501, (1 << 31) - 1)
    add("full_scale3x200_i32", 4, 3, 200, full, cases._rand_native(3, 200, 4, 1502, (1 << 31) - 1), "wrap")
    # sum t^2 > 2^53 with a finite answer: |o| <= 40000 (the squares of o - mean stay below 2^31), errors up to 2^28
    for k, (nch, ns) in enumerate(((1, 65536), (2, 65536), (3, 50000))):
        x = _i32(cases.hash_i32(nch * ns, 1600 + k, 40000))
        add("big_error%dx%d_i32" % (nch, ns), 4, nch, ns, x, _noisy(x, 4, nch, ns, 1650 + k, 1 << 28), "seq_mse")
    return C


# sum |r| > 2^53 needs more than 2^22 samples (|r| <= 2^31): no input of committed size reaches it, this generated one does
REF_SEQ = dict(name="ref_chain5x3400000_i32", bps=4, nch=5, ns=3400000, group="seq_ref")


def ref_seq_case():
    c = dict(REF_SEQ)
    c["orig"] = cases._rand_native(c["nch"], c["ns"], 4, 1700, 1 << 30)
    c["dec"] = _noisy(c["orig"], 4, c["nch"], c["ns"], 1701, 1 << 8)
    return c


# The sequential chain at the sample widths below int32: the smallest blocks whose sum t^2 leaves 2^53 (path 1, need_m, a finite
# PRDN).  int24: one sample past a chunk of 1024 (a second chunk of one sample), and two channels of three chunks, where the channel
# changes between chunks.  int16: t^2 < 2^32, so no block below 2^21 samples can be flagged; full-scale samples against their
# complements reach 2^53 at 2300000.  int8 cannot be flagged at all (t^2 <= 2^16 would need 2^37 samples), so it has no case.
SEQ_WIDTH_CASES = [dict(name="seq1x1025_i24", bps=3, nch=1, ns=1025), dict(name="seq2x2049_i24", bps=3, nch=2, ns=2049),
                   dict(name="seq1x2300000_i16", bps=2, nch=1, ns=2300000)]
_seq_width = {}


def seq_width_case(name):
    """the case of SEQ_WIDTH_CASES with its two blocks; int24 ones with `calm`, an unflagged pair (orig, dec) of the same shape"""
    if name not in _seq_width:
        c = dict(next(c for c in SEQ_WIDTH_CASES if c["name"] == name))
        bps, nch, ns = c["bps"], c["nch"], c["ns"]
        if bps == 3:
            c["orig"] = cases._rand_native(nch, ns, 3, 2103, 1 << 22)
            c["dec"] = _noisy(c["orig"], 3, nch, ns, 2153, 1 << 23)
            calm = cases._rand_native(nch, ns, 3, 2104, 1 << 22)
            c["calm"] = (calm, _noisy(calm, 3, nch, ns, 2154, 200))
        else:
            o = np.where(cases.hash_i32(ns, 2200, 2) >= 0, 32767, -32768).astype(np.int16)
            c["orig"], c["dec"] = o.view(np.uint8), (-1 - o).view(np.uint8)
        _seq_width[name] = c
    return _seq_width[name]


def lossy_fixtures():
    """every dct and hadamard fixture of tests/cases.py"""
    return [c for c in cases.packer_cases() if c["kind"] in ("dct", "hadamard")]


def lossy_case(c, decoded):
    return dict(name=c["name"], bps=c["bps"], nch=c["nch"], ns=c["ns"], orig=c["data"], dec=np.frombuffer(decoded, dtype=np.uint8), group="lossy")


def oracle_decoded(orc, c):
    pk = orc.packer(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"])
    dec, used, rc = pk.decompress(pk.compress(c["data"]))
    pk.close()
    assert rc == 0
    return dec


# the large batches of the GPU test (the bench's synthetic blocks)
BIG_BATCHES = [dict(name="synth64x(64x65536)_i32", nblocks=64, bps=4, nch=64, ns=65536), dict(name="synth1024x(12x8192)_i32", nblocks=1024, bps=4, nch=12, ns=8192)]
