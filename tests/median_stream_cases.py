"""The rolling-median stage with a carried state: its test inputs and a numpy restatement.

A case is ONE recording of nblocks * ns rows cut into nblocks blocks of the handle's shape (bps, nch, ns).  The reference
user keeps one rolling_window_median<double>(W) per channel and calls insert() on every sample of every block in order, so
the answer does not depend on where the recording is cut: with X the channel's recording and T an index in it,
    lo = max(0, T - W + 1),  m = T - lo + 1,  s = sorted(X[lo .. T])
    y[T] = m odd ? s[m / 2] : (int32_t)(((int64_t)s[m / 2 - 1] + s[m / 2]) / 2)      (C division: toward zero)
with W NOT clamped to ns.  The cases feed tests/golden/make_median_stream_record.py, which records the compiled reference's
answers in tests/golden/median_stream_record.json; the inputs are integer arithmetic or the shipped recordings.
"""
import bisect

import numpy as np

import cases
import casetools
import median_cases as mc
from casetools import _i32, _take
from median_cases import crc, i32_to_native, native_to_i32  # noqa: F401
from rspt_amd import synth

MAX_CARRY = 1 << 17  # the longest carried window (W - 1) above the short regime
SHORT_MAX = 32


def stream_cases():
    """name, bps, nch, ns, nblocks, W, data (native bytes of nblocks * ns rows)"""
    ecg = np.frombuffer(synth.ecg_12ch_i32(), dtype=np.uint8)  # 34199 rows -> 16 blocks of 12 x 2048
    ds = np.frombuffer(synth.data_stream_3ch_i24(), dtype=np.uint8)  # 20000 rows -> 20 blocks of 3 x 1000
    C = []

    def add(name, bps, nch, ns, nblocks, W, data):
        C.append(dict(name=name, bps=bps, nch=nch, ns=ns, nblocks=nblocks, W=W, data=_take(data, bps, nch, ns * nblocks)))

    # rspt_test.cpp test_8_rolling_window_median: its 20 inputs as 5 blocks of 4
    for W in (5, 6, 7):
        add("ref20_4x5_w%d" % W, 4, 1, 4, 5, W, _i32(mc.REF20))
    # both edges of every register bucket of k_med_short and the first generic window, over every sample width; ns below 64 and
    # above 64 but no multiple of it; nch = 1
    shapes = [(1, 1, 40, 8), (2, 5, 100, 6), (3, 3, 70, 5), (4, 7, 232, 4)]
    data = [cases._rand_native(nch, ns * nb, bps, 5000 + bps, 1 << (8 * bps - 2), walk=bps == 4) for bps, nch, ns, nb in shapes]
    for i, W in enumerate((1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33)):
        for k in (i % 4, (i + 1) % 4):
            bps, nch, ns, nb = shapes[k]
            add("rand%dx%dx%d_i%d_w%d" % (nch, ns, nb, 8 * bps, W), bps, nch, ns, nb, W, data[k])
    s5 = synth.synth_native(5, 3000, 3, bps=2, ecg=True).numpy()
    for W in (100, 101):
        add("synth5x300x10_i16_w%d" % W, 2, 5, 300, 10, W, s5)
    add("ecg12x2048x16_i32_w31", 4, 12, 2048, 16, 31, ecg)
    add("ecg12x2048x16_i32_w1500", 4, 12, 2048, 16, 1500, ecg)  # the window of the reference's own test
    add("ds3x1000x20_i24_w101", 3, 3, 1000, 20, 101, ds)
    add("ds3x1000x20_i24_w1000", 3, 3, 1000, 20, 1000, ds)  # W - 1 = ns - 1
    add("rand3x700x4_i24_w4097", 3, 3, 700, 4, 4097, cases._rand_native(3, 2800, 3, 5010, 1 << 22))  # W - 1 > ns
    add("rand2x40x5_i32_w65536", 4, 2, 40, 5, 65536, cases._rand_native(2, 200, 4, 5011, 1 << 22))  # W - 1 > the recording
    # the generic path past 2^18 rows per channel: a segment edge falls inside the recording
    add("walk1x65536x5_i32_w101", 4, 1, 65536, 5, 101, cases._rand_native(1, 327680, 4, 5012, 1 << 24, walk=True))
    add("rand1x60000x5_i16_w131073", 2, 1, 60000, 5, MAX_CARRY + 1, cases._rand_native(1, 300000, 2, 5013, 1 << 14))  # the limit
    # ns above 2^18 with a generic window (the stateless entry refuses it); int8: heavy ties
    add("rand1x300000x2_i8_w33", 1, 1, 300000, 2, 33, cases._rand_native(1, 600000, 1, 5014, 100))
    # ties: the reference's iterator logic branches on equal values
    for W in (7, 40):
        add("constant3x50x6_i16_w%d" % W, 2, 3, 50, 6, W, np.full(3 * 300, -1234, dtype=np.int16).view(np.uint8))
    alt = np.where((np.arange(2 * 1001) // 2) % 2 == 0, 17, -5).astype(np.int8).view(np.uint8)  # per channel 17, -5, 17, ...
    for W in (6, 51):
        add("alternating2x143x7_i8_w%d" % W, 1, 2, 143, 7, W, alt)
    # pairs of negative values with an odd sum: the mean truncates toward zero
    neg = -(np.abs(cases.hash_i32(2 * 400, 5015, 1 << 20).astype(np.int64)) * 2 + (np.arange(800) // 2) % 2 + 1).astype(np.int32)
    for W in (2, 4, 34):
        add("negative2x100x4_i32_w%d" % W, 4, 2, 100, 4, W, _i32(neg))
    return C


# ---- the restatement ----

def _by_bisect(x, W):
    """any W: a sorted list per channel, one insertion and at most one deletion per sample"""
    rows, nch = x.shape
    y = np.empty((rows, nch), dtype=np.int32)
    for c in range(nch):
        col = x[:, c].tolist()
        s, out = [], y[:, c]
        for t, v in enumerate(col):
            bisect.insort(s, v)
            if t >= W:
                del s[bisect.bisect_left(s, col[t - W])]
            m = len(s)
            if m & 1:
                out[t] = s[m // 2]
            else:
                h = s[m // 2 - 1] + s[m // 2]
                out[t] = -((-h) // 2) if h < 0 else h // 2
    return y


def median_stream_i32(x, W):
    """[rows][nch] int32, the whole recording -> y[T][c] = the (int32_t) median of x[max(0, T - W + 1) .. T][c].  Over the whole
    recording the formula is the stateless one on a single block of all its rows (a window of the recording's length or more is
    the expanding median), so windows up to 4097 go through median_cases.median_i32; longer ones through a sorted list."""
    x = np.asarray(x, dtype=np.int32)
    W = int(W)
    if W <= 4097 or W >= x.shape[0]:
        return mc.median_i32(x, W)
    return _by_bisect(x, W)


def filtered(c):
    """the filtered recording in the native sample width (bytes), as the stream entry leaves it"""
    rows = c["ns"] * c["nblocks"]
    return i32_to_native(median_stream_i32(native_to_i32(c["data"], c["bps"], c["nch"], rows), c["W"]), c["bps"])


def state_after(data, bps, nch, W):
    """the state's bytes after the recording `data` (native bytes of whole rows): uint64 fill = min(rows, W - 1), then W - 1 rows
    of which the last `fill` are the recording's last rows and the others zero, padded to a multiple of 8 bytes"""
    stride = bps * nch
    d = np.asarray(data, dtype=np.uint8).reshape(-1, stride)
    fill = min(d.shape[0], W - 1)
    n = (W - 1) * stride
    out = np.zeros(8 + (n + 7) // 8 * 8, dtype=np.uint8)
    out[:8] = np.frombuffer(np.uint64(fill).tobytes(), dtype=np.uint8)
    if fill:
        out[8 + n - fill * stride : 8 + n] = d[d.shape[0] - fill :].reshape(-1)
    return out


def splits(nblocks):
    """the drivings of a recording: all blocks in one call, one block per call, an uneven cut (1, 3, rest)"""
    return casetools.splits(nblocks, (1, 3, nblocks))


def random_case(seed):
    """a small seeded recording: shape, width, W on both sides of 32, the cut, in place or not"""
    r = np.random.RandomState(7000 + seed)
    bps = int(r.randint(1, 5))
    nch = int(r.choice([1, 2, 3, 5, 8, 17]))
    ns = int(r.choice([1, 7, 40, 64, 100, 333]))
    nblocks = int(r.randint(1, 9))
    W = int(r.choice([2, 3, 4, 5, 7, 8, 12, 16, 17, 25, 32, 33, 34, 50, 64, 99, 200, 700, 3000]))
    amp = int(r.choice([2, 50, 1 << (8 * bps - 2)]))
    amp = min(amp, 1 << (8 * bps - 2))
    data = cases._rand_native(nch, ns * nblocks, bps, 7100 + seed, amp, walk=bool(seed & 1) and bps > 1)
    cut, left = [], nblocks
    while left:
        k = int(r.randint(1, left + 1))
        cut.append(k)
        left -= k
    return dict(name="seed%d" % seed, bps=bps, nch=nch, ns=ns, nblocks=nblocks, W=W, data=_take(data, bps, nch, ns * nblocks), cut=cut,
                out_of_place=bool(r.randint(0, 2)))


# in place, W > 32, more than 2^25 samples in one call: the generic path takes the call in more than one piece
PIECES = dict(bps=1, nch=8, ns=65536, nblocks=80, W=101, seed=5020)


def pieces_data():
    P = PIECES
    return cases._rand_native(P["nch"], P["ns"] * P["nblocks"], P["bps"], P["seed"], 100)
