"""The planar form of the rolling-window median (rspt_hip_median_filter_planar_batch_dev / _stream_dev): inputs and answers.

A planar buffer is the converters' int32 matrix [nblocks][nch][ns]: the whole int32 is the sample and the median is stored whole.
The answers are median_cases.median_i32 per row for a stateless call and median_stream_cases.median_stream_i32 on the blocks of all
calls concatenated for a stream case, transposed into the matrix: no second statement of the median.  Both restatements are pinned
to the compiled reference by median_record.json and median_stream_record.json.

The short kernel's geometry, as planar_win_model restates the host's rule (planar_win with kMedpMinLanes, host_stages.hip): a lane holds R = 32
consecutive outputs, a workgroup 256 lanes; a row of ns samples takes the smallest power of two of lanes that covers it, at least
8 and at most 256, so a chunk is lanes * 32 outputs, at most CHUNK = 8192, and 256 / lanes rows share a workgroup; rows of more
than one chunk are split into spans of whole chunks, each at least 4 (W - 1) samples, until there are about four workgroups per CU.

Every generated block has a different seed per channel, so that a store past a row's end or a window that reaches into the wrong
row shows.  tests/test_median_planar.py asserts what these lists cover.
"""
import functools

import numpy as np

import cases
import median_cases as mc
import median_stream_cases as msc
import planar_win_model
from iir_planar_cases import block, cut, native_of, planar_of, rows_of  # noqa: F401  (the layout helpers)
from median_cases import INT32_MAX, INT32_MIN, i32_to_native, native_to_i32  # noqa: F401
from planar_win_model import state_bytes  # noqa: F401  (state_bytes(W, nch))

R, THREADS, MIN_LANES = 32, 256, 8
CHUNK = R * THREADS
SHORT_MAX = 32
MAX_RANKS = 1 << 18
NCH = (1, 3, 64, 65)
OFFSETS = (0, 4, 8, 12)  # bytes between a 16-byte boundary and a buffer: word offsets 0, 1, 2, 3
BUCKET_WS = (2, 3, 4, 5, 8, 9, 16, 17, 31, 32)  # both edges of the register buckets 4, 8, 16, 32
MANY_ROWS_NS = 40  # 32 rows to a workgroup
ROW_NS = (1, 2, R - 1, R, R + 1, 2 * R + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5, MANY_ROWS_NS)
SPAN_WS = (3, 32)
REGIME_WS = (32, 33)
REGIME_NS = (1023, 1024, 1025, 4095, 4096, 4097, 8193)  # walk spans of 1024; one tile of 4096, one and two merge passes
STREAM_NS = (5, 12, 48, 100)
STREAM_CUTS = ((1, 4, 2), (5, 1, 3), (2, 3, 1))  # blocks per call; three calls per recording
FULL = (1 << 31) - 1


# ---- the geometry ----

def geom(num_cu, nblocks, nch, ns, W):
    """dict(lanes, rows_per_workgroup, chunk, span, nsplit) of a short-window call, as the host decides it"""
    return planar_win_model.geom(num_cu, nblocks, nch, ns, W, THREADS, R, MIN_LANES)


# ---- the answers ----

def stateless_expected(P, W):
    """every (block, channel) a fresh object: the window clamped to ns"""
    nb, nch, ns = P.shape
    y = mc.median_i32(P.transpose(2, 0, 1).reshape(ns, nb * nch), W)
    return np.ascontiguousarray(y.reshape(ns, nb, nch).transpose(1, 2, 0))


def stream_expected(P, W):
    """the blocks are one recording: (the answer [nblocks][nch][ns], the state's bytes behind it)"""
    nb, nch, ns = P.shape
    rows = rows_of(P)
    return planar_of(msc.median_stream_i32(rows, W), nb, nch, ns), state_image(rows, W)



def state_image(rows, W):
    """the documented state behind the recording rows [T][nch]: the native one at bps = 4 (median_stream_cases.state_after)"""
    rows = np.asarray(rows, dtype="<i4")
    return msc.state_after(rows.view(np.uint8).reshape(-1), 4, rows.shape[1], W)


def expected(c):
    """(answer, state bytes or None), computed once per case (read-only)"""
    return _expected(c["name"])


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = by_name()[name]
    out = stream_expected(c["planar"], c["W"]) if c["calls"] else (stateless_expected(c["planar"], c["W"]), None)
    out[0].setflags(write=False)
    return out


# ---- the cases ----

def _case(C, name, P, W, src_off, dst_off, calls=None, bps=4):
    """dst_off None: in place"""
    P.setflags(write=False)
    nb, nch, ns = P.shape
    C.append(dict(name=name, nch=nch, ns=ns, nblocks=nb, planar=P, W=W, src_off=src_off, dst_off=dst_off, calls=calls, bps=bps))


def _mode(do):
    return "in_place" if do is None else "dst%d" % do


@functools.lru_cache(maxsize=None)
def row_cases():
    """stateless row ends on the short path: every ns, two cases in place and two out of place, over the channel counts, the
    bucket edges and both buffers' offsets; every bucket edge in both modes on 16-byte aligned rows (the wide path) and off them;
    W = ns - 1, ns and above ns on both sides of the regime switch"""
    C = []
    for idx, ns in enumerate(ROW_NS):
        for j in range(4):
            i, t = 4 * idx + j, 2 * idx + j // 2
            nch = NCH[(idx + j) % 4] if ns < 1000 else (3, 1, 2, 3)[j]
            nb = (2, 3)[i % 2]
            W = BUCKET_WS[(i + idx) % len(BUCKET_WS)]
            so, do = OFFSETS[t % 4], OFFSETS[(t // 4) % 4]
            do = None if j % 2 == 1 else do
            _case(C, "row_ns%d_%dch_x%d_w%d_src%d_%s" % (ns, nch, nb, W, so, _mode(do)), block(nb, nch, ns, 2100 + i), W, so, do)
    for i, W in enumerate(BUCKET_WS):
        for j, (so, do) in enumerate(((0, None), (0, 0), (4, None), (8, 12))):
            ns = (300, 8192 + 64)[(i + j) % 2] if j < 2 else 301
            _case(C, "bucket_w%d_ns%d_src%d_%s" % (W, ns, so, _mode(do)), block(2, 3 if ns < 1000 else 1, ns, 2200 + 4 * i + j), W, so, do)
    for i, (ns, Ws) in enumerate(((20, (19, 20, 25)), (50, (49, 50, 60)))):
        for j, W in enumerate(Ws):
            do = None if j % 2 else 4
            _case(C, "window_ns%d_w%d_%s" % (ns, W, _mode(do)), block(2, 3, ns, 2300 + 3 * i + j), W, 4 * j, do)
    return C


@functools.lru_cache(maxsize=None)
def span_cases():
    """rows that the geometry splits, in place: 1 x (2 ch x 40000)"""
    C = []
    for W in SPAN_WS:
        for off in (0, 4):
            _case(C, "span_2ch_x1_ns40000_w%d_off%d" % (W, off), block(1, 2, 40000, 2400 + W + off), W, off, None)
    return C


@functools.lru_cache(maxsize=None)
def value_cases():
    """runs of INT32_MIN / INT32_MAX (the kernel's pads), pairs with a negative odd sum, a ternary signal; short and generic"""
    C = []
    nb, nch, ns = 2, 3, 200
    n = nb * nch * ns
    full = np.where(cases.hash_i32(n, 2501, 4) >= 0, INT32_MAX, INT32_MIN).astype(np.int32).reshape(nb, nch, ns)
    full[0, 0, :70], full[0, 1, :70], full[1, 2, 100:] = INT32_MIN, INT32_MAX, INT32_MIN
    neg = (-(np.abs(cases.hash_i32(n, 2502, 1 << 20).astype(np.int64)) * 2 + (np.arange(n) // 2) % 2 + 1)).astype(np.int32).reshape(nb, nch, ns)
    tern = (cases.hash_i32(n, 2503, 3) % 3 - 1).astype(np.int32).reshape(nb, nch, ns)
    for tag, P, Ws in (("full_scale", full, (2, 4, 31, 40)), ("negative_odd", neg, (2, 4, 34)), ("ternary", tern, (6, 32, 51))):
        for j, W in enumerate(Ws):
            _case(C, "%s_w%d" % (tag, W), P.copy(), W, 4 * (j % 4), None if j % 2 else 0)
            _case(C, "%s_w%d_stream" % (tag, W), P.copy(), W, 0, None if j % 2 == 0 else 8, calls=(1, 1))
    return C


def outside(bps, nb, nch, ns, seed):
    """full-scale int32 values, with 1 << 8 bps, its negative and the int32 limits at the rows' ends and inside them"""
    P = block(nb, nch, ns, seed, FULL)
    marks = (1 << (8 * bps), -(1 << (8 * bps)), FULL, -FULL - 1, (1 << (8 * bps)) + 1)
    for k, v in enumerate(marks):
        P[:, :, (k * 13 + 5) % ns] = v
    P[:, :, 0], P[:, :, ns - 1] = 1 << (8 * bps), -(1 << (8 * bps))
    return P


@functools.lru_cache(maxsize=None)
def width_cases():
    """handles of 1, 2 and 3 bytes per sample under values that need all 32 bits"""
    C = []
    for bps in (1, 2, 3):
        nch, ns = (3, 65, 1)[bps - 1], (130, 70, 200)[bps - 1]
        tag = "width_i%d_%dch_ns%d" % (8 * bps, nch, ns)
        _case(C, tag + "_w5", outside(bps, 2, nch, ns, 2600 + bps), 5, 4 * bps, None, bps=bps)
        _case(C, tag + "_w1_out_of_place", outside(bps, 2, nch, ns, 2610 + bps), 1, 0, 4, bps=bps)
        _case(C, tag + "_w17_stream", outside(bps, 3, nch, ns, 2620 + bps), 17, 8, None, calls=(1, 2), bps=bps)
        _case(C, tag + "_w40", outside(bps, 2, nch, ns, 2630 + bps), 40, 0, 8, bps=bps)
    return C


@functools.lru_cache(maxsize=None)
def regime_cases():
    """both sides of the regime switch on rows around the generic path's walk span, tile and merge passes"""
    C = []
    for i, ns in enumerate(REGIME_NS):
        for j, W in enumerate(REGIME_WS):
            do = None if (i + j) % 2 else 4 * (i % 4)
            _case(C, "regime_ns%d_w%d_%s" % (ns, W, _mode(do)), block(2, 2, ns, 2700 + 2 * i + j), W, 4 * ((i + j) % 4), do)
    return C


def stream_windows(ns):
    """W - 1 below ns; between 2 ns and 3 ns, reaching three blocks back; above a whole call (the longest has five blocks)"""
    return (ns // 2 + 2, 2 * ns + ns // 2 + 1, 5 * ns + ns // 2 + 1)


GENERIC_STREAM = "stream_generic_2ch_30000x3_w101_in_place"
SPLIT_STREAM = "stream_split_2ch_40000x2_w5_out_of_place"


@functools.lru_cache(maxsize=None)
def stream_cases():
    C, i = [], 0
    for ns in STREAM_NS:
        for ci, cut_ in enumerate(STREAM_CUTS):
            for ki, W in enumerate(stream_windows(ns)):
                nch = NCH[i % 4] if W < 3 * ns else (1, 3, 5, 2)[i % 4]
                so, do = OFFSETS[i % 4], OFFSETS[(i // 4 + 1) % 4]
                do = None if (ci + ki) % 2 == 0 else do
                _case(C, "stream_ns%d_%s_%dch_w%d_%s" % (ns, "".join(map(str, cut_)), nch, W, _mode(do)), block(sum(cut_), nch, ns, 2800 + i), W, so, do,
                      calls=cut_)
                i += 1
    # a generic carried call of two segments (65536 - 100 new rows each): 90000 rows in one call, then a started state
    _case(C, GENERIC_STREAM, block(4, 2, 30000, 2890), 101, 0, None, calls=(3, 1))
    # a carried short-window call on rows that the geometry splits, out of place: span 0 of every row has a staged front, the
    # other spans read d_src (npiece = 1, nsplit > 1); and the same in place (npiece = nsplit)
    _case(C, SPLIT_STREAM, block(2, 2, 40000, 2893), 5, 0, 4, calls=(1, 1))
    _case(C, "stream_split_2ch_40000x2_w5_in_place", block(2, 2, 40000, 2894), 5, 4, None, calls=(1, 1))
    _case(C, "stream_w1_copy", block(3, 3, 50, 2891), 1, 4, 8, calls=(2, 1))
    _case(C, "stream_w1_in_place", block(3, 3, 50, 2892), 1, 4, None, calls=(2, 1))
    return C


def all_cases():
    return row_cases() + span_cases() + value_cases() + width_cases() + regime_cases() + stream_cases()


@functools.lru_cache(maxsize=None)
def by_name():
    C = all_cases()
    assert len({c["name"] for c in C}) == len(C)
    return {c["name"]: c for c in C}


SWEEP_WS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 25, 31, 32, 33, 34, 50, 99, 200)


def sweep_cases(n=300, seed=20261019):
    """random small cases: shape, offsets, W on both sides of 32, in or out of place, stateless or a random cut into calls"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nb, nch, ns, W = int(rng.integers(1, 6)), int(rng.integers(1, 10)), int(rng.integers(1, 301)), int(rng.choice(SWEEP_WS))
        so, do = int(rng.choice(OFFSETS)), (None if rng.integers(0, 2) else int(rng.choice(OFFSETS)))
        calls = None
        if rng.integers(0, 2):
            calls, left = [], nb
            while left:
                calls.append(int(rng.integers(1, left + 1)))
                left -= calls[-1]
        amp = int(rng.choice([FULL, 1 << 20, 100, 2]))
        out.append(dict(name="sweep%d" % i, nch=nch, ns=ns, nblocks=nb, planar=block(nb, nch, ns, 9500 + i, amp), W=W, src_off=so, dst_off=do,
                        calls=tuple(calls) if calls else None, bps=4))
    return out


# ---- the records' cases as the planar entries see them ----

def record_planar(c, nblocks=1):
    """native_to_i32 of a record case's bytes, as [nblocks][nch][ns]"""
    return planar_of(native_to_i32(c["data"], c["bps"], c["nch"], c["ns"] * nblocks), nblocks, c["nch"], c["ns"])


@functools.lru_cache(maxsize=None)
def record_expected(name):
    """the planar answer of a case of median_cases(), computed once (read-only)"""
    c = next(c for c in mc.median_cases() if c["name"] == name)
    y = stateless_expected(record_planar(c), c["W"])
    y.setflags(write=False)
    return y
