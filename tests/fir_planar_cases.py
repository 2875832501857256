"""The planar form of the FIR pre-filter (rspt_hip_fir_prefilter_planar_batch_dev / _stream_dev): inputs and answers.

A planar buffer is the converters' int32 matrix [nblocks][nch][ns]: the whole int32 is the sample, the result is trunc_i32 of the
double, stored whole.  The answers are fir_cases.fir_i32 + trunc_i32 per channel on the int32 run -- a block's row for a stateless
call, the blocks of all calls concatenated for a stream case -- transposed into the matrix: no second statement of the filter.

The kernel's geometry, as planar_win_model restates the host's rule (planar_win, host_stages.hip): a lane holds R = 16 consecutive outputs, a
workgroup 256 lanes; a row of ns samples takes the smallest power of two of lanes that covers it (at most 256), so a chunk is
lanes * 16 outputs, at most CHUNK = 4096, and 256 / lanes rows share a workgroup; rows of more than one chunk are split into
spans of whole chunks, each at least 4 (K - 1) samples, until there are about four workgroups per CU.

Every generated block has a different seed per channel, so that a store past a row's end or a load clamped by address instead of
by index shows in the neighbouring row.  tests/test_fir_planar.py asserts what these lists cover.
"""
import functools

import numpy as np

import fir_cases as fc
import planar_win_model
from fir_cases import i32_to_native, native_to_i32, trunc_i32  # noqa: F401
from iir_planar_cases import block, cut, native_of, planar_of, rows_of  # noqa: F401  (the layout helpers)
from planar_win_model import state_bytes  # noqa: F401  (state_bytes(K, nch))

R, THREADS = 16, 256
CHUNK = R * THREADS
NCH = (1, 3, 64, 65)
OFFSETS = (0, 4, 8, 12)  # bytes between a 16-byte boundary and a buffer
ROW_KS = (1, 2, 16, 17, 33, 255)
SHORT_NS = (1, 2, 15, 16, 17, 63, 64, 65)  # several rows to a workgroup
LONG_NS = 2 * CHUNK + 64  # a first, a middle and a short last chunk
ROW_NS = SHORT_NS + (100, 255, 257, 700, 2000, CHUNK - 1, CHUNK, CHUNK + 1, LONG_NS)
STREAM_NS = (17, 48, 64, 100)
STREAM_CUTS = ((1, 4, 2), (5, 1, 3), (2, 3, 1))  # blocks per call; three calls per recording
FULL = (1 << 31) - 1


# ---- the geometry ----

def geom(num_cu, nblocks, nch, ns, K):
    """dict(lanes, rows_per_workgroup, chunk, span, nsplit) of a call, as the host decides it"""
    return planar_win_model.geom(num_cu, nblocks, nch, ns, K, THREADS, R)


# ---- the answers ----

def fir_rows(rows, kernel):
    """[T][lanes] int32 -> the uncut int32 answer of one run per lane"""
    return trunc_i32(fc.fir_i32(rows, kernel))


def stateless_expected(P, kernel):
    """every (block, channel) a run of its own"""
    nb, nch, ns = P.shape
    y = fir_rows(P.transpose(2, 0, 1).reshape(ns, nb * nch), kernel)
    return np.ascontiguousarray(y.reshape(ns, nb, nch).transpose(1, 2, 0))


def stream_expected(P, kernel):
    """the blocks are one recording: (the answer [nblocks][nch][ns], the state's rows behind it [K - 1][nch])"""
    nb, nch, ns = P.shape
    rows = rows_of(P)
    K = len(kernel)
    tail = np.concatenate([np.repeat(rows[:1], K - 1, axis=0), rows], axis=0)[rows.shape[0]:]
    return planar_of(fir_rows(rows, kernel), nb, nch, ns), np.ascontiguousarray(tail, dtype=np.int32)



def state_image(K, nch, tail):
    """the documented state: uint64 started = 1, then the last K - 1 rows, oldest first, each nch int32, zero padding"""
    img = np.zeros(state_bytes(K, nch), dtype=np.uint8)
    img[:8] = np.array([1], dtype="<u8").view(np.uint8)
    img[8 : 8 + (K - 1) * nch * 4] = np.ascontiguousarray(tail, dtype="<i4").view(np.uint8).reshape(-1)
    return img


def expected(c):
    """(answer, state rows or None), computed once per case (read-only)"""
    return _expected(c["name"])


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = by_name()[name]
    out = stream_expected(c["planar"], c["kernel"]) if c["calls"] else (stateless_expected(c["planar"], c["kernel"]), None)
    out[0].setflags(write=False)
    return out


# ---- the cases ----

def kernel(K, seed, exp=None):
    """K taps in {-8/2^exp .. 7/2^exp} (fir_cases._rand_kernel); the default exp keeps the sums of full 20-bit samples in int32"""
    return fc._rand_kernel(K, seed, max(4, int(np.ceil(np.log2(K))) + 2) if exp is None else exp)


def _case(C, name, P, K, seed, src_off, dst_off, calls=None, bps=4, k=None):
    """dst_off None: in place"""
    P.setflags(write=False)
    nb, nch, ns = P.shape
    C.append(dict(name=name, nch=nch, ns=ns, nblocks=nb, planar=P, kernel=kernel(K, seed) if k is None else np.asarray(k, dtype=np.float64), K=K,
                  src_off=src_off, dst_off=dst_off, calls=calls, bps=bps))


@functools.lru_cache(maxsize=None)
def row_cases():
    """stateless row ends: every ns, two cases in place and two out of place, over the channel counts, the taps and both buffers'
    offsets; then 16-byte aligned buffers on rows of a chunk and more (the wide path's clamped and unclamped chunks), and a window
    longer than the row"""
    C = []
    for idx, ns in enumerate(ROW_NS):
        for j in range(4):
            i, t = 4 * idx + j, 2 * idx + j // 2
            nch = NCH[(idx + j) % 4] if ns < 700 else (3, 1, 2, 3)[j]
            nb = (2, 3)[i % 2]
            K = ROW_KS[(i + idx) % 6]
            so, do = OFFSETS[t % 4], OFFSETS[(t // 4) % 4]
            in_place = j % 2 == 1
            _case(C, "row_ns%d_%dch_x%d_k%d_src%d_%s" % (ns, nch, nb, K, so, "in_place" if in_place else "dst%d" % do), block(nb, nch, ns, 1100 + i), K, 1100 + i,
                  so, None if in_place else do)
    for j, (ns, K, do) in enumerate(((CHUNK, 33, None), (CHUNK, 255, 0), (LONG_NS, 255, None), (LONG_NS, 17, 0))):
        _case(C, "row_wide_ns%d_2ch_x2_k%d_%s" % (ns, K, "in_place" if do is None else "dst0"), block(2, 2, ns, 1180 + j), K, 1180 + j, 0, do)
    # (the fir record's K = 4097 on 700 samples)
    for j, do in enumerate((None, 8)):
        _case(C, "row_ns700_3ch_x2_k4097_src%d_%s" % (4 * j, "in_place" if do is None else "dst8"), block(2, 3, 700, 1190 + j), 4097, 1190 + j, 4 * j, do)
    return C


SPAN_KS = (101, 1001, 2049)


@functools.lru_cache(maxsize=None)
def span_cases():
    """rows that the geometry splits, in place: 1 x (2 ch x 40000).  K = 101 and K = 1001: as many spans as whole chunks allow
    (4 (K - 1) <= CHUNK); K = 2049: the span rule 4 (K - 1) = 8192 limits the split"""
    C = []
    for K in SPAN_KS:
        for off in (0, 4):
            _case(C, "span_2ch_x1_ns40000_k%d_off%d" % (K, off), block(1, 2, 40000, 1200 + K + off), K, 1200 + K, off, None)
    return C


def stream_taps(ns):
    """K - 1 below ns; above ns, reaching three blocks back; above a whole call (the longest has five blocks)"""
    return (ns // 2 + 1, 2 * ns + 7, 5 * ns + 4)


@functools.lru_cache(maxsize=None)
def stream_cases():
    C, i = [], 0
    for ns in STREAM_NS:
        for ci, cut_ in enumerate(STREAM_CUTS):
            for ki, K in enumerate(stream_taps(ns)):
                nch = NCH[i % 4] if K < 3 * ns else (1, 3, 5, 2)[i % 4]
                nb = sum(cut_)
                so, do = OFFSETS[i % 4], OFFSETS[(i // 4 + 1) % 4]
                in_place = (ci + ki) % 2 == 0
                _case(C, "stream_ns%d_%s_%dch_k%d_%s" % (ns, "".join(map(str, cut_)), nch, K, "in_place" if in_place else "out_of_place"),
                      block(nb, nch, ns, 1300 + i), K, 1300 + i, so, None if in_place else do, calls=cut_)
                i += 1
    return C


def _outside(bps, nb, nch, ns, seed):
    """full-scale int32 values, with 1 << 8 bps, its negative and the int32 limits at the rows' ends and inside them"""
    P = block(nb, nch, ns, seed, FULL)
    marks = (1 << (8 * bps), -(1 << (8 * bps)), FULL, -FULL - 1, (1 << (8 * bps)) + 1)
    for k, v in enumerate(marks):
        P[:, :, (k * 13 + 5) % ns] = v
    P[:, :, 0], P[:, :, ns - 1] = 1 << (8 * bps), -(1 << (8 * bps))
    return P


@functools.lru_cache(maxsize=None)
def width_cases():
    """handles of 1, 2 and 3 bytes per sample under values that need all 32 bits; kernels whose sums stay inside int32"""
    C = []
    for bps in (1, 2, 3):
        nch, ns = (3, 65, 1)[bps - 1], (130, 70, 200)[bps - 1]
        tag = "width_i%d_%dch_ns%d" % (8 * bps, nch, ns)
        _case(C, tag + "_k3", _outside(bps, 2, nch, ns, 1400 + bps), 3, 0, 4 * bps, None, bps=bps, k=[0.25, 0.5, 0.125])
        _case(C, tag + "_k1_out_of_place", _outside(bps, 2, nch, ns, 1410 + bps), 1, 0, 0, 4, bps=bps, k=[0.75])
        _case(C, tag + "_k17_stream", _outside(bps, 3, nch, ns, 1420 + bps), 17, 0, 8, None, calls=(1, 2), bps=bps, k=np.full(17, 1.0 / 32))
    return C


@functools.lru_cache(maxsize=None)
def overflow_cases():
    """fir_cases' inf/NaN kernel and its full-scale gain case, on the matrix"""
    by = {c["name"]: c for c in fc.fir_cases()}
    C = []
    for name in ("rand4x2000_i32_inf_nan", "full_scale6x3000_i32_gain_overflow"):
        c = by[name]
        P = planar_of(native_to_i32(c["data"], c["bps"], c["nch"], c["ns"]), 1, c["nch"], c["ns"])
        _case(C, "overflow_" + name, np.ascontiguousarray(np.concatenate([P, P[:, ::-1]], axis=0)), len(c["kernel"]), 0, 4, None, k=c["kernel"])
    return C


def all_cases():
    return row_cases() + span_cases() + stream_cases() + width_cases() + overflow_cases()


@functools.lru_cache(maxsize=None)
def by_name():
    C = all_cases()
    assert len({c["name"] for c in C}) == len(C)
    return {c["name"]: c for c in C}


def sweep_cases(n=200, seed=20261019):
    """random small cases: (i, nch, ns, nblocks, kernel, src_off, dst_off or None, calls or None)"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        nb, nch, ns, K = int(rng.integers(1, 6)), int(rng.integers(1, 10)), int(rng.integers(1, 301)), int(rng.integers(1, 201))
        k = rng.standard_normal(K) * float(rng.choice([1e-3, 1.0 / K, 1.0, 3.0]))
        so, do = int(rng.choice(OFFSETS)), (None if rng.integers(0, 2) else int(rng.choice(OFFSETS)))
        calls = None
        if rng.integers(0, 2):
            calls, left = [], nb
            while left:
                calls.append(int(rng.integers(1, left + 1)))
                left -= calls[-1]
        amp = int(rng.choice([FULL, 1 << 20, 100]))
        out.append(dict(name="sweep%d" % i, nch=nch, ns=ns, nblocks=nb, planar=block(nb, nch, ns, 9000 + i, amp), kernel=k, K=K, src_off=so, dst_off=do,
                        calls=tuple(calls) if calls else None, bps=4))
    return out


# ---- the records' cases as the planar entries see them ----

def record_planar(c, nblocks=1):
    """native_to_i32 of a record case's bytes, as [nblocks][nch][ns]"""
    return planar_of(native_to_i32(c["data"], c["bps"], c["nch"], c["ns"] * nblocks), nblocks, c["nch"], c["ns"])

