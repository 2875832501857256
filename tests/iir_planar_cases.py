"""The planar forms of the IIR pre-filter and the IIR cascade (rspt_hip_iir_*_planar_*_dev): test inputs and answers.

A planar buffer is the converters' int32 matrix [nblocks][nch][ns], filtered in place: the whole int32 is the sample, the result
is trunc_i32 of the double, stored whole.  The answers come from tests/iir_model.py through iir_cases.iir_double and
iir_cascade_cases.chain_double on the whole values (a native block of int32 samples is the same numbers interleaved), transposed
into the matrix: no second statement of the filter.

    sweep_planar / sweep_expected   a case of tests/iir_sweep_cases.py as the planar entries see it: native_to_i32 of its bytes,
                                    and the uncut answer; cut to the case's bps it is the compiled reference's record
    row_cases       stateless row ends: ns around the chunk and the 16-sample part x the base's offset from a 16-byte boundary
    stream_cases    carried runs whose block boundaries fall inside a producer part, on a part boundary, on a chunk boundary
    route_cases     the shapes that take the plain kernels
    width_cases     values outside the handle's sample width

Every generated block has a different seed per channel, so that a store past a row's end or a load clamped by address instead
of by index shows in the neighbouring row.  tests/test_iir_planar.py asserts what these lists cover.
"""
import functools

import numpy as np

import cases
import iir_cascade_cases as cc
import iir_cases as ic
import iir_sweep_cases as sw
from fir_cases import i32_to_native, native_to_i32, trunc_i32  # noqa: F401

NCH = (1, 3, 64, 65)
ROW_NS = (64, 65, 66, 67, 79, 80, 127, 129, 200)
OFFSETS = (0, 4, 8, 12)  # bytes between a 16-byte boundary and the buffer
STREAM_NS = (17, 48, 64, 80, 100, 128)
STREAM_CUTS = ((1, 4, 2), (5, 1, 3), (2, 3, 1))  # blocks per call; three calls per recording
SWEEP_LEGS = ("single", "single_stream", "cascade", "cascade_stream")
SINGLE_CHUNK, CASCADE_CHUNK, PART = ic.CHUNK_PIPE, cc.CHUNK, 16
FULL = (1 << 31) - 1
# the filters of the single stage, one per order: the harness's band-pass for order 4 (5 coefficients)
COEFS = {2: ic.STABLE[2], 3: cases.IIR_LOWPASS, 4: ic.STABLE[4], 5: cases.IIR_BANDPASS}


# ---- the layouts ----

def rows_of(P):
    """[nblocks][nch][ns] -> [nblocks * ns][nch]: the recording's rows (what a native block interleaves)"""
    nb, nch, ns = P.shape
    return np.ascontiguousarray(P.transpose(0, 2, 1)).reshape(nb * ns, nch)


def planar_of(rows, nblocks, nch, ns):
    """[nblocks * ns][nch] (or [nblocks][ns][nch]) -> [nblocks][nch][ns]"""
    return np.ascontiguousarray(np.asarray(rows).reshape(nblocks, ns, nch).transpose(0, 2, 1))


def native_of(P):
    """the int32 native blocks (bytes) that hold P's samples"""
    return rows_of(P).astype("<i4").view(np.uint8).reshape(-1)


def block(nblocks, nch, ns, seed, amp=1 << 20):
    """[nblocks][nch][ns] int32 within +-amp, every channel from a seed of its own"""
    return np.ascontiguousarray(np.stack([cases.hash_i32(nblocks * ns, 7919 * seed + ch, amp).reshape(nblocks, ns) for ch in range(nch)], axis=1))


def sections_of(c):
    return c["sections"] if "sections" in c else [(c["n"], c["d"], c["init"], False)]


# ---- the answers ----

def stateless_expected(c):
    """the uncut answer [nblocks][nch][ns] of a stateless case (kind 'single' or 'cascade') on c['planar']"""
    P = c["planar"]
    nb, nch, ns = P.shape
    if c["kind"] == "single":
        y = ic.iir_double(native_of(P), 4, nch, ns, c["n"], c["d"], c["init"], c["shared"], nb)
    else:  # every (block, channel) a fresh chain: the blocks as further lanes
        x = P.transpose(2, 0, 1).reshape(ns, nb * nch).astype(np.float64)
        y = cc.chain_double(x, c["sections"])[0].reshape(ns, nb, nch).transpose(1, 0, 2)
    return planar_of(trunc_i32(y), nb, nch, ns)


def stream_expected(c):
    """a carried case over its whole recording: the uncut answer [nblocks][nch][ns], and per section the rings (x, y), each
    [nc][nch], as the model holds them behind the last row"""
    P = c["planar"]
    nb, nch, ns = P.shape
    models = []
    y, _ = cc.chain_double(rows_of(P).astype(np.float64), sections_of(c), models)
    return planar_of(trunc_i32(y), nb, nch, ns), [(np.array(f.x, dtype=np.float64), np.array(f.y, dtype=np.float64)) for f in models]


def expected(c):
    """(answer, rings or None), computed once per case (read-only)"""
    return _expected(c["name"])


@functools.lru_cache(maxsize=None)
def _readme_answers():
    """every stateless README-pair case in ONE run of the model, the lanes of all cases side by side (its history of 8000 steps
    is then run once); a case's rows past its ns are zeros that nothing reads"""
    C = [c for c in all_cases() if c["kind"] == "cascade" and not c["calls"] and c["sections"] is README_PAIR]
    L = max(c["ns"] for c in C)
    cols = []
    for c in C:
        x = np.zeros((L, c["nblocks"] * c["nch"]))
        x[: c["ns"]] = c["planar"].transpose(2, 0, 1).reshape(c["ns"], -1)
        cols.append(x)
    y, out, at = cc.chain_double(np.concatenate(cols, axis=1), README_PAIR)[0], {}, 0
    for c, x in zip(C, cols):
        yc = y[: c["ns"], at : at + x.shape[1]].reshape(c["ns"], c["nblocks"], c["nch"]).transpose(1, 0, 2)
        out[c["name"]] = planar_of(trunc_i32(yc), c["nblocks"], c["nch"], c["ns"])
        at += x.shape[1]
    return out


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = by_name()[name]
    if c["kind"] == "cascade" and not c["calls"] and c["sections"] is README_PAIR:
        out = (_readme_answers()[name], None)
    else:
        out = stream_expected(c) if c["calls"] else (stateless_expected(c), None)
    out[0].setflags(write=False)
    return out


# ---- a sweep case as the planar entries see it ----

def sweep_planar(c):
    """native_to_i32 of the case's bytes, as [nblocks][nch][ns]"""
    return planar_of(native_to_i32(c["data"], c["bps"], c["nch"], c["ns"] * c["nblocks"]), c["nblocks"], c["nch"], c["ns"])


def sweep_doubles(c):
    """the model's doubles of a sweep case, in the native order [nblocks * ns][nch]"""
    leg, rows = c["leg"], c["ns"] * c["nblocks"]
    if leg == "single":
        return ic.iir_double(c["data"], c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"], c["shared"], c["nblocks"]).reshape(rows, c["nch"])
    if leg == "cascade":
        x = native_to_i32(c["data"], c["bps"], c["nch"], rows).astype(np.float64).reshape(c["nblocks"], c["ns"], c["nch"])
        y = cc.chain_double(x.transpose(1, 0, 2).reshape(c["ns"], -1), c["sections"])[0]
        return y.reshape(c["ns"], c["nblocks"], c["nch"]).transpose(1, 0, 2).reshape(rows, c["nch"])
    if leg in sw.STREAM_LEGS:
        return sw.stream_doubles(c)[0]
    raise ValueError(leg)


@functools.lru_cache(maxsize=None)
def _sweep_expected(leg, name):
    c = next(c for c in sw.sweep_cases()[leg] if c["name"] == name)
    out = planar_of(trunc_i32(sweep_doubles(c)), c["nblocks"], c["nch"], c["ns"])
    out.setflags(write=False)
    return out


def sweep_expected(c):
    """trunc_i32 of the model's doubles, uncut, as [nblocks][nch][ns] (computed once, read-only)"""
    return _sweep_expected(c["leg"], c["name"])


def cut(P, bps):
    """the native blocks (bytes) of a planar answer: what convert_i32_to_native makes of it"""
    return i32_to_native(rows_of(P), bps)


# ---- the cases ----

def _case(C, kind, name, P, off, calls=None, **kw):
    P.setflags(write=False)
    nb, nch, ns = P.shape
    C.append(dict(kind=kind, name=name, nch=nch, ns=ns, nblocks=nb, planar=P, off=off, calls=calls, bps=kw.pop("bps", 4), **kw))


def _single_kw(nc, init, shared):
    n, d = COEFS[nc]
    return dict(n=[float(v) for v in n], d=[float(v) for v in d], init=init, shared=shared)


README_PAIR = [([float(v) for v in n], [float(v) for v in d], init, f) for n, d, init, f in cc.README_PAIR]


@functools.lru_cache(maxsize=None)
def row_cases():
    """stateless row ends: every ns x offset, per channel and shared through the single stage, and through the cascade"""
    C, i = [], 0
    for ns in ROW_NS:
        for off in OFFSETS:
            nch = NCH[i % 4]
            nc = 2 + (i // 4 + i) % 4
            nb = (1, 2, 3)[i % 3]
            _case(C, "single", "row_single_ns%d_off%d_%dch_x%d_nc%d_per_channel" % (ns, off, nch, nb, nc), block(nb, nch, ns, 100 + i), off, **_single_kw(nc, 3, False))
            # shared: a lane is a block and the channels a serial chain -- the wide handles only at the shortest rows
            snch = NCH[(i + 1) % 4] if ns <= 67 else (3, 1)[i % 2]
            snb = (1, 5, 2)[i % 3]
            _case(C, "single", "row_single_ns%d_off%d_%dch_x%d_nc%d_shared" % (ns, off, snch, snb, nc), block(snb, snch, ns, 200 + i), off, **_single_kw(nc, 2, True))
            cnch = NCH[(i + 2) % 4]
            _case(C, "cascade", "row_cascade_ns%d_off%d_%dch_x%d_readme" % (ns, off, cnch, nb), block(nb, cnch, ns, 300 + i), off, sections=README_PAIR)
            i += 1
    return C


@functools.lru_cache(maxsize=None)
def stream_cases():
    """carried runs: handle ns x the cuts; three calls per recording, the first below the route switch or above it"""
    C, i = [], 0
    O, F = False, True
    for ns in STREAM_NS:
        for cut_ in STREAM_CUTS:
            nch, nc, off = NCH[i % 4], 2 + i % 4, OFFSETS[(i // 2) % 4]
            nb = sum(cut_)
            _case(C, "single", "stream_single_ns%d_%s_%dch_nc%d" % (ns, "".join(map(str, cut_)), nch, nc), block(nb, nch, ns, 400 + i), off, calls=cut_,
                  **_single_kw(nc, (0, 1, 5)[i % 3], False))
            secs = cc._sections(((5, 3), (2, 4, 5), (3,), (4, 2))[i % 4], (20, 0, 3), ((O, O), (O, F, O), (F,), (O, F))[i % 4])
            _case(C, "cascade", "stream_cascade_ns%d_%s_%dch_%s" % (ns, "".join(map(str, cut_)), NCH[(i + 1) % 4], sw._tag(secs)), block(nb, NCH[(i + 1) % 4], ns, 500 + i),
                  off, calls=cut_, sections=secs)
            i += 1
    return C


@functools.lru_cache(maxsize=None)
def route_cases():
    """the plain kernels: rows shorter than a chunk, and a history shorter than nc - 1 in front of a row of a chunk and more"""
    C, i = [], 0
    for ns in (1, 2, 15, 16, 17, 40, 63):
        for shared in (False, True):
            nch, nc = NCH[i % 4], 2 + i % 4
            _case(C, "single", "route_single_ns%d_%dch_nc%d_%s" % (ns, nch, nc, "shared" if shared else "per_channel"), block(3, nch, ns, 600 + i), OFFSETS[i % 4],
                  **_single_kw(nc, i % 3, shared))
            i += 1
    for ns in (1, 5, 31):
        for k in range(2):
            secs = cc._sections(((5, 3), (2, 4, 3))[k], (2, 0, 1), ((False, False), (True, False, True))[k])
            _case(C, "cascade", "route_cascade_ns%d_%dch_%s" % (ns, NCH[i % 4], sw._tag(secs)), block(2, NCH[i % 4], ns, 700 + i), OFFSETS[i % 4], sections=secs)
            i += 1
    for nc, ns in ((3, 100), (4, 64), (5, 129), (5, 200)):  # 4 * init < nc - 1: no history for the producers to stand on
        for shared in (False, True):
            nch = NCH[i % 4]
            _case(C, "single", "route_single_ns%d_%dch_nc%d_init0_%s" % (ns, nch, nc, "shared" if shared else "per_channel"), block(2, nch, ns, 800 + i), OFFSETS[i % 4],
                  **_single_kw(nc, 0, shared))
            i += 1
    return C


def _outside(bps, nb, nch, ns, seed):
    """full-scale int32 values, with 1 << 8 bps, its negative and the int32 limits at the rows' ends and inside them"""
    P = block(nb, nch, ns, seed, FULL)
    marks = (1 << (8 * bps), -(1 << (8 * bps)), FULL, -FULL - 1, (1 << (8 * bps)) + 1)
    for k, v in enumerate(marks):
        P[:, :, (k * 13) % ns] = v
    P[:, :, 0], P[:, :, ns - 1] = 1 << (8 * bps), -(1 << (8 * bps))
    return P


@functools.lru_cache(maxsize=None)
def width_cases():
    """handles of 1, 2 and 3 bytes per sample under values that need all 32 bits: the answer is the model's on the whole values"""
    C = []
    for bps in (1, 2, 3):
        nch, ns = (3, 65, 1)[bps - 1], (130, 70, 200)[bps - 1]
        tag = "width_i%d_%dch_ns%d" % (8 * bps, nch, ns)
        _case(C, "single", tag + "_single_per_channel", _outside(bps, 2, nch, ns, 900 + bps), 4 * bps, bps=bps, **_single_kw(5, 3, False))
        _case(C, "single", tag + "_single_shared", _outside(bps, 2, nch, ns, 910 + bps), 0, bps=bps, **_single_kw(3, 2, True))
        _case(C, "cascade", tag + "_cascade", _outside(bps, 2, nch, ns, 920 + bps), 8, bps=bps, sections=README_PAIR)
        _case(C, "single", tag + "_single_stream", _outside(bps, 3, nch, ns, 930 + bps), 12, calls=(1, 2), bps=bps, **_single_kw(4, 1, False))
        _case(C, "cascade", tag + "_cascade_stream", _outside(bps, 3, nch, ns, 940 + bps), 4, calls=(2, 1), bps=bps, sections=cc._sections((3, 5), (5, 0), (False, False)))
    return C


def all_cases():
    return row_cases() + stream_cases() + route_cases() + width_cases()


@functools.lru_cache(maxsize=None)
def by_name():
    C = all_cases()
    assert len({c["name"] for c in C}) == len(C)
    return {c["name"]: c for c in C}


def route(c, rows=None):
    """'pipe' or 'plain': the kernel a run of the case takes (rows: a carried call's length)"""
    if c["kind"] == "cascade":
        return "pipe" if (rows if c["calls"] else c["ns"]) >= CASCADE_CHUNK else "plain"
    if c["calls"]:
        return "pipe" if rows >= SINGLE_CHUNK else "plain"
    return "pipe" if ic.kernel_of(c["ns"], c["init"], len(c["n"])) == "pipe" else "plain"
