"""The zero-phase IIR stage on the planar int32 matrix (rspt_hip_iir_zero_phase_planar_batch_dev): test inputs and answers.

A planar buffer is the converters' int32 matrix [nblocks][nch][ns]: the whole int32 is the sample and the result is trunc_i32 of
the double, stored whole.  The answers come from the one restatement there is, iir_zero_phase_cases.zero_phase_double on
tests/iir_model.py, with every row of the matrix a lane.

    native_cases    the cases of tests/iir_zero_phase_cases.py as matrices: native_to_i32 of their bytes; the answer cut to the
                    case's bps is the compiled reference's record (tests/golden/iir_zero_phase_record.json)
    shape_cases     int32 rows of every length, row count, order and history the kernels tell apart, a seed per row
    width_cases     values outside the sample width of a narrower handle
The last two feed tests/golden/make_iir_zero_phase_planar_record.py, which drives them through the compiled reference at
bps = 4 and records its answers in tests/golden/iir_zero_phase_planar_record.json.

Every generated matrix has a different seed per row, so that a store past a row's end or a load clamped by address instead of by
index shows in the neighbouring row.  tests/test_iir_zero_phase_planar.py asserts what these lists cover.
"""
import functools

import numpy as np

import iir_cases as ic
import iir_zero_phase_cases as zc
from fir_cases import crc, i32_to_native, native_to_i32, trunc_i32  # noqa: F401
from iir_planar_cases import FULL, block, cut, native_of, planar_of, rows_of  # noqa: F401

CHUNK, PART = zc.CHUNK, 16
OFFSETS = (0, 4, 8, 12)  # bytes between a 16-byte boundary and the matrix
# what the issue names: the plain route, exactly one chunk, partial last chunks, rows whose starts are off 16 bytes, every partial part
NS = (1, 2, 5, 63, 64, 65, 67, 127, 128, 129, 191, 200)
NS_RESIDUES = (66, 68, 69, 70, 71, 73, 74, 75, 76, 77, 78)  # with NS: every residue of ns mod 16 through the pipelined kernel
ROWS = ((1, 1), (3, 1), (1, 3), (1, 64), (4, 16), (1, 65), (5, 13), (2, 65), (10, 13))  # (nblocks, nch): 1, 3, 64, 65, 130 rows
BINIT = (0, 1, 2000)
NEIGHBOURS = "shape_ns67_2x65_nc5_init2000_b0_neighbours"
UNSTABLE_NAMES, SAME_DATA_PAIR, README_NAMES = zc.UNSTABLE_NAMES, zc.SAME_DATA_PAIR, zc.README_NAMES


def inits(nc):
    """the forward histories the routes tell apart: none, one short of the ring's tail (the plain kernel at any length), the
    tail exactly, the harness's"""
    return (0, nc - 2, nc - 1, 2000)


def route(c):
    """'pipe' or 'plain': the kernel a call on the case takes (launch_iir_zero_phase)"""
    return zc.kernel_of(c["ns"], c["init"], len(c["n"]))


def _case(C, name, P, nc, init, binit, off, bps=4, coef=None):
    P.setflags(write=False)
    nb, nch, ns = P.shape
    n, d = coef if coef is not None else ic.STABLE[nc]
    C.append(dict(name=name, bps=bps, nch=nch, ns=ns, nblocks=nb, planar=P, n=[float(v) for v in n], d=[float(v) for v in d], init=int(init),
                  binit=int(binit), off=off))


@functools.lru_cache(maxsize=None)
def shape_cases():
    """two cases per row length the issue names, the row counts, orders and histories cycling through them; one through the
    pipelined kernel per further residue of the part; and the neighbours case: 130 rows of 67 samples, where every row starts
    off a 16-byte boundary and ends inside a part"""
    C = []

    def add(i, ns, rows, nc, init, binit, off):
        nb, nch = rows
        _case(C, "shape_ns%d_%dx%d_nc%d_init%d_b%d" % (ns, nb, nch, nc, init, binit), block(nb, nch, ns, 1100 + i), nc, init, binit, off)

    for k, ns in enumerate(NS):
        for j in range(2):
            nc = 2 + (k + 2 * j + k // 4) % 4
            add(2 * k + j, ns, ROWS[(k + 5 * j) % len(ROWS)], nc, inits(nc)[(k // 2 + 2 * j + 1) % 4], BINIT[(k + j + k // 3) % 3], OFFSETS[(k + 3 * j) % 4])
    for k, ns in enumerate(NS_RESIDUES):
        nc = 2 + (k + 1) % 4
        add(50 + k, ns, ROWS[(2 * k + 3) % len(ROWS)], nc, (nc - 1, 2000)[k % 2], BINIT[k % 3], OFFSETS[(k + 1) % 4])
    _case(C, NEIGHBOURS, block(2, 65, 67, 1199), 5, 2000, 0, 4)
    return C


def _outside(bps, nb, nch, ns, seed):
    """values far outside every narrower width (within +-2^26, so that the filters' gain stays inside int32), with 1 << 8 bps, its
    negative and the int32 limits inside the rows and at their ends (around the limits the answer overflows to INT32_MIN)"""
    P = block(nb, nch, ns, seed, 1 << 26)
    for k, v in enumerate((1 << (8 * bps), -(1 << (8 * bps)), FULL, -FULL - 1, (1 << (8 * bps)) + 1)):
        P[:, :, (k * 13 + 7) % ns] = v
    P[:, :, 0], P[:, :, ns - 1] = 1 << (8 * bps), -(1 << (8 * bps))
    return P


@functools.lru_cache(maxsize=None)
def width_cases():
    """handles of 1, 2 and 3 bytes per sample under values that need all 32 bits, through both kernels"""
    C = []
    for bps in (1, 2, 3):
        nch, ns = (3, 65, 1)[bps - 1], (130, 70, 200)[bps - 1]
        tag = "width_i%d_%dch_ns%d" % (8 * bps, nch, ns)
        _case(C, tag + "_pipe", _outside(bps, 2, nch, ns, 1200 + bps), 5, 4, 1, 4 * bps, bps=bps)
        _case(C, tag + "_plain", _outside(bps, 2, nch, ns, 1210 + bps), 4, 0, 0, 12 - 4 * bps, bps=bps)
    return C


def recorded_cases():
    """what tests/golden/iir_zero_phase_planar_record.json holds, in its order"""
    return shape_cases() + width_cases()


@functools.lru_cache(maxsize=None)
def native_cases():
    """the native record's cases as matrices (the coefficients as computed here: the tests take the record's)"""
    C = []
    for k, c in enumerate(zc.zero_phase_cases()):
        P = planar_of(native_to_i32(c["data"], c["bps"], c["nch"], c["ns"] * c["nblocks"]), c["nblocks"], c["nch"], c["ns"])
        _case(C, c["name"], P, len(c["n"]), c["init"], c["binit"], OFFSETS[k % 4], bps=c["bps"], coef=(c["n"], c["d"]))
    return C


# ---- the answers ----

def doubles(c):
    """(backward, forward) untruncated outputs as [nblocks][nch][ns]: every row of the matrix a lane of the restatement"""
    P = c["planar"]
    nb, nch, ns = P.shape
    x = P.reshape(nb * nch, ns).T.astype(np.float64)
    back, fwd = zc.zero_phase_double(x, c["n"], c["d"], c["init"], c["binit"])
    return back.T.reshape(nb, nch, ns), fwd.T.reshape(nb, nch, ns)


def expected(c):
    """the uncut answer [nblocks][nch][ns] int32, as rspt_hip_iir_zero_phase_planar_batch_dev stores it"""
    return np.ascontiguousarray(trunc_i32(doubles(c)[0]).reshape(c["planar"].shape))


def to_record(c):
    return {"n": ic.to_bits(c["n"]), "d": ic.to_bits(c["d"]), "init": c["init"], "backward_init": c["binit"]}


def with_record_coefficients(c, r):
    """the case with the record's coefficients (exact) in place of the ones computed here"""
    return dict(c, n=ic.from_bits(r["n"]), d=ic.from_bits(r["d"]), rec=r)
