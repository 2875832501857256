"""The zero-phase IIR stage (rspt_hip_iir_zero_phase_batch_dev): its test inputs and a numpy restatement.

A case is nblocks blocks of the handle's shape (bps, nch, ns), one coefficient set (n, d) and the two history lengths.  The
reference user's loop is one fresh i_filter::new_iir object per (block, channel), run forward and then -- the same object, its
rings as they stand -- backward over its own untruncated output, as peak_detector_offline::detect runs its filters:
    f->init_history_values((double)x[0], init);         for t = 0 .. ns-1:  w[t] = f->filter_opt((double)x[t])
    f->init_history_values(w[ns-1], backward_init);     for t = ns-1 .. 0:  w[t] = f->filter_opt(w[t])
    y[t] = (int32_t)w[t]

The cases feed tests/golden/make_iir_zero_phase_record.py, which records the compiled reference's answers in
tests/golden/iir_zero_phase_record.json.  The tests take the coefficients from that record (stored exactly).
"""
import functools

import numpy as np

import cases
import iir_cases as ic
from casetools import _take
from fir_cases import crc, i32_to_native, native_to_i32, trunc_i32  # noqa: F401
from iir_model import IirModel
from rspt_amd import synth

CHUNK = 64  # k_iir_zp_pipe: samples per chunk; blocks of fewer rows take the plain kernel k_iir_zp

README_NAMES = ("readme_ecg12x2048x16_i32_bandpass", "readme_ds3x1000x20_i24_bandpass")
UNSTABLE_NAMES = ("unstable3x200x2_i32_pipe", "unstable2x60x3_i8_plain")
SAME_DATA_PAIR = ("ns200_i32_3ch_x2_nc3_init1_b1_plain", "ns200_i32_3ch_x2_nc3_init3_b1_pipe")


def kernel_of(ns, init, nc):
    """which kernel rspt_hip_iir_zero_phase_batch_dev runs (launch_iir_zero_phase)"""
    return "pipe" if ns >= CHUNK and init >= nc - 1 else "plain"


@functools.lru_cache(maxsize=None)
def zero_phase_cases():
    """name, bps, nch, ns, nblocks, n, d, init, binit, data (native bytes of nblocks * ns rows)"""
    C = []

    def add(name, bps, nch, ns, nblocks, coef, init, binit, data=None, seed=0, walk=False):
        if data is None:
            data = cases._rand_native(nch, ns * nblocks, bps, 7000 + seed, 1 << (8 * bps - 3), walk=walk)
        C.append(dict(name=name, bps=bps, nch=nch, ns=ns, nblocks=nblocks, n=[float(v) for v in coef[0]], d=[float(v) for v in coef[1]],
                      init=int(init), binit=int(binit), data=_take(data, bps, nch, ns * nblocks)))

    S = ic.STABLE
    # the README's band-pass (filter.h:113-114) on the two recordings
    add(README_NAMES[0], 4, 12, 2048, 16, cases.IIR_BANDPASS, 2000, 0, np.frombuffer(synth.ecg_12ch_i32(), dtype=np.uint8))
    add(README_NAMES[1], 3, 3, 1000, 20, cases.IIR_BANDPASS, 2000, 0, np.frombuffer(synth.data_stream_3ch_i24(), dtype=np.uint8))
    # ns around the chunk (a partial last chunk on both passes), nch around a wave and a workgroup, every width, 1..7 blocks,
    # every order, both kernels (ns < 64 or init < nc - 1: plain), every backward history
    add("ns1_i8_3ch_x7_nc3_init2000_b0", 1, 3, 1, 7, S[3], 2000, 0, seed=1)
    add("ns2_i16_65ch_x6_nc5_init3_b1", 2, 65, 2, 6, S[5], 3, 1, seed=2)  # (shorter than the ring: the history's x0 stays in it)
    add("ns5_i24_1ch_x5_nc4_init0_b2000", 3, 1, 5, 5, S[4], 0, 2000, seed=3)
    add("ns63_i32_64ch_x4_nc5_init2000_b0", 4, 64, 63, 4, S[5], 2000, 0, seed=4)
    add("ns64_i32_3ch_x3_nc5_init2000_b0", 4, 3, 64, 3, S[5], 2000, 0, seed=5, walk=True)
    add("ns64_i16_130ch_x2_nc2_init1_b1", 2, 130, 64, 2, S[2], 1, 1, seed=6)
    add("ns65_i24_3ch_x7_nc3_init3_b2000", 3, 3, 65, 7, S[3], 3, 2000, seed=7)
    add("ns65_i32_3ch_x2_nc3_init1_b0_plain", 4, 3, 65, 2, S[3], 1, 0, seed=8)
    add("ns103_i8_65ch_x1_nc4_init3_b1", 1, 65, 103, 1, S[4], 3, 1, seed=9)
    add("ns103_i32_3ch_x2_nc5_init3_b0_plain", 4, 3, 103, 2, S[5], 3, 0, seed=10)
    add("ns129_i32_130ch_x2_nc5_init2000_b1", 4, 130, 129, 2, S[5], 2000, 1, seed=11)  # (4 backward steps: one forward input stays in the ring)
    add("ns129_i16_3ch_x3_nc4_init0_b0_plain", 2, 3, 129, 3, S[4], 0, 0, seed=12)
    add("ns200_i32_3ch_x4_nc5_init2000_b2000", 4, 3, 200, 4, S[5], 2000, 2000, seed=13, walk=True)
    add("ns200_i24_64ch_x1_nc2_init2000_b0", 3, 64, 200, 1, S[2], 2000, 0, seed=14)
    add("ns200_i32_1ch_x1_nc4_init3_b0", 4, 1, 200, 1, S[4], 3, 0, seed=15)
    # the same data through the plain and through the pipelined kernel (init below and at nc - 1)
    add(SAME_DATA_PAIR[0], 4, 3, 200, 2, S[3], 1, 1, seed=16)
    add(SAME_DATA_PAIR[1], 4, 3, 200, 2, S[3], 3, 1, seed=16)
    # an unstable filter: the forward pass reaches +-inf and NaN before the turn, the backward pass starts from poisoned rings
    add(UNSTABLE_NAMES[0], 4, 3, 200, 2, ic.unstable(1e3), 3, 0, ic.onset_block(3, 400, 4, 7101, [None, 50, 0], 1000))
    add(UNSTABLE_NAMES[1], 1, 2, 60, 3, ic.unstable(1e10), 0, 1, ic.onset_block(2, 180, 1, 7102, [None, 10], 100))
    return C


# ---- the restatement ----

def zero_phase_double(x, n, d, init, binit):
    """x: [rows][lanes] float64, an independent object per lane.  -> (w after the backward pass, w after the forward pass),
    both [rows][lanes] and untruncated; every product and sum rounded on its own"""
    with np.errstate(over="ignore", invalid="ignore"):
        f = IirModel(n, d, np.zeros(x.shape[1]))
        f.init_history(x[0], 4 * init)
        fwd = np.array(f.run(list(x)))
        f.init_history(fwd[-1], 4 * binit)  # the same object: the rings run on
        back = np.array(f.run(list(fwd[::-1]))[::-1])
    return back, fwd


def _lanes(c):
    """the case's samples as [ns][nblocks * nch] float64: every (block, channel) a lane"""
    x = native_to_i32(c["data"], c["bps"], c["nch"], c["ns"] * c["nblocks"]).astype(np.float64).reshape(c["nblocks"], c["ns"], c["nch"])
    return x.transpose(1, 0, 2).reshape(c["ns"], -1)


def _blocks(c, y):
    return y.reshape(c["ns"], c["nblocks"], c["nch"]).transpose(1, 0, 2).reshape(c["ns"] * c["nblocks"], c["nch"])


def doubles(c, binit=None):
    """(backward, forward) untruncated outputs as [nblocks * ns][nch]"""
    back, fwd = zero_phase_double(_lanes(c), c["n"], c["d"], c["init"], c["binit"] if binit is None else binit)
    return _blocks(c, back), _blocks(c, fwd)


def filtered(c, binit=None):
    """the filtered blocks in the native sample width (bytes), as rspt_hip_iir_zero_phase_batch_dev writes them"""
    return i32_to_native(trunc_i32(doubles(c, binit)[0]), c["bps"])


def forward_reverse_forward(c):
    """what the single stage gives when it is called, the buffer reversed in time, and called again: a forward pass truncated to
    the sample width, then a fresh object, initialised on the LAST sample, over the reversed block, truncated again"""
    def forward(data):
        return ic.iir_prefilter(data, c["bps"], c["nch"], c["ns"], c["n"], c["d"], c["init"], shared=False, nblocks=c["nblocks"])

    def reverse(data):
        return np.ascontiguousarray(data.reshape(c["nblocks"], c["ns"], c["nch"] * c["bps"])[:, ::-1]).reshape(-1)

    return reverse(forward(reverse(forward(c["data"]))))


def to_record(c):
    return {"n": ic.to_bits(c["n"]), "d": ic.to_bits(c["d"]), "init": c["init"], "backward_init": c["binit"]}


def with_record_coefficients(c, r):
    """the case with the record's coefficients (exact) in place of the ones computed here"""
    return dict(c, n=ic.from_bits(r["n"]), d=ic.from_bits(r["d"]), rec=r)
