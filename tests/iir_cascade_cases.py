"""The IIR cascade stage (rspt_hip_iir_cascade_batch_dev / _stream_dev): its test inputs and a numpy restatement.

A case is ONE recording of nblocks * ns rows cut into nblocks blocks of the handle's shape (bps, nch, ns), and a chain of 1 to 4
sections (n, d, init_nr_samples, use_filter).  The reference user's loop is one i_filter::new_iir object per section and
channel, every one initialised with init_history_values(the channel's RAW first sample, init), then per sample
v = x; v = f_k->filter(v) or f_k->filter_opt(v) for k = 0 .. S-1; y = (int32_t)v.  Two answers per case:
    stateless   a fresh chain per (block, channel): every block on its own
    stream      one chain per channel over the whole recording, wherever it is cut into calls

The cases feed tests/golden/make_iir_cascade_record.py, which records the compiled reference's answers in
tests/golden/iir_cascade_record.json.  The tests take the coefficients from that record (stored exactly).
"""
import functools

import numpy as np

import cases
import casetools
import iir_cases as ic
from casetools import _take
from fir_cases import crc, i32_to_native, native_to_i32, trunc_i32  # noqa: F401
from iir_model import IirModel
from rspt_amd import synth

CHUNK = 32  # k_iir_cascade_pipe: samples per chunk; runs of fewer rows take the plain kernel k_iir_cascade

HP04 = ([1.00000000000, -1.99822284729, 0.99822442503], [0.99911181808, -1.99822363616, 0.99911181808])  # filter.h:122-123
LP100 = cases.IIR_LOWPASS  # filter.h:116-117
README_PAIR = [(HP04[0], HP04[1], 2000, False), (LP100[0], LP100[1], 0, False)]  # lp->filter_opt(hp->filter_opt(x))
README_NAMES = ("readme_ecg12x2048x16_i32_hp04_lp100", "readme_ds3x1000x20_i24_hp04_lp100")


def _sections(ncs, inits, modes):
    return [(list(ic.STABLE[nc][0]), list(ic.STABLE[nc][1]), init, bool(m)) for nc, init, m in zip(ncs, inits, modes)]


@functools.lru_cache(maxsize=None)
def cascade_cases():
    """name, bps, nch, ns, nblocks, sections [(n, d, init, use_filter)], data (native bytes of nblocks * ns rows)"""
    C = []

    def add(name, bps, nch, ns, nblocks, sections, data=None, seed=0, walk=False):
        if data is None:
            data = cases._rand_native(nch, ns * nblocks, bps, 5000 + seed, 1 << (8 * bps - 3), walk=walk)
        secs = [([float(v) for v in n], [float(v) for v in d], int(init), bool(f)) for n, d, init, f in sections]
        C.append(dict(name=name, bps=bps, nch=nch, ns=ns, nblocks=nblocks, sections=secs, data=_take(data, bps, nch, ns * nblocks)))

    # the README's use: HP 0.4 Hz, then LP 100 Hz, on the two recordings
    add(README_NAMES[0], 4, 12, 2048, 16, README_PAIR, np.frombuffer(synth.ecg_12ch_i32(), dtype=np.uint8))
    add(README_NAMES[1], 3, 3, 1000, 20, README_PAIR, np.frombuffer(synth.data_stream_3ch_i24(), dtype=np.uint8))
    # ns around the chunk, nch around a wave and a workgroup, every width, 1..7 blocks, 1..4 sections, mixed orders, inits, modes
    O, F = False, True
    add("ns1_i8_3ch_x7_s2", 1, 3, 1, 7, _sections((3, 2), (2000, 0), (O, O)), seed=1)
    add("ns5_i16_65ch_x6_s3_mixed_modes", 2, 65, 5, 6, _sections((2, 5, 3), (3, 0, 1), (F, O, F)), seed=2)
    add("ns16_i32_3ch_x7_s2_plain_pipe_plain", 4, 3, 16, 7, _sections((5, 3), (2000, 0), (O, O)), seed=3, walk=True)
    add("ns31_i24_1ch_x5_s4_nc2534", 3, 1, 31, 5, _sections((2, 5, 3, 4), (2000, 0, 0, 0), (O, O, O, O)), seed=4)
    add("ns32_i32_64ch_x4_s2_nc55", 4, 64, 32, 4, _sections((5, 5), (50, 0), (O, O)), seed=5)
    add("ns33_i16_130ch_x3_s1", 2, 130, 33, 3, _sections((5,), (2000,), (O,)), seed=6)
    add("ns103_i32_3ch_x2_s4_nc2534_mixed_modes", 4, 3, 103, 2, _sections((2, 5, 3, 4), (100, 0, 7, 0), (O, F, O, F)), seed=7)
    add("ns103_i8_65ch_x1_s3_all_filter", 1, 65, 103, 1, _sections((4, 3, 5), (10, 10, 10), (F, F, F)), seed=8)
    add("ns33_i24_3ch_x7_s2_init0", 3, 3, 33, 7, _sections((3, 4), (0, 0), (O, O)), seed=9)
    add("ns31_i32_3ch_x3_s2_init0_plain", 4, 3, 31, 3, _sections((3, 4), (0, 0), (O, F)), seed=10)
    add("ns103_i16_5ch_x3_s1_filter", 2, 5, 103, 3, _sections((3,), (5,), (F,)), seed=11)
    add("ns103_i32_3ch_x2_s1_nc2", 4, 3, 103, 2, _sections((2,), (1,), (O,)), seed=12)
    add("ns96_i32_3ch_x2_s1_nc4_init0", 4, 3, 96, 2, _sections((4,), (0,), (O,)), seed=13)
    add("ns103_i32_130ch_x2_s3", 4, 130, 103, 2, _sections((5, 3, 5), (2000, 0, 0), (O, O, O)), seed=14)
    add("ns70_i24_3ch_x3_s4_all_filter", 3, 3, 70, 3, _sections((5, 2, 4, 3), (3, 0, 2, 0), (F, F, F, F)), seed=15)
    # the same data and coefficients through filter_opt and through filter
    for mode, tag in ((O, "opt"), (F, "filter")):
        add("ns103_i32_3ch_x2_s2_nc53_all_" + tag, 4, 3, 103, 2, _sections((5, 3), (20, 0), (mode, mode)), seed=16, walk=True)
    # an unstable section feeding a stable one: channel 1 is fed from row 700 on, passes 2^31, becomes +-inf and then NaN near
    # row 2450 (block 4); the stable section's rings carry the NaN over the block edge
    g15, g1e3 = ic.unstable(1.5), ic.unstable(1e3)
    add("unstable3x500x7_i32_into_lp100", 4, 3, 500, 7, [(g15[0], g15[1], 3, O), (LP100[0], LP100[1], 0, O)],
        ic.onset_block(3, 3500, 4, 5102, [None, 700, 0], 1000))
    add("unstable2x20x7_i8_into_nc4_small_calls", 1, 2, 20, 7, [(g1e3[0], g1e3[1], 0, O)] + _sections((4,), (0,), (F,)),
        ic.onset_block(2, 140, 1, 5103, [None, 5], 100))
    return C


# ---- the restatement ----

def chain_double(x, sections, models=None):
    """x: [rows][lanes] float64, an independent chain per lane.  -> the last section's outputs before the truncation, and every
    section's outputs ([S][rows][lanes]).  models: a list that takes the S filter objects as they stand behind the last row"""
    rows, lanes = x.shape
    per = np.empty((len(sections), rows, lanes))
    with np.errstate(over="ignore", invalid="ignore"):
        chain = []
        for n, d, init, use_filter in sections:  # every section's history is made of the RAW first sample
            f = IirModel(n, d, np.zeros(lanes))
            f.init_history(x[0], 4 * init)
            chain.append(f.filter if use_filter else f.filter_opt)
            if models is not None:
                models.append(f)
        for t in range(rows):
            v = x[t]
            for k, step in enumerate(chain):
                v = per[k, t] = step(v)
    return per[-1], per


def stream_double(c, sections=None):
    rows = c["ns"] * c["nblocks"]
    x = native_to_i32(c["data"], c["bps"], c["nch"], rows).astype(np.float64)
    return chain_double(x, c["sections"] if sections is None else sections)


def filtered(c, form, sections=None):
    """the filtered recording in the native sample width (bytes); form 'stream' or 'stateless'"""
    rows = c["ns"] * c["nblocks"]
    secs = c["sections"] if sections is None else sections
    if form == "stream":
        y = stream_double(c, secs)[0]
    else:  # every block a fresh chain: the blocks as further lanes
        x = native_to_i32(c["data"], c["bps"], c["nch"], rows).astype(np.float64).reshape(c["nblocks"], c["ns"], c["nch"])
        y = chain_double(x.transpose(1, 0, 2).reshape(c["ns"], -1), secs)[0].reshape(c["ns"], c["nblocks"], c["nch"]).transpose(1, 0, 2)
    return i32_to_native(trunc_i32(y.reshape(rows, c["nch"])), c["bps"])


def two_truncating_passes(c):
    """what two successive calls of the single-section stage give for a two-section chain (stream form): the first section's
    result truncated and stored in the sample width, the second section run on that, initialised with ITS first sample"""
    rows = c["ns"] * c["nblocks"]
    a, b = c["sections"]
    mid = dict(c, data=i32_to_native(trunc_i32(stream_double(c, [a])[0]), c["bps"]))
    return i32_to_native(trunc_i32(stream_double(mid, [b])[0].reshape(rows, c["nch"])), c["bps"])


def sections_to_record(c):
    return [{"n": ic.to_bits(n), "d": ic.to_bits(d), "init": init, "use_filter": int(f)} for n, d, init, f in c["sections"]]


def with_record_coefficients(c, r):
    """the case with the record's coefficients (exact) in place of the ones computed here"""
    return dict(c, sections=[(ic.from_bits(s["n"]), ic.from_bits(s["d"]), s["init"], bool(s["use_filter"])) for s in r["sections"]], rec=r)


def splits(c):
    """the drivings of a recording as a stream: all blocks in one call, one block per call, an uneven cut (1, 5, 1, 8, ... blocks)"""
    return casetools.splits(c["nblocks"], (1, 5, 1, 8))
