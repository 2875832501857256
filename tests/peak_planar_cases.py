"""Both R-peak detectors on the planar int32 matrix (rspt_hip_peak_detect_planar_batch_dev,
rspt_hip_peak_detect_offline_planar_batch_dev): the test matrices and what is expected of them.

A case is a matrix [nblocks][nch][ns] of int32, a handle width (which must not matter), a detector ("online": a variant of
tests/peak_cases.py; "offline": tests/peak_offline_cases.py), a sampling rate and a mode.  The detectors see row b * nch + c as
the samples of (block b, channel c), the whole int32 value as the sample -- so the expected answer is the restatement
(peak_cases.detect, peak_offline_cases.detect) on the transposed matrix [nblocks][ns][nch], which is also what the reference's
shims take.  tests/golden/make_peak_planar_record.py records the compiled reference's answers on recorded_cases() in
tests/golden/peak_planar_record.json; native_cases() are the native records' own cases as matrices, whose expected results are
those records'.
"""
import numpy as np

import peak_cases as pc
import peak_offline_cases as oc
from casetools import crc  # noqa: F401
from rspt_amd import synth

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1

# what the cases must cover (test_peak_planar.py: test_the_cases_cover_what_they_must)
ROW_LENGTHS = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 200)  # every residue mod 4, both sides of the 16-sample chunk
ROW_COUNTS = (1, 63, 64, 65, 130)                                       # the last wave partly empty, more than one wave
STATE_NCH, STATE_NBLOCKS = (1, 3, 65), (1, 2, 5)
BASE_OFFSETS = (0, 4, 8, 12)                                            # bytes from a 16-byte boundary
# the options every GPU run of a case is taken through (test_peak_planar.py: OPTION_RUNS picks from these)
MARKERS = (1.0, -1.0)
MAX_PEAKS = (0, 1, None)  # None: enough for every event
TRACES = (True, False)


def rows_of(P):
    """the matrix [nblocks][nch][ns] as the blocks [nblocks][ns][nch] the restatement and the reference's shims take"""
    return np.ascontiguousarray(np.asarray(P).transpose(0, 2, 1))


def planar_of(X):
    """blocks [nblocks][ns][nch] (samples or traces) as the matrix [nblocks][nch][ns]"""
    return np.ascontiguousarray(np.asarray(X).transpose(0, 2, 1))


def matrix_bytes(P):
    return np.ascontiguousarray(P, dtype="<i4").view(np.uint8).reshape(-1)


def _walk(nblocks, nch, ns, seed, amp=1 << 16):
    """random walks with a spike now and then: events at the low rates the short rows are run at"""
    rng = np.random.default_rng(seed)
    x = np.cumsum(rng.integers(-amp, amp + 1, size=(nblocks, nch, ns)), axis=2)
    x += np.where(rng.integers(0, 7, size=x.shape) == 0, amp * 40, 0)
    return np.clip(x, INT32_MIN, INT32_MAX).astype(np.int32)


def _ecg(nblocks, nch, ns, seed):
    """the synthetic ECG of the native cases, as a matrix"""
    blocks = [pc.native_to_i32(synth.synth_native(nch, ns, seed + b, bps=4, ecg=True).numpy(), 4, nch, ns) for b in range(nblocks)]
    return planar_of(np.stack(blocks)).astype(np.int32)


def _wide(nch, ns, seed):
    """an ECG scaled over the whole int32 range with INT32_MIN / INT32_MAX in it: cut to any narrower width it is another signal"""
    x = _ecg(1, nch, ns, seed).astype(np.int64)
    x = x * ((1 << 30) // max(1, int(np.abs(x).max())))
    x[0, :, 100::251] = INT32_MAX
    x[0, :, 177::263] = INT32_MIN
    return np.clip(x, INT32_MIN, INT32_MAX).astype(np.int32)


def recorded_cases():
    """name, kind, variant, fs, bps, nch, ns, nblocks, stateful, calls, planar, off, group"""
    C = []
    vn = sorted(pc.VARIANTS)

    def add(group, name, kind, fs, bps, planar, variant=None, stateful=False, calls=None):
        nblocks, nch, ns = planar.shape
        assert planar.dtype == np.int32
        C.append(dict(group=group, name="%s_%s_fs%g" % (name, variant if kind == "online" else "offline", fs), kind=kind,
                      variant=pc.VARIANTS[variant] if kind == "online" else None, fs=fs, bps=bps, nch=nch, ns=ns, nblocks=nblocks,
                      stateful=stateful, calls=calls, planar=planar, off=BASE_OFFSETS[(len(C) + len(C) // 4) % 4]))

    # row lengths: 2 x 3 rows; online at 5 Hz (nr_slope 0: an event on most samples) up to 3 samples and at 50 Hz above (a few events
    # a row: the record stays small), offline at 50 Hz (radius 0) and 250 Hz
    for k, ns in enumerate(ROW_LENGTHS):
        P = _walk(2, 3, ns, 100 + ns)
        for v in vn:
            add("len", "len2x3x%d" % ns, "online", 5.0 if ns <= 3 else 50.0, 1 + k % 4, P, v)
        add("len", "len2x3x%d" % ns, "offline", 50.0 if k % 2 == 0 else 250.0, 1 + k % 4, P)
    # row counts: ns 37 (rows on every residue mod 16) and 48 (three whole chunks, 16-byte loads at offset 0); 150 Hz
    # (an event on some rows) where there are many rows, for a small record
    for k, (nb, nch) in enumerate(((1, 1), (9, 7), (1, 64), (64, 1), (5, 13), (2, 65))):
        for ns in (37, 48):
            P = _walk(nb, nch, ns, 200 + 10 * k + ns)
            add("rows", "rows%dx%dx%d" % (nb, nch, ns), "online", 5.0 if nb * nch == 1 else 150.0, 4, P, vn[(k + ns) % 3])
            add("rows", "rows%dx%dx%d" % (nb, nch, ns), "offline", 50.0 if nb * nch == 1 else 150.0, 4, P)
    # carried state: channel c through rows c, nch + c, ...
    for i, nch in enumerate(STATE_NCH):
        for j, nb in enumerate(STATE_NBLOCKS):
            ns = (100, 50, 33)[j]
            P = _walk(nb, nch, ns, 300 + 10 * i + j)
            add("state", "state%dx%dx%d" % (nb, nch, ns), "online", (250.0, 50.0, 150.0)[i], 4, P, vn[(i + j) % 3], stateful=True)
            add("state", "state%dx%dx%d" % (nb, nch, ns), "offline", (50.0, 50.0, 150.0)[i], 4, P, stateful=True)
    add("state", "alt5x3x120", "offline", 50.0, 4, _walk(5, 3, 120, 390), stateful=True, calls=["fw", "detect", "detect", "fw", "detect"])
    # rows long enough for events at the native cases' rates
    E = _ecg(2, 3, 2500, 11)
    for v in vn:
        add("events", "ecg2x3x2500", "online", 250.0, 4, E, v)
    add("events", "ecg2x3x2500", "offline", 250.0, 4, E)
    E = planar_of(pc.native_to_i32(np.frombuffer(synth.ecg_12ch_i32(), dtype=np.uint8)[: 4 * 12 * 3001], 4, 12, 3001)[None]).astype(np.int32)
    add("events", "ecg1x12x3001", "online", 1000.0, 4, E, "online")
    add("events", "ecg1x12x3001", "online", 2000.0, 4, E, "online_1st")
    add("events", "ecg1x12x3001", "offline", 500.0, 4, E)
    S = _ecg(4, 3, 1000, 21)
    for v in vn:
        add("events", "ecgstate4x3x1000", "online", 360.0, 2, (S // 65536).astype(np.int32), v, stateful=True)
    add("events", "ecgstate4x3x1000", "offline", 360.0, 2, (S // 65536).astype(np.int32), stateful=True)
    # the offline detector's moved peaks (peak_offline_cases: revisits, collisions, firings near nr_slope_samples)
    add("moved", "trispikes1x4x4000", "offline", 250.0, 4, planar_of(oc._tri_spikes(4000)[None]).astype(np.int32))
    add("moved", "burst1x3x3000", "offline", 1000.0, 4, planar_of(oc._burst(3000, 3)[None]).astype(np.int32))
    add("moved", "ramps1x2x6000", "offline", 1000.0, 4, planar_of(oc._ramps(6000, 2)[None]).astype(np.int32))
    # widths: handles of bps 1, 2, 3 whose matrices hold values outside the width
    for bps in (1, 2, 3):
        W = _wide(3, 1500, 30 + bps)
        add("width", "wide1x3x1500_bps%d" % bps, "online", 250.0, bps, W, vn[bps % 3])
        add("width", "wide1x3x1500_bps%d" % bps, "offline", 250.0, bps, W)
    return C


def cut_to_width(P, bps):
    """what from_planar_i32 + the native entry sees of a matrix: every value cut to the handle's width"""
    nblocks, nch, ns = P.shape
    X = rows_of(P)
    return planar_of(np.stack([pc.native_to_i32(pc.i32_to_native(X[b], bps), bps, nch, ns) for b in range(nblocks)])).astype(np.int32)


def expected(c, marker=1.0, planar=None):
    """the restatement's answer on a case's matrix (or on `planar` in its place): what peak_cases.detect returns, traces
    [nblocks][ns][nch]"""
    X = rows_of(c["planar"] if planar is None else planar)
    if c["kind"] == "online":
        return pc.detect(X, c["variant"], c["fs"], marker, c["stateful"])
    return oc.detect(X, c["fs"], marker, c["stateful"], c["calls"])


def summarize(r, r_m1):
    """what the record holds of a case, from its marker 1.0 and marker -1.0 results (traces [nblocks][ns][nch])"""
    flat_count = lambda q: [v for row in q["count"] for v in row]  # noqa: E731
    return dict(count=flat_count(r), index=pc.flat(r["index"]), count_m1=flat_count(r_m1), index_m1=pc.flat(r_m1["index"]),
                values_m1=pc.vhex(pc.flat(r_m1["value"])), sig=pc.tdigest(r["sig"]), thr=pc.tdigest(r["thr"]))


RECORD_KEYS = ("count", "index", "count_m1", "index_m1", "values_m1", "sig", "thr")


def native_cases():
    """the native records' cases as matrices: (the case of peak_cases / peak_offline_cases with kind and planar added, its record
    file).  The detectors are blind to the layout, so the expected results are the native records' own."""
    out = []
    for kind, cs, rec in (("online", pc.peak_cases(), "peak_record.json"), ("offline", oc.offline_cases(), "peak_offline_record.json")):
        for c in cs:
            out.append((dict(c, kind=kind, variant=c.get("variant"), calls=c.get("calls"), planar=planar_of(pc.case_i32(c)).astype(np.int32)), rec))
    return out
