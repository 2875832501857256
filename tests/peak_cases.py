"""The R-peak detector stage: its test inputs and a numpy restatement of the reference.

Restates create_filter_iir (lib_rspt/lib_filter/iir_filter_design.cpp) and the three detectors of lib_rspt/peak_detector.h as
rspt_hip_peak_detect_batch_dev runs them (include/rspt_hip.h): one detector per (block, channel), or one per channel through the
blocks in order (stateful), fed (double) of every sample.  Every product and sum is one IEEE double operation in the reference's
order (numpy and Python floats round each on its own, as the reference's x86-64 build does), so the restatement is bit-exact.
The cases feed tests/golden/make_peak_record.py, which records the compiled reference's answers in tests/golden/peak_record.json.
"""
import hashlib
import math

import numpy as np

import cases
from casetools import _i32, crc  # noqa: F401
from fir_cases import i32_to_native, native_to_i32  # (the same sample reading as the other stages)
from iir_model import IirModel
from rspt_amd import synth

HIGH_PASS, LOW_PASS, BAND_PASS, BAND_STOP = 0, 1, 2, 3
ONLINE, ONLINE_1ST, OFFLINE_FW = 0, 1, 2
VARIANTS = {"online": ONLINE, "online_1st": ONLINE_1ST, "offline_fw": OFFLINE_FW}
INT32_MAX = (1 << 31) - 1


# ---- the designer ----

def _sqrt(v):
    """sqrt as C has it: NaN below zero (math.sqrt raises)"""
    return math.sqrt(v) if v >= 0 else float("nan")


def _binom_row(n, sign):
    """(z - 1)^n (sign -1) or (z + 1)^n (sign +1), highest power first, each coefficient built as the reference builds it"""
    out = []
    for k in range(n + 1):
        c = 1.0
        for i in range(1, k + 1):
            c = c * (float(n - i + 1) / i)
        out.append(c * (1.0 if (k % 2 == 0 or sign > 0) else -1.0))
    return out


def _conv(p, q):
    r = [0.0] * (len(p) + len(q) - 1)
    for i in range(len(p)):
        for j in range(len(q)):
            r[i + j] = r[i + j] + p[i] * q[j]
    return r


def design_iir(ftype, order, fs, lo, hi):
    """create_filter_iir(num, den, butterworth, ftype, order, fs, lo, hi): (num, den) lists, or None where it returns false"""
    if order == 2 and ftype in (LOW_PASS, HIGH_PASS):
        if fs <= 0 or lo <= 0:
            return None
        K = math.tan(math.pi * lo / fs)
        K2 = K * K
        r2 = _sqrt(2.0)
        a0 = 1.0 + r2 * K + K2
        a1 = 2.0 * (K2 - 1.0)
        a2 = 1.0 - r2 * K + K2
        num = [K2 / a0, (2.0 * K2) / a0, K2 / a0] if ftype == LOW_PASS else [1.0 / a0, -2.0 / a0, 1.0 / a0]
        return num, [1.0, a1 / a0, a2 / a0]
    if order == 2:
        if ftype != BAND_PASS or fs <= 0 or lo <= 0 or hi <= lo:
            return None
        k = 2.0 / (1.0 / fs)
        w1 = k * math.tan(math.pi * lo / fs)
        w2 = k * math.tan(math.pi * hi / fs)
        bw = w2 - w1
        w0 = _sqrt(w1 * w2)
        a3 = _sqrt(2.0) * bw
        a2 = 2.0 * w0 * w0 + bw * bw
        a1 = _sqrt(2.0) * bw * w0 * w0
        a0 = w0 * w0 * w0 * w0
        terms = [
            (_binom_row(4, -1), 1.0 * math.pow(k, 4)),
            (_conv(_binom_row(3, -1), _binom_row(1, 1)), a3 * math.pow(k, 3)),
            (_conv(_binom_row(2, -1), _binom_row(2, 1)), a2 * (k * k)),
            (_conv(_binom_row(1, -1), _binom_row(3, 1)), a1 * k),
            (_binom_row(4, 1), a0),
        ]
        den = [c * terms[0][1] for c in terms[0][0]]
        for poly, s in terms[1:]:
            den = [a + c * s for a, c in zip(den, poly)]
        g = bw * bw * (k * k)
        num = [c * g for c in (1.0, 0.0, -2.0, 0.0, 1.0)]
        norm = den[0]
        return [c / norm for c in num], [c / norm for c in den]
    if order == 1 and ftype in (LOW_PASS, HIGH_PASS):
        if fs <= 0 or lo <= 0:
            return None
        K = math.tan(math.pi * lo / fs)
        a0, a1 = 1.0 + K, 1.0 - K
        num = [K / a0, K / a0] if ftype == LOW_PASS else [1.0 / a0, -1.0 / a0]
        return num, [1.0, -a1 / a0]
    if order == 1:  # band_pass, and band_stop too: the reference's first-order band-pass never looks at the type
        if fs <= 0 or lo <= 0 or hi <= lo:
            return None
        K1 = math.tan(math.pi * lo / fs)
        K2 = math.tan(math.pi * hi / fs)
        nh = [1.0 / (1.0 + K1), -1.0 / (1.0 + K1)]
        dh = [1.0, -(1.0 - K1) / (1.0 + K1)]
        nl = [K2 / (1.0 + K2), K2 / (1.0 + K2)]
        dl = [1.0, -(1.0 - K2) / (1.0 + K2)]
        num = [nl[0] * nh[0], nl[0] * nh[1] + nl[1] * nh[0], nl[1] * nh[1]]
        den = [dl[0] * dh[0], dl[0] * dh[1] + dl[1] * dh[0], dl[1] * dh[1]]
        norm = den[0]
        return [c / norm for c in num], [c / norm for c in den]
    return None


# (type, order, lo, hi) of the band-pass, integrator and threshold filters, and the attenuation constant, per variant
DETECTOR_DESIGNS = {
    ONLINE: ((BAND_PASS, 2, 10.0, 20.0), (LOW_PASS, 2, 3.0, 0.0), (LOW_PASS, 2, 0.15, 0.0), 25.0),
    ONLINE_1ST: ((BAND_PASS, 1, 10.0, 20.0), (LOW_PASS, 1, 3.0, 0.0), (LOW_PASS, 2, 0.15, 0.0), 25.0),
    OFFLINE_FW: ((BAND_PASS, 1, 15.0, 25.0), (LOW_PASS, 1, 3.0, 0.0), (LOW_PASS, 2, 0.15, 0.0), 70.0),
}


def detector_constants(variant, fs):
    """the three filters as (ff, fb) -- the struct's d (the designer's numerator) and n (its denominator) -- and the constants"""
    bp, ig, th, A = DETECTOR_DESIGNS[variant]
    filt = []
    for t, o, lo, hi in (bp, ig, th):
        num, den = design_iir(t, o, fs, lo, hi)
        filt.append((num, den))
    return dict(filters=filt, nslope=int((100.0 * fs) / 1000.0), atten=1.0 / (1.0 + A / fs), hist=4 * int(fs))


# ---- the detector ----

class _Filt(IirModel):
    """an iir_filter_*_order over L lanes, from the designer's (ff, fb) = the object's (d, n); its history runs filter_opt"""

    def __init__(self, ff, fb, L):
        super().__init__(fb, ff, np.zeros(L))


class Detector:
    """L detectors of one variant and sampling rate, fresh"""

    def __init__(self, variant, fs, L):
        self.variant, self.fs, self.L = variant, float(fs), L
        k = detector_constants(variant, fs)
        self.k = k
        self.bp, self.ig, self.th = (_Filt(ff, fb, L) for ff, fb in k["filters"])
        self.prev_amp = np.zeros(L)
        self.prev_sig = np.zeros(L)
        self.searching = np.zeros(L, dtype=bool)
        self.after = np.zeros(L, dtype=np.int64)
        self.idx = np.zeros(L, dtype=np.int64)

    def block(self, x, marker):
        """x: [ns][L] (doubles of the samples).  Returns (fire [ns][L] bool, ret [ns][L], sig [ns][L], thr [ns][L])"""
        ns, L = x.shape
        k = self.k
        fire, ret = np.zeros((ns, L), dtype=bool), np.zeros((ns, L))
        sig, thr = np.zeros((ns, L)), np.zeros((ns, L))
        if self.variant == OFFLINE_FW and ns:
            self.bp.init_history(x[0], k["hist"], np.ones(L, dtype=bool), opt=True)  # (every detect_fw call)
        for t in range(ns):
            v = x[t]
            if self.variant != OFFLINE_FW:
                first = self.idx == 0  # (if (!sample_indx_++))
                if first.any():
                    self.bp.init_history(v, k["hist"], first, opt=True)
                self.idx = (self.idx + 1 + (1 << 31)) % (1 << 32) - (1 << 31)  # an int: wraps
            s = self.bp.filter_opt(v)
            s = self.ig.filter_opt(s * s)
            h = self.th.filter_opt(s)
            sig[t], thr[t] = s, h
            c1 = self.searching & (s > h * 1.5) & (self.prev_sig > s)
            take = c1 & ((self.prev_amp == 0) | (self.prev_sig > self.prev_amp * 0.5))
            damp = c1 & ~take
            c2 = ~c1 & (self.prev_sig < s)
            self.prev_amp = np.where(take, self.prev_sig, np.where(damp, self.prev_amp * k["atten"], self.prev_amp))
            self.after = np.where(take, 1, np.where(c2, 0, self.after))
            self.searching = np.where(take, False, np.where(c2, True, self.searching))
            self.prev_sig = s
            self.after = np.where(self.after != 0, self.after + 1, self.after)
            f = self.after == k["nslope"]
            self.after = np.where(f, 0, self.after)
            fire[t] = f
            ret[t] = np.where(f, s if marker == -1.0 else marker, 0.0)
        return fire, ret, sig, thr


def detect(x_i32, variant, fs, marker=1.0, stateful=False):
    """x_i32: [nblocks][ns][nch].  What rspt_hip_peak_detect_batch_dev computes, as lists per (block, channel):
    dict(count [nblocks][nch], index / value: [nblocks][nch] lists, sig / thr: [nblocks][ns][nch] doubles)."""
    with np.errstate(all="ignore"):
        return _detect(np.asarray(x_i32, dtype=np.float64), variant, fs, marker, stateful)


def _detect(x, variant, fs, marker, stateful):
    nblocks, ns, nch = x.shape
    fire = np.zeros((nblocks, ns, nch), dtype=bool)
    ret, sig, thr = (np.zeros((nblocks, ns, nch)) for _ in range(3))
    if stateful:
        d = Detector(variant, fs, nch)
        for b in range(nblocks):
            fire[b], ret[b], sig[b], thr[b] = d.block(x[b], marker)
    else:
        d = Detector(variant, fs, nblocks * nch)
        xs = x.transpose(1, 0, 2).reshape(ns, nblocks * nch)  # lanes = (block, channel)
        f, r, s, h = d.block(xs, marker)
        fire, ret, sig, thr = (a.reshape(ns, nblocks, nch).transpose(1, 0, 2) for a in (f, r, s, h))
    index = [[np.nonzero(fire[b, :, c])[0].tolist() for c in range(nch)] for b in range(nblocks)]
    value = [[ret[b, index[b][c], c].tolist() for c in range(nch)] for b in range(nblocks)]
    count = [[len(index[b][c]) for c in range(nch)] for b in range(nblocks)]
    return dict(count=count, index=index, value=value, sig=np.ascontiguousarray(sig), thr=np.ascontiguousarray(thr))


# ---- what the record holds ----

def canon(a):
    """doubles with every NaN made the one quiet NaN (x86-64 and gfx950 differ in NaN payloads, not in which values are NaN)"""
    a = np.ascontiguousarray(a, dtype=np.float64).copy()
    a[np.isnan(a)] = np.nan
    return a


def tdigest(a):
    """first 32 hex digits of the sha256 of a trace ([nblocks][ns][nch] doubles, NaNs made one)"""
    return hashlib.sha256(canon(a).tobytes()).hexdigest()[:32]


def vhex(values):
    """exact doubles as one hex string (little-endian float64, NaNs made one)"""
    return canon(np.asarray(values, dtype=np.float64).reshape(-1)).tobytes().hex()


def flat(lists):
    return [v for row in lists for col in row for v in col]


# ---- the GPU entries' results (torch is imported only here) ----

def dev(data):
    """native bytes -> a uint8 device tensor"""
    import torch

    return torch.from_numpy(np.array(data, dtype=np.uint8)).cuda()


def to_result(out, max_peaks, traces=True):
    """(count, index, value[, sig, thr]) tensors of a peak entry -> what detect returns (index / value lists cut at max_peaks)"""
    count = out[0].cpu().numpy().astype(np.int64)
    nblocks, nch = count.shape
    idx, val = out[1].cpu().numpy(), out[2].cpu().numpy()
    r = dict(count=count.tolist(),
             index=[[idx[b, c, : min(count[b, c], max_peaks)].tolist() for c in range(nch)] for b in range(nblocks)],
             value=[[val[b, c, : min(count[b, c], max_peaks)].tolist() for c in range(nch)] for b in range(nblocks)])
    if traces:
        r["sig"], r["thr"] = out[3].cpu().numpy(), out[4].cpu().numpy()
    return r


def events_equal(got, want, max_peaks=None):
    """counts, indices (the first max_peaks) and value bits (NaNs made one)"""
    assert got["count"] == want["count"]
    cut = (lambda l: l[:max_peaks]) if max_peaks is not None else (lambda l: l)  # noqa: E731
    for b in range(len(want["index"])):
        for c in range(len(want["index"][b])):
            assert got["index"][b][c] == cut(want["index"][b][c]), (b, c)
            assert vhex(got["value"][b][c]) == vhex(cut(want["value"][b][c])), (b, c)


# ---- the cases ----

def peak_inputs():
    """name, bps, nch, ns, nblocks, data (native bytes of nblocks blocks), fs list, stateful"""
    ecg = np.frombuffer(synth.ecg_12ch_i32(), dtype=np.uint8)
    ds = np.frombuffer(synth.data_stream_3ch_i24(), dtype=np.uint8)
    C = []

    def add(name, bps, nch, ns, data, fss, nblocks=1, stateful=False):
        data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).reshape(-1)[: bps * nch * ns * nblocks])
        assert data.size == bps * nch * ns * nblocks, name
        C.append(dict(name=name, bps=bps, nch=nch, ns=ns, nblocks=nblocks, data=data, fss=list(fss), stateful=stateful))

    add("ecg12x34199_i32", 4, 12, 34199, ecg, (500.0, 1000.0, 2000.0))
    add("ds3x20000_i24", 3, 3, 20000, ds, (1000.0,))
    add("const2x3000_i32", 4, 2, 3000, _i32(np.full(6000, 1000)), (500.0,))
    i8 = np.clip(synth.synth_native(4, 2500, 1, bps=4, ecg=True).numpy().view(np.int32) // 256, -128, 127)
    add("synth4x2500_i8", 1, 4, 2500, i32_to_native(i8, 1), (250.0,))
    add("synth5x3000_i16", 2, 5, 3000, synth.synth_native(5, 3000, 2, bps=2, ecg=True).numpy(), (360.0,))
    add("walk3x400_i16_fs5", 2, 3, 400, cases._rand_native(3, 400, 2, 91, 1 << 10, walk=True), (5.0,))
    add("walk2x500_i16_fs15", 2, 2, 500, cases._rand_native(2, 500, 2, 92, 1 << 10, walk=True), (15.0,))
    for ns in (1, 2, 63, 1237):
        add("synth3x%d_i32" % ns, 4, 3, ns, synth.synth_native(3, ns, 3, bps=4, ecg=True).numpy(), (250.0, 2000.0))
    spikes = np.zeros((4000, 4), dtype=np.int64)
    spikes[200::700, :] = INT32_MAX
    spikes[550::700, :] = -INT32_MAX - 1
    spikes[::3, 1] += cases.hash_i32(1334, 93, 1 << 20)[:1334]
    add("spikes4x4000_i32", 4, 4, 4000, _i32(np.clip(spikes, -INT32_MAX - 1, INT32_MAX)), (1000.0,))
    add("synth3blk7x1500_i32", 4, 7, 1500, np.concatenate([synth.synth_native(7, 1500, b, bps=4, ecg=True).numpy() for b in range(3)]),
        (500.0,), nblocks=3)
    # stateful: one detector per channel through the blocks (the ECG recording cut into 4 blocks of 8000 samples)
    add("ecg12x4blk8000_i32_state", 4, 12, 8000, ecg, (2000.0,), nblocks=4, stateful=True)
    add("synth3x4blk997_i16_state", 2, 3, 997, np.concatenate([synth.synth_native(3, 997, b, bps=2, ecg=True).numpy() for b in range(4)]),
        (250.0, 15.0), nblocks=4, stateful=True)
    return C


def peak_cases():
    """every input x every variant x each of its sampling rates: name, variant, fs, and the input's fields"""
    out = []
    for inp in peak_inputs():
        for fs in inp["fss"]:
            for vname, v in VARIANTS.items():
                c = dict(inp, variant=v, fs=fs, name="%s_%s_fs%g" % (inp["name"], vname, fs))
                del c["fss"]
                out.append(c)
    return out


def case_i32(c):
    """[nblocks][ns][nch] int32 of a case's native bytes"""
    bb = c["bps"] * c["nch"] * c["ns"]
    return np.stack([native_to_i32(c["data"][b * bb : (b + 1) * bb], c["bps"], c["nch"], c["ns"]) for b in range(c["nblocks"])])


def summarize(r, r_m1):
    """the record of one case from the marker 1.0 and -1.0 results"""
    return dict(count=[v for row in r["count"] for v in row], index=flat(r["index"]), values_m1=vhex(flat(r_m1["value"])),
                sig=tdigest(r["sig"]), thr=tdigest(r["thr"]))


# ---- the designer grid ----

DESIGN_FS = (250.0, 500.0, 1000.0, 2000.0, 15.0, 360.5, 0.0, -100.0)
DESIGN_CUTS = ((10.0, 20.0), (15.0, 25.0), (3.0, 0.0), (0.15, 0.0), (0.5, 40.0), (0.0, 10.0), (20.0, 10.0), (-1.0, 5.0))


def design_grid():
    return [(t, o, fs, lo, hi) for t in range(4) for o in range(4) for fs in DESIGN_FS for lo, hi in DESIGN_CUTS]
