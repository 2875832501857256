"""The zero-phase offline R-peak detector: its test inputs and a numpy restatement of the reference.

Restates peak_detector_offline::detect (lib_rspt/peak_detector.h) as rspt_hip_peak_detect_offline_batch_dev runs it
(include/rspt_hip.h): one object per (block, channel), or one per channel through the blocks in order (stateful), vectorised
across those lanes and looping over time.  Every product and sum is one IEEE double operation in the reference's order, so the
restatement is bit-exact.  The cases feed tests/golden/make_peak_offline_record.py, which records the compiled reference's
answers in tests/golden/peak_offline_record.json.
"""
import numpy as np

import cases
import peak_cases as pc
from casetools import _i32
from rspt_amd import synth

BASELINE = (pc.LOW_PASS, 1, 0.5, 0.0)


def constants(fs):
    """band-pass, integrator, threshold (as detect_fw's), the baseline, and the constants of peak_detector_offline(fs)"""
    k = pc.detector_constants(pc.OFFLINE_FW, fs)
    k["baseline"] = pc.design_iir(*BASELINE[:2], fs, *BASELINE[2:])
    k["radius"] = int((10.0 * fs) / 1000.0)
    return k


class Offline:
    """L peak_detector_offline objects of one sampling rate, fresh"""

    def __init__(self, fs, L):
        self.fs, self.L = float(fs), L
        self.k = k = constants(fs)
        self.bp, self.ig, self.th = (pc._Filt(ff, fb, L) for ff, fb in k["filters"])
        self.bl = pc._Filt(*k["baseline"], L)
        self.prev_amp = np.zeros(L)
        self.prev_sig = np.zeros(L)
        self.searching = np.zeros(L, dtype=bool)
        self.after = np.zeros(L, dtype=np.int64)
        self.stats = dict(revisit_moves=0, collisions=0, collisions_ahead=0)
        self.collided = np.zeros(L, dtype=bool)  # (lanes with a collision)

    def _machine(self, s, h, marker):
        k = self.k
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
        return f, np.where(f, s if marker == -1.0 else marker, 0.0)

    def fw(self, x, marker):
        """detect_fw on x [ns][L]: (peak_signal, filt_signal, threshold_signal, fired) [ns][L]"""
        ns, L = x.shape
        self.bp.init_history(x[0], self.k["hist"], np.ones(L, dtype=bool), opt=True)
        f, h, p = np.zeros((ns, L)), np.zeros((ns, L)), np.zeros((ns, L))
        fired = np.zeros((ns, L), dtype=bool)
        for t in range(ns):
            f[t] = self.bp.filter_opt(x[t])
        for t in range(ns):
            f[t] = self.ig.filter_opt(f[t] * f[t])
        for t in range(ns):
            h[t] = self.th.filter_opt(f[t])
        for t in range(ns):
            fired[t], p[t] = self._machine(f[t], h[t], marker)
        return p, f, h, fired

    def detect(self, x, marker):
        """detect on x [ns][L]: (peak_signal, filt_signal, threshold_signal) [ns][L]"""
        ns, L = x.shape
        k = self.k
        all_ = np.ones(L, dtype=bool)
        self.bp.init_history(x[0], k["hist"], all_, opt=True)
        self.bl.init_history(x[0], k["hist"], all_, opt=True)
        b, f, h, p = (np.zeros((ns, L)) for _ in range(4))
        for t in range(ns):
            b[t] = self.bl.filter_opt(x[t])
        for t in range(ns - 1, -1, -1):
            b[t] = self.bl.filter_opt(b[t].copy())  # (a copy: the filter keeps its input, and b[t] is overwritten)
        for t in range(ns):
            self.bp.filter_opt(x[t])
        for t in range(ns - 1, -1, -1):
            f[t] = self.bp.filter_opt(x[t])  # (on the input again)
        for t in range(ns):
            f[t] = self.ig.filter_opt(f[t] * f[t])
        for t in range(ns - 1, -1, -1):
            f[t] = self.ig.filter_opt(f[t].copy())
        for t in range(ns):
            self.th.filter_opt(f[t])
        for t in range(ns - 1, -1, -1):
            h[t] = self.th.filter_opt(f[t])
        for t in range(ns):
            p[t] = self._machine(f[t], h[t], marker)[1]
        ns_ = k["nslope"]
        for i in range(ns_, ns):
            nz = p[i] != 0
            if nz.any():
                p[i - ns_ + 1] = np.where(nz, p[i], p[i - ns_ + 1])
                p[i] = np.where(nz, 0.0, p[i])
        r = k["radius"]
        v = x - b
        lanes = np.arange(L)
        moved = np.zeros((ns, L), dtype=bool)  # (positions a value was moved ahead to: for the statistics)
        for i in range(r, ns - r):
            nz = p[i] != 0
            if not nz.any():
                continue
            ls = lanes[nz]
            mx, mxi = np.full(ls.size, -2000000.0), np.zeros(ls.size, dtype=np.int64)
            mn, mni = np.full(ls.size, 2000000.0), np.zeros(ls.size, dtype=np.int64)
            if r:
                w = v[i - r : i + r][:, ls]  # j = -r .. r - 1
                wmax = np.where(np.isnan(w), -np.inf, w)
                wmin = np.where(np.isnan(w), np.inf, w)
                am, an = wmax.argmax(axis=0), wmin.argmin(axis=0)  # (the first of equal values: strict < / >)
                m, n = wmax[am, np.arange(ls.size)], wmin[an, np.arange(ls.size)]
                up, dn = m > mx, n < mn
                mx, mxi = np.where(up, m, mx), np.where(up, i - r + am, mxi)
                mn, mni = np.where(dn, n, mn), np.where(dn, i - r + an, mni)
            to = np.where(mx > -mn, mxi, mni)
            val = p[i, ls].copy()
            p[i, ls] = 0.0
            self.stats["revisit_moves"] += int((moved[i, ls] & (to != i)).sum())
            hit = p[to, ls] != 0
            self.stats["collisions"] += int(hit.sum())
            self.stats["collisions_ahead"] += int((hit & (to > i)).sum())  # (onto a live peak not yet visited)
            self.collided[ls[hit]] = True
            p[to, ls] = val
            moved[to[to > i], ls[to > i]] = True
        return p, f, h


def detect(x_i32, fs, marker=1.0, stateful=False, calls=None, stats=None):
    """x_i32: [nblocks][ns][nch].  What rspt_hip_peak_detect_offline_batch_dev computes, as lists per (block, channel):
    dict(count, index, value, sig, thr), as peak_cases.detect returns it.  calls (stateful only): per block "detect" or "fw"
    (detect_fw, whose events are its firings, as rspt_hip_peak_detect_batch_dev reports them); default all "detect".
    stats: a dict that receives the relocation's revisit_moves and collisions."""
    with np.errstate(all="ignore"):
        x = np.asarray(x_i32, dtype=np.float64)
        nblocks, ns, nch = x.shape
        p, f, h = (np.zeros((nblocks, ns, nch)) for _ in range(3))
        fired = np.zeros((nblocks, ns, nch), dtype=bool)
        if stateful:
            d = Offline(fs, nch)
            for b in range(nblocks):
                if calls is not None and calls[b] == "fw":
                    p[b], f[b], h[b], fired[b] = d.fw(x[b], marker)
                else:
                    p[b], f[b], h[b] = d.detect(x[b], marker)
                    fired[b] = p[b] != 0
        else:
            d = Offline(fs, nblocks * nch)
            xs = x.transpose(1, 0, 2).reshape(ns, nblocks * nch)
            a = d.detect(xs, marker)
            p, f, h = (t.reshape(ns, nblocks, nch).transpose(1, 0, 2) for t in a)
            fired = p != 0
        if stats is not None:
            stats.update(d.stats)
    index = [[np.nonzero(fired[b, :, c])[0].tolist() for c in range(nch)] for b in range(nblocks)]
    value = [[p[b, index[b][c], c].tolist() for c in range(nch)] for b in range(nblocks)]
    count = [[len(index[b][c]) for c in range(nch)] for b in range(nblocks)]
    return dict(count=count, index=index, value=value, sig=np.ascontiguousarray(f), thr=np.ascontiguousarray(h))


# ---- the cases ----

def offline_inputs():
    """name, bps, nch, ns, nblocks, data (native bytes of nblocks blocks), fs list, stateful, calls"""
    ecg = np.frombuffer(synth.ecg_12ch_i32(), dtype=np.uint8)
    C = []

    def add(name, bps, nch, ns, data, fss, nblocks=1, stateful=False, calls=None):
        data = np.ascontiguousarray(np.asarray(data, dtype=np.uint8).reshape(-1)[: bps * nch * ns * nblocks])
        assert data.size == bps * nch * ns * nblocks, name
        C.append(dict(name=name, bps=bps, nch=nch, ns=ns, nblocks=nblocks, data=data, fss=list(fss), stateful=stateful, calls=calls))

    add("ecg12x34199_i32", 4, 12, 34199, ecg, (250.0, 500.0, 1000.0, 2000.0))
    i8 = np.clip(synth.synth_native(4, 2500, 1, bps=4, ecg=True).numpy().view(np.int32) // 256, -128, 127)
    add("synth4x2500_i8", 1, 4, 2500, pc.i32_to_native(i8, 1), (250.0,))
    add("synth5x3000_i16", 2, 5, 3000, synth.synth_native(5, 3000, 2, bps=2, ecg=True).numpy(), (360.0,))
    add("ds3x20000_i24", 3, 3, 20000, np.frombuffer(synth.data_stream_3ch_i24(), dtype=np.uint8), (1000.0,))
    add("synth7x3blk1500_i32", 4, 7, 1500, np.concatenate([synth.synth_native(7, 1500, b, bps=4, ecg=True).numpy() for b in range(3)]),
        (500.0,), nblocks=3)
    add("ecg12x4blk8000_i32_state", 4, 12, 8000, ecg, (2000.0,), nblocks=4, stateful=True)
    add("ecg12x4blk6000_i32_alt", 4, 12, 6000, ecg, (1000.0,), nblocks=4, stateful=True, calls=["fw", "detect", "fw", "detect"])
    add("synth3x2000_i16_fs50", 2, 3, 2000, synth.synth_native(3, 2000, 4, bps=2, ecg=True).numpy(), (50.0,))
    add("walk2x500_i16_fs15", 2, 2, 500, cases._rand_native(2, 500, 2, 92, 1 << 10, walk=True), (15.0,))
    add("ramps2x6000_i32", 4, 2, 6000, _i32(_ramps(6000, 2)), (1000.0,))
    add("burst3x3000_i32", 4, 3, 3000, _i32(_burst(3000, 3)), (1000.0,))
    add("trispikes4x4000_i32", 4, 4, 4000, _i32(_tri_spikes(4000)), (250.0,))
    return C


def _ramps(ns, nch):
    """spikes that fire the detector, each followed by a long rising ramp of x - baseline: a peak relocated onto the ramp is
    visited again and moved on along it"""
    t = np.arange(ns)
    x = np.zeros((ns, nch), dtype=np.int64)
    for c in range(nch):
        period = 700 + 90 * c
        ph = t % period
        x[:, c] = np.where(ph < 8, 400000, 0) + np.where((ph >= 8) & (ph < 220), (ph - 8) * (1500 + 200 * c), 0)
    return x


def _tri_spikes(ns):
    """a triangle wave with a spike train on it, one (period, slope, phase, spike, spacing, width) per channel.  At 250 Hz
    (radius 2) peaks relocated onto the rising ramps are visited again and move up them, and chains of two peaks meet: a peak
    moves ahead onto a live one not yet visited, or onto one already at the top (collisions at a radius above 0)"""
    t = np.arange(ns)
    chans = ((319, 1000, 0, 100000, 81, 2), (600, 10000, 0, -1000000, 58, 1), (1445, 1000, 0, 100000, 58, 1), (600, 10000, 200, 1000000, 81, 2))
    return np.stack([np.abs(((t + ph) % P) * 2 - P) * S + np.where((t % sp) < w, a, 0) for P, S, ph, a, sp, w in chans], axis=1)


def _burst(ns, nch):
    """sharp bursts from the first samples on, over noise: firings from the block's start, near nr_slope_samples"""
    x = np.zeros((ns, nch), dtype=np.int64)
    for c in range(nch):
        seq = cases.hash_i32(ns, 300 + c, 1 << 12)[:ns].astype(np.int64)
        x[:, c] = seq
        for s in (2 + c, 100 + 3 * c, 205 + c):
            x[s : s + 3, c] += 3000000
        x[:: 500 + 40 * c, c] += 2000000
    return x


def offline_cases():
    """every input x each of its sampling rates"""
    out = []
    for inp in offline_inputs():
        for fs in inp["fss"]:
            c = dict(inp, fs=fs, name="%s_fs%g" % (inp["name"], fs))
            del c["fss"]
            out.append(c)
    return out


def case_i32(c):
    return pc.case_i32(c)
