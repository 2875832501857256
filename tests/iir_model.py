"""The reference's IIR filter object, restated once for every test that judges a stage against it.

Restates i_filter::new_iir's object (lib_rspt/lib_filter/iir_filter.cpp:46-116; the iir_filter_*_order classes of
lib_rspt/iir_filter_opt.h run the same filter_opt expression): two rings of nc values, newest first, and every product and sum
one IEEE double operation in the reference's order (numpy and Python floats round each on its own, as the reference's x86-64
build does), so the restatement is bit-exact.  The device-side counterpart is rspt_amd/csrc/iir.hpp.

A ring element is a Python float or a numpy array: one independent object per lane.  The steps never write into an element,
and they keep the caller's input in the x ring as it is, so a caller that overwrites an array it has fed passes a copy.
"""
import numpy as np


class IirModel:
    """x[i], y[i] = input / output i samples ago; n the feedback and d the feed-forward coefficients (n[0] is never read)"""

    def __init__(self, n, d, zero=0.0):
        """zero: what the rings start from -- 0.0, or np.zeros(lanes)"""
        self.n, self.d = [float(v) for v in n], [float(v) for v in d]
        self.x, self.y = [zero] * len(self.n), [zero] * len(self.n)

    def filter(self, v):
        """filter(): feed-forward and feedback terms interleaved"""
        n, d = self.n, self.d
        x = self.x = [v] + self.x[:-1]
        y = self.y = [None] + self.y[:-1]
        acc = d[0] * v
        for i in range(1, len(n)):
            acc = acc + d[i] * x[i]
            acc = acc - n[i] * y[i]
        y[0] = acc
        return acc

    def filter_opt(self, v):
        """filter_opt() (rolling_iir_filter_N_): one expression, left to right, every feed-forward term first"""
        n, d = self.n, self.d
        x = self.x = [v] + self.x[:-1]
        y = self.y = [None] + self.y[:-1]
        acc = d[0] * v
        for i in range(1, len(n)):
            acc = acc + d[i] * x[i]
        for i in range(1, len(n)):
            acc = acc - n[i] * y[i]
        y[0] = acc
        return acc

    def init_history(self, v, steps, mask=None, opt=False):
        """init_history_values(v, steps / 4): steps calls on v -- of filter(), or with opt of the filter_opt expression, which
        is what the iir_filter_*_order classes run for their history.  mask: only on those lanes; the others keep their rings"""
        keep = (self.x, self.y)
        step = self.filter_opt if opt else self.filter
        for _ in range(steps):
            step(v)
        if mask is not None:
            self.x, self.y = ([np.where(mask, a, b) for a, b in zip(new, old)] for new, old in zip((self.x, self.y), keep))

    def run(self, cols, opt=True):
        """the outputs of one call per element of cols, in order"""
        step = self.filter_opt if opt else self.filter
        return [step(v) for v in cols]


def state_rings(state, nch, S=1):
    """a device state's bytes by the layout rspt_hip.h documents: per channel, and per channel x section for the cascade,
    double x[5], y[5]; uint64 started -> x, y as [nch][S][5] float64 and started as [nch][S] uint64"""
    raw = state.cpu().numpy()
    assert raw.size == 88 * nch * S
    words = raw.view(np.uint64).reshape(nch, S, 11)
    return words[:, :, 0:5].view(np.float64), words[:, :, 5:10].view(np.float64), words[:, :, 10]


def same_doubles(a, b):
    """bit for bit, but any NaN matches any NaN (payload and sign differ between x86 and the GPU)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
