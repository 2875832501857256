"""init_history_values with fewer calls than the ring has places: init_nr_samples = 1 with five coefficients.

The history initialisation is 4 * init_nr_samples calls of filter() on the channel's first sample.  With init_nr_samples = 1 and
five coefficients that is four calls: the x ring never fills with the first sample, its last place stays 0.0, and the
constant-input shortcut of the kernels (IirState::init_history, iir.hpp) is never reached.  Every kernel that initialises a
filter is driven there -- k_iir and k_iir_carry (ns = 40), k_iir_pipe (ns = 70: one full chunk and a tail), the cascade's plain
kernel (ns = 31) and its pipelined one (ns = 33), the cascades with one filter_opt and one filter section -- on 3 channels of int32
and int24, stateless and carried.  Expected values are the numpy restatements' (tests/iir_cases.py, tests/iir_cascade_cases.py),
compared bit for bit."""
import functools

import numpy as np
import pytest

import iir_cascade_cases as cc
import iir_cases as ic
from devframe import api  # noqa: F401

NC, INIT, NCH, NBLOCKS = 5, 1, 3, 2
N5, D5 = ic.STABLE[NC]
WIDTHS = (4, 3)


def _data(bps, ns):
    return ic.cases._rand_native(NCH, ns * NBLOCKS, bps, 7100 + 10 * ns + bps, 1 << (8 * bps - 3))


@functools.lru_cache(maxsize=None)
def _want_iir(bps, ns, form):
    """the restatement's answer for NBLOCKS blocks of ns rows, computed once per process (read-only)"""
    data = _data(bps, ns)
    if form == "carried":  # one filter per channel over the whole recording
        y = ic.iir_prefilter(data, bps, NCH, ns * NBLOCKS, N5, D5, INIT, shared=False)
    else:
        y = ic.iir_prefilter(data, bps, NCH, ns, N5, D5, INIT, shared=form == "shared", nblocks=NBLOCKS)
    y = np.ascontiguousarray(y).reshape(-1)
    y.setflags(write=False)
    return y


def _cascade_case(bps, ns):
    sections = [(list(N5), list(D5), INIT, False), (list(N5), list(D5), INIT, True)]  # filter_opt, then filter
    return dict(bps=bps, nch=NCH, ns=ns, nblocks=NBLOCKS, sections=sections, data=_data(bps, ns))


@functools.lru_cache(maxsize=None)
def _want_cascade(bps, ns, form):
    y = np.ascontiguousarray(cc.filtered(_cascade_case(bps, ns), form)).reshape(-1)
    y.setflags(write=False)
    return y


def test_the_case_stops_short_of_a_full_ring():
    """fewer calls of filter() than the ring has places, and the kernels' routes are the ones named above"""
    assert 4 * INIT < NC == len(N5) == len(D5)
    assert ic.kernel_of(40, INIT, NC) == "iir" and ic.kernel_of(70, INIT, NC) == "pipe" and ic.CHUNK_PIPE < 70 < 2 * ic.CHUNK_PIPE
    assert 31 < cc.CHUNK < 33


@pytest.mark.gpu
@pytest.mark.parametrize("bps", WIDTHS)
@pytest.mark.parametrize("ns", [40, 70])
@pytest.mark.parametrize("form", ["per_channel", "shared", "carried"])
def test_gpu_iir_prefilter(api, bps, ns, form):
    """k_iir (ns = 40) and k_iir_pipe (ns = 70), a filter per channel and one for all channels; carried: one call per block on
    one state, k_iir_carry and k_iir_pipe's carried form, the first call initialising and the second continuing"""
    import torch

    pk = api.new_hzr(bps, NCH, ns)
    buf = torch.from_numpy(np.array(_data(bps, ns))).cuda()
    if form == "carried":
        state, bb = pk.iir_state(), pk.block_bytes
        for b in range(NBLOCKS):
            pk.iir_prefilter_batch(buf[b * bb : (b + 1) * bb], N5, D5, INIT, per_channel=True, state=state)
    else:
        pk.iir_prefilter_batch(buf, N5, D5, INIT, per_channel=form == "per_channel")
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), _want_iir(bps, ns, form))
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bps", WIDTHS)
@pytest.mark.parametrize("ns", [31, 33])
@pytest.mark.parametrize("form", ["stateless", "stream"])
def test_gpu_iir_cascade(api, bps, ns, form):
    """k_iir_cascade (ns = 31) and k_iir_cascade_pipe (ns = 33): a filter_opt section, then a filter section, both short of a
    full ring; stream: one call per block on one state"""
    import torch

    pk = api.new_hzr(bps, NCH, ns)
    c = _cascade_case(bps, ns)
    buf = torch.from_numpy(np.array(c["data"])).cuda()
    if form == "stream":
        state, bb = pk.iir_cascade_state(2), pk.block_bytes
        for b in range(NBLOCKS):
            pk.iir_cascade_batch(buf[b * bb : (b + 1) * bb], c["sections"], state=state)
    else:
        pk.iir_cascade_batch(buf, c["sections"])
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy(), _want_cascade(bps, ns, form))
    pk.close()
