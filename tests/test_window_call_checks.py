"""The order of the argument checks of the eight sliding-window entries: FIR and median, native block and planar int32 matrix,
stateless and carried (rspt_hip_{fir_prefilter,median_filter}[_planar]_{batch,stream}_dev).

One function checks a windowed call for all of them (window_call_checks, host_stages.hip); which code a call with two faults
returns is part of the C ABI: a null or misaligned pointer and buffers that overlap without being the same are ERR_ARG and are
decided before a handle of more than 8191 channels is ERR_UNSUPPORTED, and a stream entry looks at its state first.  No call here
launches anything."""
import ctypes as C

import pytest

from devframe import ERR_ARG, ERR_UNSUPPORTED

BPS = 2  # (a native sample is not a planar one: 2 and 4 bytes)
ENTRIES = [(stage, planar, carried) for stage in ("fir_prefilter", "median_filter") for planar in (False, True) for carried in (False, True)]


def _name(stage, planar, carried):
    return "rspt_hip_%s_%s%s_dev" % (stage, "planar_" if planar else "", "stream" if carried else "batch")


@pytest.mark.gpu
def test_gpu_every_window_entry_decides_its_refusals_in_one_order():
    import torch

    from rspt_amd import api

    L = api.lib()
    assert L.rspt_hip_device_count() > 0, "no gfx950 device visible"
    assert len({_name(*e) for e in ENTRIES}) == 8 and all(hasattr(L, _name(*e)) for e in ENTRIES)
    st = torch.cuda.current_stream().cuda_stream
    taps = (C.c_double * 3)(0.25, 0.5, 0.25)
    small, wide = api.new_hzr(BPS, 2, 16), api.new_hzr(BPS, 8192, 4)
    state = torch.zeros(8 + 2 * 8192 * 4 + 8, dtype=torch.uint8, device="cuda")  # (K - 1 = 2 rows of either handle, either layout)
    assert state.data_ptr() % 8 == 0
    seen = 0
    for pk, too_wide in ((small, False), (wide, True)):
        nch, ns = pk.nch, pk.ns
        for stage, planar, carried in ENTRIES:
            sample = 4 if planar else BPS
            n = nch * ns * sample  # bytes of the call's one block
            buf = torch.full((3 * n + 16,), 0x5A, dtype=torch.uint8, device="cuda")
            base = buf.data_ptr()
            assert base % 16 == 0
            fn = getattr(L, _name(stage, planar, carried))

            def call(s=base, d=base + 2 * n, state_ptr=state.data_ptr()):
                a = [pk._h, s, d, 1] + ([taps, 3] if stage == "fir_prefilter" else [3])
                return fn(*(a + ([state_ptr] if carried else []) + [st]))

            what = (_name(stage, planar, carried), nch, ns)
            # apart (n bytes between the buffers), and in place: the only fault left is the handle's width
            if too_wide:
                assert call() == ERR_UNSUPPORTED and call(d=base) == ERR_UNSUPPORTED, what
            # a null buffer
            assert call(s=None) == ERR_ARG and call(d=None) == ERR_ARG, what
            # a planar pointer off its 4-byte alignment, either buffer or both (in place)
            if planar:
                assert call(s=base + 2) == ERR_ARG and call(d=base + 2 * n + 2) == ERR_ARG and call(s=base + 2, d=base + 2) == ERR_ARG, what
            # overlapping by one sample, the destination behind the source and in front of it: before "too wide"
            assert call(d=base + n - sample) == ERR_ARG and call(s=base + n - sample, d=base) == ERR_ARG, what
            # a stream entry looks at its state before anything else
            if carried:
                assert call(state_ptr=None) == ERR_ARG and call(state_ptr=state.data_ptr() + 4) == ERR_ARG, what
                assert call(d=base + n - sample, state_ptr=None) == ERR_ARG, what
            torch.cuda.synchronize()
            assert int((buf != 0x5A).count_nonzero()) == 0 and int(state.count_nonzero()) == 0, what  # nothing was launched
            seen += 1
    assert seen == 16
    small.close()
    wide.close()
