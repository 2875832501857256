"""The IIR cascade stage: 1 to 4 reference i_filter::new_iir objects per channel chained in double and
truncated once, on the GPU: rspt_hip_iir_cascade_batch_dev, rspt_hip_iir_cascade_stream_dev.

CPU: the record's inputs, the numpy restatement (tests/iir_cascade_cases.py) against the reference's answers
(tests/golden/iir_cascade_record.json), what the record covers, the C ABI, the device ISA of the new kernels, and the argument
checks that need no device.
GPU (-m gpu): every case bit-exact against the record and the restatement, stateless and as a stream however the recording is
cut into calls, the equivalence of one section with the IIR pre-filter stage (states included), that the state is used, and
the statuses.

These are hand-picked cases, and their streams are cut at whole blocks in three patterns.  Every residue of a run's and of a
call's length mod the pipelined kernel's chunk, every (order, producer part, place of the last sample), cuts at any row and the
contents of the carried state are covered by the seeded sweep, tests/test_iir_sweep.py (legs cascade and cascade_stream of
tests/iir_sweep_cases.py)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import devframe as df
import iir_cascade_cases as cc
import iir_cases as ic
from cases import digest
from devframe import ERR_ARG, ERR_UNSUPPORTED, api, asm  # noqa: F401

ENTRIES = ("rspt_hip_iir_cascade_batch_dev", "rspt_hip_iir_cascade_state_bytes", "rspt_hip_iir_cascade_stream_dev")
CHUNK = cc.CHUNK

CASES = cc.cascade_cases()
NAMES = [c["name"] for c in CASES]
FORMS = ("stateless", "stream")


@functools.lru_cache(maxsize=None)
def _record():
    return df.golden("iir_cascade_record.json")


@functools.lru_cache(maxsize=None)
def _case(name):
    """the case with the record's exact coefficients"""
    i = NAMES.index(name)
    r = _record()["cases"][i]
    assert r["name"] == name
    return cc.with_record_coefficients(CASES[i], r)


@functools.lru_cache(maxsize=None)
def _want(name, form):
    """the restatement's answer, computed once per process (read-only)"""
    y = cc.filtered(_case(name), form)
    y.setflags(write=False)
    return y


# ---- CPU ----

def test_record_inputs_have_not_drifted():
    rec = _record()["cases"]
    assert len(CASES) == len(rec)
    for c, r in zip(CASES, rec):
        assert (c["name"], c["bps"], c["nch"], c["ns"], c["nblocks"]) == (r["name"], r["bps"], r["nch"], r["ns"], r["nblocks"])
        assert cc.crc(c["data"]) == r["in_crc32"], c["name"]
        assert cc.sections_to_record(c) == r["sections"], c["name"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(name):
    c = _case(name)
    for form in FORMS:
        y = _want(name, form)
        assert digest(y) == c["rec"][form]["digest"] and cc.crc(y) == c["rec"][form]["crc32"], form


def test_the_record_covers_what_it_must():
    rec = _record()["cases"]
    assert {r["ns"] for r in rec} >= {1, 5, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7}
    assert {r["nch"] for r in rec} >= {1, 3, 64, 65, 130}
    assert {r["bps"] for r in rec} == {1, 2, 3, 4}
    assert {r["nblocks"] for r in rec} >= set(range(1, 8))
    assert {len(r["sections"]) for r in rec} == {1, 2, 3, 4}
    ncs = {tuple(len(s["n"]) for s in r["sections"]) for r in rec}
    assert (2, 5, 3, 4) in ncs and (5, 5) in ncs
    inits = {tuple(s["init"] for s in r["sections"]) for r in rec}
    assert any(i[0] == 2000 and set(i[1:]) == {0} for i in inits if len(i) > 1)  # (2000, 0, ...)
    zero = [r for r in rec if not any(s["init"] for s in r["sections"])]
    assert any(r["ns"] < CHUNK for r in zero) and any(r["ns"] >= CHUNK for r in zero)  # init = 0 throughout, both kernels
    modes = [{s["use_filter"] for s in r["sections"]} for r in rec if len(r["sections"]) > 1]
    assert {0} in modes and {1} in modes and {0, 1} in modes  # all filter_opt, all filter, mixed
    pair = [{"n": ic.to_bits(n), "d": ic.to_bits(d), "init": init, "use_filter": int(f)} for n, d, init, f in cc.README_PAIR]
    readme = [r for r in rec if r["sections"] == pair]
    assert {(r["bps"], r["nch"], r["ns"], r["nblocks"]) for r in readme} == {(4, 12, 2048, 16), (3, 3, 1000, 20)}
    assert pair[0]["n"] == ic.to_bits([1.0, -1.99822284729, 0.99822442503]) and pair[1]["d"] == ic.to_bits([0.02008336556, 0.04016673113, 0.02008336556])
    for r in rec:  # a stream's uneven cut holds a call shorter than a chunk beside longer ones somewhere
        if r["ns"] < CHUNK and any(k * r["ns"] >= CHUNK for k in cc.splits(r)["uneven"]):
            break
    else:
        raise AssertionError("no case cuts a stream into calls below and above a chunk")


@pytest.mark.parametrize("name", ["unstable3x500x7_i32_into_lp100", "unstable2x20x7_i8_into_nc4_small_calls"])
def test_the_unstable_section_feeds_its_nan_into_the_stable_one_across_a_block_edge(name):
    """section 0's output passes 2^31, becomes inf and NaN inside one block; section 1 takes it in untruncated, and the whole of
    the next block is NaN: the NaN is in the stable section's rings"""
    c = _case(name)
    _, per = cc.stream_double(c)
    first, last = per[0][:, 1], per[-1][:, 1]
    past = np.isfinite(first) & (np.abs(first) >= 2.0 ** 31)
    assert past.any() and np.isinf(first).any() and np.isnan(first).any()
    nan0 = int(np.argmax(np.isnan(first)))
    assert int(np.argmax(past)) < int(np.argmax(np.isinf(first))) < nan0
    assert (np.isfinite(last) & (np.abs(last) >= 2.0 ** 31)).any()  # the stable section passes on what no int32 holds
    nan1 = int(np.argmax(np.isnan(last)))
    assert np.isnan(last[nan1:]).all() and nan1 >= int(np.argmax(np.isinf(first)))
    assert 0 < nan1 % c["ns"] and nan1 // c["ns"] + 1 < c["nblocks"]  # inside a block, and a block follows
    assert np.isfinite(per[-1][:, 0]).all()  # the channel that is never fed stays finite


@pytest.mark.parametrize("name", cc.README_NAMES)
def test_the_chain_is_not_two_truncating_passes(name):
    """condition 1: on the README pair the chain differs from two successive calls of the single-section stage"""
    c = _case(name)
    chained, twice = _want(name, "stream"), cc.two_truncating_passes(c)
    assert chained.shape == twice.shape and not np.array_equal(chained, twice)


def test_filter_and_filter_opt_round_differently():
    """condition 2: the same data and coefficients through filter() and through filter_opt()"""
    a, b = _case("ns103_i32_3ch_x2_s2_nc53_all_opt"), _case("ns103_i32_3ch_x2_s2_nc53_all_filter")
    assert np.array_equal(a["data"], b["data"])
    assert [s[:3] for s in a["sections"]] == [s[:3] for s in b["sections"]]
    assert not np.array_equal(_want(a["name"], "stateless"), _want(b["name"], "stateless"))


def test_header_declares_the_entries_and_the_library_exports_them():
    df.check_entries((
        "int rspt_hip_iir_cascade_batch_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, size_t nsections, const double* n, const double* d, "
        "const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* stream);",
        "int rspt_hip_iir_cascade_state_bytes(rspt_hip_packer* p, size_t nsections, size_t* bytes);",
        "int rspt_hip_iir_cascade_stream_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, size_t nsections, const double* n, const double* d, "
        "const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, void* d_state, void* stream);",
    ), ENTRIES)


def test_the_cascade_kernels_hold_no_fused_multiply_add(asm):
    """k_iir_cascade (sample width x carried) and k_iir_cascade_pipe ((int8, int16 (+aligned), int24, int32 (+aligned)) x carried)"""
    plain = [n for n in asm if re.search(r"13k_iir_cascadeIL", n)]
    pipe = [n for n in asm if re.search(r"18k_iir_cascade_pipeIL", n)]
    assert len(plain) == 8, sorted(plain)
    assert len(pipe) == 12, sorted(pipe)
    for n in plain + pipe:
        assert not [ln for ln in asm[n] if df.FUSED_F64_F32.match(ln)], n


def test_argument_checks_that_need_no_device():
    """a NULL handle, a NULL `bytes` and a section count outside 1..4 are refused before anything touches a device"""
    from rspt_amd import api

    L = api.lib()
    n = C.c_size_t(12345)
    assert L.rspt_hip_iir_cascade_state_bytes(None, 2, C.byref(n)) == ERR_ARG and n.value == 12345
    k = (C.c_double * 10)(*([1.0, 0.5, 0.25, 0.0, 0.0] * 2))
    nc, init = (C.c_uint32 * 2)(3, 3), (C.c_int32 * 2)(0, 0)
    state = C.create_string_buffer(4096)
    sp = C.addressof(state) & ~7
    assert L.rspt_hip_iir_cascade_batch_dev(None, sp, 1, 2, k, k, nc, init, None, None) == ERR_ARG
    assert L.rspt_hip_iir_cascade_stream_dev(None, sp, 1, 2, k, k, nc, init, None, sp, None) == ERR_ARG


# ---- GPU ----

def _drive(pk, sections, data, split, state):
    """the recording through successive calls of split[i] blocks each (state None: stateless calls); -> the filtered bytes"""
    import torch

    buf = torch.from_numpy(np.array(data, dtype=np.uint8)).cuda()
    bb, b0 = pk.block_bytes, 0
    for k in split:
        pk.iir_cascade_batch(buf[b0 * bb : (b0 + k) * bb], sections, state=state)
        b0 += k
    assert b0 * bb == buf.numel()
    torch.cuda.synchronize()
    return buf.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_stateless_bit_exact(api, name):
    c = _case(name)
    want = _want(name, "stateless")
    assert digest(want) == c["rec"]["stateless"]["digest"]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    for split in ([c["nblocks"]], [1] * c["nblocks"]):  # every block a fresh chain, in one call or in many
        got = _drive(pk, c["sections"], c["data"], split, None)
        assert np.array_equal(got, want) and digest(got) == c["rec"]["stateless"]["digest"], split
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_stream_bit_exact_however_the_recording_is_cut(api, name):
    c = _case(name)
    want = _want(name, "stream")
    assert digest(want) == c["rec"]["stream"]["digest"]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    for how, split in cc.splits(c).items():
        got = _drive(pk, c["sections"], c["data"], split, pk.iir_cascade_state(len(c["sections"])))
        assert np.array_equal(got, want) and digest(got) == c["rec"]["stream"]["digest"], how
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ns103_i32_3ch_x2_s4_nc2534_mixed_modes", "ns33_i24_3ch_x7_s2_init0", "ns5_i16_65ch_x6_s3_mixed_modes"])
def test_gpu_base_address_off_the_sample_width(api, name):
    """the byte-wise instantiations: the recording one byte off any 2- or 4-byte boundary"""
    import torch

    c = _case(name)
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    n = c["data"].size
    for form in FORMS:
        raw = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        buf = raw[1 : 1 + n]
        buf.copy_(torch.from_numpy(np.array(c["data"])))
        assert buf.data_ptr() % 2 == 1
        pk.iir_cascade_batch(buf, c["sections"], state=pk.iir_cascade_state(len(c["sections"])) if form == "stream" else None)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), _want(name, form)), form
        assert int(raw[0]) == 0 and int(raw[1 + n :].count_nonzero()) == 0
    pk.close()


S1 = ["ns33_i16_130ch_x3_s1", "ns103_i32_3ch_x2_s1_nc2", "ns96_i32_3ch_x2_s1_nc4_init0"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", S1)
def test_gpu_one_section_equals_the_iir_prefilter_stage(api, name):
    """S = 1 through filter_opt: iir_prefilter_batch(per_channel=True) and iir_prefilter_batch(state=...) byte for byte"""
    import torch

    c = _case(name)
    (n, d, init, f), = c["sections"]
    assert not f
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    for form in FORMS:
        old = torch.from_numpy(np.array(c["data"])).cuda()
        pk.iir_prefilter_batch(old, n, d, init_nr_samples=init, per_channel=True, state=pk.iir_state() if form == "stream" else None)
        new = _drive(pk, c["sections"], c["data"], [c["nblocks"]], pk.iir_cascade_state(1) if form == "stream" else None)
        torch.cuda.synchronize()
        assert np.array_equal(old.cpu().numpy(), new), form
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", S1)
def test_gpu_a_one_section_state_moves_between_the_two_entries(api, name):
    import torch

    c = _case(name)
    (n, d, init, _), = c["sections"]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    assert pk.iir_cascade_state_bytes(1) == pk.iir_state_bytes()
    bb = pk.block_bytes
    want = _want(name, "stream")
    for first in ("cascade", "prefilter"):
        state = pk.iir_state()
        buf = torch.from_numpy(np.array(c["data"])).cuda()
        for b in range(c["nblocks"]):
            piece = buf[b * bb : (b + 1) * bb]
            if (b % 2 == 0) == (first == "cascade"):
                pk.iir_cascade_batch(piece, c["sections"], state=state)
            else:
                pk.iir_prefilter_batch(piece, n, d, init_nr_samples=init, per_channel=True, state=state)
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), want), first
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ns103_i32_3ch_x2_s4_nc2534_mixed_modes", "ns16_i32_3ch_x7_s2_plain_pipe_plain"])
def test_gpu_two_states_in_turn_on_one_handle(api, name):
    """two recordings of one shape, their blocks alternating on one handle and one stream, each with its own state"""
    import torch

    c = _case(name)
    S = len(c["sections"])
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    other = dict(c, data=cc.cases._rand_native(c["nch"], c["ns"] * c["nblocks"], c["bps"], 4242, 1 << (8 * c["bps"] - 3)))
    bufs = [torch.from_numpy(np.array(x["data"])).cuda() for x in (c, other)]
    states = [pk.iir_cascade_state(S), pk.iir_cascade_state(S)]
    bb = pk.block_bytes
    for b in range(c["nblocks"]):
        for buf, st in zip(bufs, states):
            pk.iir_cascade_batch(buf[b * bb : (b + 1) * bb], c["sections"], state=st)
    torch.cuda.synchronize()
    assert np.array_equal(bufs[0].cpu().numpy(), _want(name, "stream"))
    assert np.array_equal(bufs[1].cpu().numpy(), cc.filtered(other, "stream"))
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["readme_ds3x1000x20_i24_hp04_lp100", "ns16_i32_3ch_x7_s2_plain_pipe_plain"])
def test_gpu_the_state_is_used_and_zeroing_it_starts_afresh(api, name):
    c = _case(name)
    S = len(c["sections"])
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    bb = pk.block_bytes
    first, second = c["data"][: 2 * bb], c["data"][2 * bb : 4 * bb]
    state = pk.iir_cascade_state(S)
    assert state.numel() == 88 * c["nch"] * S and state.data_ptr() % 8 == 0 and int(state.count_nonzero()) == 0
    a = _drive(pk, c["sections"], first, [2], state)
    started = state.cpu().numpy().view(np.uint64).reshape(c["nch"], S, 11)[:, :, 10]
    assert (started == 1).all()  # a call writes all S of them
    carried = _drive(pk, c["sections"], second, [2], state)  # continues the recording
    fresh = _drive(pk, c["sections"], second, [2], pk.iir_cascade_state(S))  # a new recording that starts with the same rows
    assert np.array_equal(np.concatenate([a, carried]), _want(name, "stream")[: 4 * bb])
    assert np.array_equal(fresh, cc.filtered(dict(c, nblocks=2, data=second), "stream"))
    assert not np.array_equal(carried, fresh)
    state.zero_()
    assert np.array_equal(_drive(pk, c["sections"], second, [2], state), fresh)
    pk.close()


@pytest.mark.gpu
def test_gpu_entries_reject_bad_arguments(api):
    import torch

    L = api.lib()
    pk = api.new_hzr(4, 3, 100)
    bb = pk.block_bytes
    buf = torch.zeros(2 * bb, dtype=torch.uint8, device="cuda")
    h, st = pk._h, torch.cuda.current_stream().cuda_stream
    state = torch.zeros(pk.iir_cascade_state_bytes(4) + 8, dtype=torch.uint8, device="cuda")
    nb = C.c_size_t()
    assert L.rspt_hip_iir_cascade_state_bytes(h, 2, None) == ERR_ARG
    assert L.rspt_hip_iir_cascade_state_bytes(h, 0, C.byref(nb)) == ERR_ARG and L.rspt_hip_iir_cascade_state_bytes(h, 5, C.byref(nb)) == ERR_ARG
    assert [pk.iir_cascade_state_bytes(s) for s in (1, 2, 3, 4)] == [88 * 3 * s for s in (1, 2, 3, 4)]
    NULL = object()

    def call(S=2, nc=(3, 3, 3, 3), init=(2, 0, 0, 0), nblocks=2, p=buf.data_ptr(), state_ptr=None, stream_form=False, n=None, d=None, ncp=None, initp=None):
        coef = np.tile(np.array([1.0, -0.5, 0.1, 0.0, 0.0]), 4)
        ncs, inits = np.array(nc, dtype=np.uint32), np.array(init, dtype=np.int32)
        a = [h, p, nblocks, S, None if n is NULL else coef.ctypes.data_as(C.POINTER(C.c_double)),
             None if d is NULL else coef.ctypes.data_as(C.POINTER(C.c_double)), None if ncp is NULL else ncs.ctypes.data_as(C.POINTER(C.c_uint32)),
             None if initp is NULL else inits.ctypes.data_as(C.POINTER(C.c_int32)), None]
        if stream_form:
            return L.rspt_hip_iir_cascade_stream_dev(*a, state_ptr, st)
        return L.rspt_hip_iir_cascade_batch_dev(*a, st)

    for sf, sp in ((False, None), (True, state.data_ptr())):
        kw = dict(stream_form=sf, state_ptr=sp)
        assert call(S=0, **kw) == ERR_ARG and call(S=5, **kw) == ERR_ARG
        assert call(nc=(3, 1, 3, 3), **kw) == ERR_ARG and call(nc=(6, 3, 3, 3), **kw) == ERR_ARG
        assert call(init=(0, -1, 0, 0), **kw) == ERR_ARG and call(init=((1 << 28) + 1, 0, 0, 0), **kw) == ERR_ARG
        assert call(n=NULL, **kw) == ERR_ARG and call(d=NULL, **kw) == ERR_ARG and call(ncp=NULL, **kw) == ERR_ARG and call(initp=NULL, **kw) == ERR_ARG
        assert call(p=None, **kw) == ERR_ARG and call(nblocks=0, **kw) == ERR_ARG
        assert call(nblocks=(1 << 31) // 3 + 1, **kw) == ERR_ARG  # nblocks * nch >= 2^31
    assert call(stream_form=True, state_ptr=None) == ERR_ARG and call(stream_form=True, state_ptr=state.data_ptr() + 4) == ERR_ARG
    # a stream call of 2^31 - 2^17 rows and more: refused before anything is launched (no such buffer exists here)
    assert call(stream_form=True, state_ptr=state.data_ptr(), nblocks=((1 << 31) - (1 << 17)) // 100 + 1) == ERR_UNSUPPORTED
    wide = api.new_hzr(1, 8192, 4)  # more than 8191 channels
    wbuf = torch.zeros(wide.block_bytes, dtype=torch.uint8, device="cuda")
    wstate = torch.zeros(88 * 8192 * 2, dtype=torch.uint8, device="cuda")
    coef = np.tile(np.array([1.0, -0.5, 0.1, 0.0, 0.0]), 2)
    cp = coef.ctypes.data_as(C.POINTER(C.c_double))
    ncs, inits = (C.c_uint32 * 2)(3, 3), (C.c_int32 * 2)(1, 0)
    assert L.rspt_hip_iir_cascade_batch_dev(wide._h, wbuf.data_ptr(), 1, 2, cp, cp, ncs, inits, None, st) == ERR_UNSUPPORTED
    assert L.rspt_hip_iir_cascade_stream_dev(wide._h, wbuf.data_ptr(), 1, 2, cp, cp, ncs, inits, None, wstate.data_ptr(), st) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.count_nonzero()) == 0 and int(state.count_nonzero()) == 0 and int(wstate.count_nonzero()) == 0  # nothing ran
    wide.close()
    # accepted: the extremes
    assert call(S=1, nc=(2, 3, 3, 3)) == 0 and call(S=4, nc=(5, 5, 5, 5), init=(0, 0, 0, 0)) == 0
    assert call(S=4, nc=(5, 2, 5, 2), stream_form=True, state_ptr=state.data_ptr()) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        pk.iir_cascade_batch(buf, [])
    with pytest.raises(ValueError):
        pk.iir_cascade_batch(buf, [([1.0], [1.0])])
    pk.close()
