"""The IIR and FIR pre-filters with a carried state: one reference i_filter per channel over a recording
that arrives in blocks, on the GPU: rspt_hip_iir_prefilter_stream_dev, rspt_hip_fir_prefilter_stream_dev.

CPU: the record's inputs, the numpy restatement (tests/stream_filter_cases.py) against the reference's answers
(tests/golden/stream_filter_record.json), what the record covers, the C ABI, the device ISA of the new kernels, and the
argument checks that need no device.
GPU (-m gpu): every case bit-exact against the record and the restatement however the recording is cut into calls, the
equivalence with the stateless stages, that the state is used, and the statuses."""
import ctypes as C
import re

import numpy as np
import pytest

import devframe as df
import fir_cases as fc
import iir_cases as ic
import stream_filter_cases as sc
from cases import IIR_BANDPASS, digest
from devframe import ERR_ARG, ERR_UNSUPPORTED, api, asm  # noqa: F401

ENTRIES = ("rspt_hip_iir_state_bytes", "rspt_hip_iir_prefilter_stream_dev", "rspt_hip_fir_state_bytes", "rspt_hip_fir_prefilter_stream_dev")


@pytest.fixture(scope="module")
def record():
    return df.golden("stream_filter_record.json")


@pytest.fixture(scope="module")
def scases(record):
    out = {}
    for c, r in zip(sc.stream_cases(), record["cases"]):
        assert c["name"] == r["name"]
        out[c["name"]] = sc.with_record_coefficients(c, r)
    return out


CASES = sc.stream_cases()
NAMES = [c["name"] for c in CASES]


# ---- CPU ----

def test_record_inputs_have_not_drifted(record):
    assert len(CASES) == len(record["cases"])
    for c, r in zip(CASES, record["cases"]):
        assert (c["name"], c["kind"], c["bps"], c["nch"], c["ns"], c["nblocks"]) == (r["name"], r["kind"], r["bps"], r["nch"], r["ns"], r["nblocks"])
        assert fc.crc(c["data"]) == r["in_crc32"], c["name"]
        if c["kind"] == "fir":
            assert np.array_equal(np.asarray(c["kernel"]), fc.kernel_from_record(r["kernel"])), c["name"]
        else:
            assert ic.to_bits(c["n"]) == r["n"] and ic.to_bits(c["d"]) == r["d"] and c["init"] == r["init"], c["name"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(scases, name):
    c = scases[name]
    y = sc.filtered(c)
    assert digest(y) == c["rec"]["digest"] and fc.crc(y) == c["rec"]["crc32"]


def test_the_record_covers_what_it_must(record):
    iir = [r for r in record["cases"] if r["kind"] == "iir"]
    fir = [r for r in record["cases"] if r["kind"] == "fir"]
    for group in (iir, fir):
        assert {r["bps"] for r in group} == {1, 2, 3, 4}
        assert any(r["nch"] == 1 for r in group)
        assert any(r["ns"] < 64 for r in group) and any(r["ns"] > 64 and r["ns"] % 64 for r in group)
    assert {(len(r["n"]), r["init"]) for r in iir} >= {(nc, init) for nc in (2, 3, 4, 5) for init in (0, 2000)}
    harness = [r for r in iir if r["n"] == ic.to_bits(IIR_BANDPASS[0]) and r["d"] == ic.to_bits(IIR_BANDPASS[1])]  # rspt_test.cpp:124-125
    assert harness and harness[0]["init"] == 2000
    assert any((r["nch"], r["ns"], r["nblocks"]) == (12, 2048, 16) for r in iir + fir)  # the ECG recording
    assert any((r["nch"], r["ns"], r["nblocks"], r["bps"]) == (3, 1000, 20, 3) for r in iir + fir)  # the 24-bit recording
    ks = {len(fc.kernel_from_record(r["kernel"])): r for r in fir}
    assert {1, 2, 31, 101, 1001, 4097, 65536} <= set(ks)
    assert ks[4097]["ns"] == 700  # K - 1 > ns
    r = ks[65536]
    assert (r["nch"], r["ns"]) == (2, 40) and 65535 > r["ns"] * r["nblocks"]  # K - 1 larger than a whole call, however it is cut
    assert any(not np.all(np.isfinite(fc.kernel_from_record(r["kernel"])) & (np.abs(fc.kernel_from_record(r["kernel"])) < 1e300)) for r in fir)


@pytest.mark.parametrize("name", ["iir_unstable3x500x7_i32_nan_carried", "iir_unstable2x40x6_i8_nan_carried_small_calls"])
def test_the_unstable_case_carries_its_nan_over_a_block_edge(scases, name):
    """the output passes 2^31, becomes NaN inside one block, and the whole of the next block is NaN: the NaN is in the rings"""
    c = scases[name]
    rows = c["ns"] * c["nblocks"]
    y = sc.iir_stream_double(c["data"], c["bps"], c["nch"], rows, c["n"], c["d"], c["init"])[:, 1]
    past = np.isfinite(y) & (np.abs(y) >= 2.0 ** 31)
    assert past.any()
    first_nan = int(np.argmax(np.isnan(y)))
    assert np.isnan(y).any() and first_nan > int(np.argmax(past))
    blk = first_nan // c["ns"]
    assert 0 < first_nan % c["ns"] and blk + 1 < c["nblocks"]  # inside a block, and a block follows
    assert np.isnan(y[first_nan:]).all()


def test_fir_nan_case_holds_overflow_and_nan(scases):
    c = scases["fir_rand4x250x8_i32_inf_nan"]
    y = fc.fir_i32(fc.native_to_i32(c["data"], 4, 4, 2000), c["kernel"])
    assert np.isnan(y).sum() > 100


def test_header_declares_the_entries_and_the_library_exports_them():
    df.check_entries((
        "int rspt_hip_iir_state_bytes(rspt_hip_packer* p, size_t* bytes);",
        "int rspt_hip_iir_prefilter_stream_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, "
        "size_t nr_coefficients, int init_nr_samples, void* d_state, void* stream);",
        "int rspt_hip_fir_state_bytes(rspt_hip_packer* p, size_t kernel_size, size_t* bytes);",
        "int rspt_hip_fir_prefilter_stream_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, const double* kernel, "
        "size_t kernel_size, void* d_state, void* stream);",
    ), ENTRIES)


def test_the_stateless_entries_keep_their_signatures():
    hdr = df.header()
    assert ("int rspt_hip_iir_prefilter_batch_dev(rspt_hip_packer* p, void* d_buf, size_t nblocks, const double* n, const double* d, "
            "size_t nr_coefficients, int init_nr_samples, int per_channel, void* stream);") in hdr
    assert ("int rspt_hip_fir_prefilter_batch_dev(rspt_hip_packer* p, const void* d_src, void* d_dst, size_t nblocks, const double* kernel, "
            "size_t kernel_size, void* stream);") in hdr


def test_the_new_filter_kernels_round_every_product_and_sum_on_their_own(asm):
    """k_iir_carry (calls of fewer than 64 rows) and the CARRY instantiations of k_iir_pipe (a fifth template argument `true`): no
    fp FMA, no f64 MFMA, and separate v_mul_f64 / v_add_f64; k_fir is the stateless stage's kernel with one more pointer, held
    to the same by tests/test_fir_prefilter.py -- here: still six instantiations, and the byte movers hold no fp arithmetic"""
    df.rounds_separately(asm, r"k_iir_carry", 16)  # sample width x order
    df.rounds_separately(asm, r"10k_iir_pipeILi\dELi\dELb0ELb[01]ELb1EE", 24)  # (int8, int16 (+aligned), int24, int32 (+aligned)) x order
    assert len([n for n in asm if re.search(r"5k_firIL", n)]) == 6
    movers = [n for n in asm if "k_fir_carry" in n]
    assert len(movers) == 2, movers
    for n in movers:
        assert not [ln for ln in asm[n] if re.match(r"^\s+v_\w+_f64\b", ln) or df.FUSED_F64_F32.match(ln)], n


def test_argument_checks_that_need_no_device():
    """a NULL handle and a NULL `bytes` are refused before anything touches a device"""
    from rspt_amd import api

    L = api.lib()
    n = C.c_size_t(12345)
    assert L.rspt_hip_iir_state_bytes(None, C.byref(n)) == ERR_ARG and n.value == 12345
    assert L.rspt_hip_fir_state_bytes(None, 5, C.byref(n)) == ERR_ARG and n.value == 12345
    k = (C.c_double * 3)(1.0, 2.0, 3.0)
    state = C.create_string_buffer(4096)
    sp = C.addressof(state) & ~7
    assert L.rspt_hip_iir_prefilter_stream_dev(None, sp, 1, k, k, 3, 0, sp, None) == ERR_ARG
    assert L.rspt_hip_fir_prefilter_stream_dev(None, sp, sp, 1, k, 3, sp, None) == ERR_ARG


# ---- GPU ----

def _state(pk, c):
    return pk.fir_state(len(c["kernel"])) if c["kind"] == "fir" else pk.iir_state()


def _call(pk, c, buf, state, dst=None):
    """one call of the case's filter on the whole blocks in buf"""
    if c["kind"] == "fir":
        return pk.fir_prefilter_batch(buf, c["kernel"], d_dst=dst, state=state)
    assert dst is None
    return pk.iir_prefilter_batch(buf, c["n"], c["d"], init_nr_samples=c["init"], per_channel=True, state=state)


def _drive(pk, c, data, split, state, out_of_place=False):
    """the recording through successive calls of split[i] blocks each; -> (filtered recording, source afterwards) as bytes"""
    import torch

    src = torch.from_numpy(np.asarray(data, dtype=np.uint8)).cuda()
    dst = torch.full_like(src, 0xA5) if out_of_place else None
    bb, b0 = pk.block_bytes, 0
    for k in split:
        lo, hi = b0 * bb, (b0 + k) * bb
        _call(pk, c, src[lo:hi], state, None if dst is None else dst[lo:hi])
        b0 += k
    assert b0 * bb == src.numel()
    torch.cuda.synchronize()
    return (dst if out_of_place else src).cpu().numpy(), src.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_stream_bit_exact_however_the_recording_is_cut(api, scases, name):
    c = scases[name]
    want = sc.filtered(c)
    assert digest(want) == c["rec"]["digest"]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    for how, split in sc.splits(c["nblocks"]).items():
        for oop in ((False, True) if c["kind"] == "fir" else (False,)):
            got, src_after = _drive(pk, c, c["data"], split, _state(pk, c), out_of_place=oop)
            assert digest(got) == c["rec"]["digest"] and np.array_equal(got, want), (how, "out of place" if oop else "in place")
            if oop:
                assert np.array_equal(src_after, c["data"]), (how, "out of place wrote d_src")
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["iir_ecg12x2048x16_i32_harness_bandpass", "iir_nc3_init0_i16_5x100x6", "iir_nc2_init2000_i8_1x40x8",
                                  "iir_nc4_init0_i24_3x64x5", "fir_ecg12x2048x16_i32_lowpass1001", "fir_rand3x700x4_i24_k4097",
                                  "fir_rand7x143x7_i8_k2", "fir_ds3x1000x20_i24_k1_gain"])
def test_gpu_stream_on_a_zeroed_state_equals_the_stateless_stage_on_one_long_block(api, scases, name):
    """B blocks of ns behind a zeroed state = the stateless per-channel IIR / stateless FIR on a handle of shape (bps, nch, B * ns)"""
    import torch

    c = scases[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    got, _ = _drive(pk, c, c["data"], [c["nblocks"]], _state(pk, c))
    pk.close()
    one = api.new_hzr(c["bps"], c["nch"], c["ns"] * c["nblocks"])
    buf = torch.from_numpy(c["data"]).cuda()
    _call(one, c, buf, None)
    torch.cuda.synchronize()
    assert np.array_equal(got, buf.cpu().numpy())
    one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["iir", "fir"])
def test_gpu_stream_equals_the_stateless_stage_at_full_size(api, kind):
    """64 ch x 65536 int32 as 16 blocks of 4096: in one call, and block by block"""
    import torch

    B = sc.BIG
    data = sc.big_data()
    if kind == "iir":
        c = dict(kind="iir", n=IIR_BANDPASS[0], d=IIR_BANDPASS[1], init=2000)
    else:
        c = dict(kind="fir", kernel=fc.big_kernel())
    one = api.new_hzr(B["bps"], B["nch"], B["ns"] * B["nblocks"])
    ref = torch.from_numpy(data).cuda()
    _call(one, c, ref, None)
    torch.cuda.synchronize()
    want = ref.cpu().numpy()
    one.close()
    pk = api.new_hzr(B["bps"], B["nch"], B["ns"])
    for split in ([B["nblocks"]], [1] * B["nblocks"]):
        got, _ = _drive(pk, c, data, split, _state(pk, c))
        assert np.array_equal(got, want), len(split)
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["iir_ds3x1000x20_i24_highpass", "fir_synth5x300x10_i16_lowpass31"])
def test_gpu_the_state_is_used_and_zeroing_it_starts_afresh(api, scases, name):
    import torch

    c = scases[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    bb = pk.block_bytes
    first, second = c["data"][: 2 * bb], c["data"][2 * bb : 4 * bb]
    state = _state(pk, c)
    assert int(state.count_nonzero()) == 0
    a, _ = _drive(pk, c, first, [2], state)
    assert int(state.count_nonzero()) > 0
    carried, _ = _drive(pk, c, second, [2], state)  # continues the recording
    fresh, _ = _drive(pk, c, second, [2], _state(pk, c))  # a new recording that starts with the same rows
    want = sc.filtered(dict(c, nblocks=4, data=c["data"][: 4 * bb]))
    assert np.array_equal(np.concatenate([a, carried]), want)
    assert np.array_equal(fresh, sc.filtered(dict(c, nblocks=2, data=second)))
    assert not np.array_equal(carried, fresh)
    state.zero_()
    again, _ = _drive(pk, c, second, [2], state)
    assert np.array_equal(again, fresh)
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["iir_nc5_init2000_i32_7x232x4", "fir_rand1x500x10_i32_bandpass101"])
def test_gpu_two_states_interleaved_on_one_handle(api, scases, name):
    """two recordings of one shape, their blocks alternating on one handle and one stream, each with its own state"""
    import torch

    c = scases[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    rows = c["ns"] * c["nblocks"]
    other = dict(c, data=fc.cases._rand_native(c["nch"], rows, c["bps"], 4242, 1 << (8 * c["bps"] - 3)))
    bufs = [torch.from_numpy(x["data"]).cuda() for x in (c, other)]
    states = [_state(pk, c), _state(pk, c)]
    bb = pk.block_bytes
    for b in range(c["nblocks"]):
        for buf, st in zip(bufs, states):
            _call(pk, c, buf[b * bb : (b + 1) * bb], st)
    torch.cuda.synchronize()
    assert np.array_equal(bufs[0].cpu().numpy(), sc.filtered(c))
    assert np.array_equal(bufs[1].cpu().numpy(), sc.filtered(other))
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["iir_nc5_init0_i32_7x232x4", "iir_nc3_init2000_i16_5x100x6", "iir_nc5_init0_i32_1x50x9_below_a_chunk",
                                  "fir_rand1x500x10_i32_bandpass101", "fir_synth5x300x10_i16_lowpass31"])
def test_gpu_stream_base_address_off_the_sample_width(api, scases, name):
    """the byte-wise instantiations: the recording one byte off any 2- or 4-byte boundary"""
    import torch

    c = scases[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    n = c["data"].size
    raw = torch.zeros(2 * n + 64, dtype=torch.uint8, device="cuda")
    src = raw[1 : 1 + n]
    src.copy_(torch.from_numpy(c["data"]))
    assert src.data_ptr() % 2 == 1
    want = sc.filtered(c)
    bb = pk.block_bytes
    if c["kind"] == "fir":
        dst = raw[n + 33 : n + 33 + n]
        state = _state(pk, c)
        for b in range(c["nblocks"]):
            _call(pk, c, src[b * bb : (b + 1) * bb], state, dst[b * bb : (b + 1) * bb])
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), want)
    state = _state(pk, c)
    for b in range(c["nblocks"]):
        _call(pk, c, src[b * bb : (b + 1) * bb], state)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), want)
    pk.close()


@pytest.mark.gpu
def test_gpu_state_sizes(api):
    for bps, nch, ns in ((4, 12, 2048), (3, 3, 1000), (1, 1, 40)):
        pk = api.new_hzr(bps, nch, ns)
        assert pk.iir_state_bytes() == 88 * nch
        for K in (1, 2, 31, 65536):
            want = 8 + ((K - 1) * nch * bps + 7) // 8 * 8
            assert pk.fir_state_bytes(K) == want
            st = pk.fir_state(K)
            assert st.numel() == want and st.data_ptr() % 8 == 0 and int(st.count_nonzero()) == 0
        pk.close()


@pytest.mark.gpu
def test_gpu_stream_entries_reject_bad_arguments(api):
    import torch

    L = api.lib()
    pk = api.new_hzr(4, 3, 100)
    bb = pk.block_bytes
    buf = torch.zeros(4 * bb, dtype=torch.uint8, device="cuda")
    src = buf[: 2 * bb]
    h, st = pk._h, torch.cuda.current_stream().cuda_stream
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    n3, d3 = np.array([1.0, -0.5, 0.1]), np.array([0.2, 0.3, 0.2])
    k3 = np.ones(3)
    istate = torch.zeros(pk.iir_state_bytes() + 8, dtype=torch.uint8, device="cuda")
    fstate = torch.zeros(pk.fir_state_bytes(65536) + 8, dtype=torch.uint8, device="cuda")
    # NULL bytes, kernel_size 0 and 65537
    nb = C.c_size_t()
    assert L.rspt_hip_iir_state_bytes(h, None) == ERR_ARG
    assert L.rspt_hip_fir_state_bytes(h, 3, None) == ERR_ARG
    assert L.rspt_hip_fir_state_bytes(h, 0, C.byref(nb)) == ERR_ARG
    assert L.rspt_hip_fir_state_bytes(h, 65537, C.byref(nb)) == ERR_ARG

    def iir(nc=3, nblocks=2, state=istate.data_ptr(), init=2, p=src.data_ptr()):
        n, d = np.resize(n3, max(nc, 1)).copy(), np.resize(d3, max(nc, 1)).copy()
        return L.rspt_hip_iir_prefilter_stream_dev(h, p, nblocks, dp(n), dp(d), nc, init, state, st)

    def fir(k=k3, nblocks=2, state=fstate.data_ptr(), s=src.data_ptr(), d=src.data_ptr(), size=None):
        return L.rspt_hip_fir_prefilter_stream_dev(h, s, d, nblocks, dp(np.ascontiguousarray(k, dtype=np.float64)), len(k) if size is None else size, state, st)

    assert iir(state=None) == ERR_ARG and iir(state=istate.data_ptr() + 4) == ERR_ARG  # NULL / misaligned state
    assert fir(state=None) == ERR_ARG and fir(state=fstate.data_ptr() + 4) == ERR_ARG
    assert iir(nc=1) == ERR_ARG and iir(nc=6) == ERR_ARG
    assert iir(nblocks=0) == ERR_ARG and fir(nblocks=0) == ERR_ARG
    assert iir(init=-1) == ERR_ARG and iir(p=None) == ERR_ARG
    assert fir(size=0) == ERR_ARG and fir(k=np.zeros(65537)) == ERR_ARG
    assert fir(s=None) == ERR_ARG and fir(d=None) == ERR_ARG
    assert fir(d=buf[16 : 16 + 2 * bb].data_ptr()) == ERR_ARG and fir(d=buf[bb : 3 * bb].data_ptr()) == ERR_ARG  # partial overlap
    # nblocks * ns at 2^31 rows and more: refused before anything is launched (no such buffer exists here)
    big = (1 << 31) // 100 + 1
    assert iir(nblocks=big) == ERR_UNSUPPORTED and fir(nblocks=big) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert int(buf.count_nonzero()) == 0 and int(istate.count_nonzero()) == 0 and int(fstate.count_nonzero()) == 0  # nothing ran
    # accepted: the extremes, apart
    assert fir(k=np.ones(65536) / 65536, d=buf[2 * bb :].data_ptr()) == 0
    assert iir(nc=2) == 0 and iir(nc=5) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError):  # a carried state is the per-channel driving
        pk.iir_prefilter_batch(src, n3, d3, per_channel=False, state=pk.iir_state())
    pk.close()
