"""The FIR pre-filter on the planar int32 matrix (rspt_hip_fir_prefilter_planar_batch_dev / _stream_dev,
rspt_hip_fir_planar_state_bytes; tests/fir_planar_cases.py).

CPU: the planar expectation of every case of the FIR records, cut to the case's sample width, is the compiled reference's record;
what the planar case lists cover; no fused multiply-add in the planar kernel; the C ABI.
GPU (-m gpu): row ends, several spans per row, stream calls with their state, native and planar calls on one state, values outside
the handle's sample width, overflow / inf / NaN, the cross identities with the native entry and with compress_planar_batch, a
seeded sweep, back-to-back calls, refusals, a foreign stream.  Every buffer and state sits between guards."""
import ctypes as C
import re

import numpy as np
import pytest

import devframe as df
import fir_cases as fc
import fir_planar_cases as pc
import stream_filter_cases as sc
from cases import digest
from devframe import ERR_ARG, ERR_UNSUPPORTED, api, asm  # noqa: F401

ENTRIES = ("rspt_hip_fir_prefilter_planar_batch_dev", "rspt_hip_fir_planar_state_bytes", "rspt_hip_fir_prefilter_planar_stream_dev")


# ---- CPU ----

def test_planar_expectation_cut_to_the_sample_width_is_the_fir_record():
    for c, r in zip(fc.fir_cases(), df.golden("fir_record.json")["cases"]):
        assert c["name"] == r["name"]
        k = fc.kernel_from_record(r["kernel"])
        P = pc.record_planar(c)
        assert P.shape == (1, c["nch"], c["ns"]) and P.dtype == np.int32
        assert fc.crc(pc.cut(P, c["bps"])) == r["in_crc32"], c["name"]  # (the layout helpers are inverse to each other)
        y = pc.cut(pc.stateless_expected(P, k), c["bps"])
        assert digest(y) == r["shared"]["digest"] and fc.crc(y) == r["shared"]["crc32"], c["name"]


def test_planar_stream_expectation_cut_to_the_sample_width_is_the_stream_record():
    recs = {r["name"]: r for r in df.golden("stream_filter_record.json")["cases"]}
    seen = 0
    for c in sc.stream_cases():
        if c["kind"] != "fir":
            continue
        r = recs[c["name"]]
        k = fc.kernel_from_record(r["kernel"])
        P = pc.record_planar(c, c["nblocks"])
        assert fc.crc(pc.cut(P, c["bps"])) == r["in_crc32"], c["name"]
        want, tail = pc.stream_expected(P, k)
        y = pc.cut(want, c["bps"])
        assert digest(y) == r["digest"] and fc.crc(y) == r["crc32"], c["name"]
        assert tail.shape == (len(k) - 1, c["nch"])
        seen += 1
    assert seen == sum(r["kind"] == "fir" for r in recs.values()) == 10


def test_row_cases_cover_every_length_offset_tap_count_and_mode():
    Cs = pc.row_cases()
    assert {c["ns"] for c in Cs} == set(pc.ROW_NS) and {c["nch"] for c in Cs} >= set(pc.NCH)
    assert {c["K"] for c in Cs} == set(pc.ROW_KS) | {4097}
    assert any(c["K"] == 4097 and c["ns"] == 700 and c["dst_off"] is None for c in Cs) and any(c["K"] == 4097 and c["dst_off"] is not None for c in Cs)
    assert {(c["src_off"], c["dst_off"]) for c in Cs if c["dst_off"] is not None} == {(s, d) for s in pc.OFFSETS for d in pc.OFFSETS}
    assert {c["src_off"] for c in Cs if c["dst_off"] is None} == set(pc.OFFSETS)
    # a lane's run of R outputs: full, one sample, all but one; a row of one chunk less one sample, one chunk, one chunk and one
    assert {ns % pc.R for ns in pc.ROW_NS} >= {0, 1, pc.R - 1} and {pc.CHUNK - 1, pc.CHUNK, pc.CHUNK + 1} <= set(pc.ROW_NS)
    assert pc.R == 16 and pc.CHUNK == 4096
    for ns in pc.SHORT_NS:  # several rows to a workgroup, both modes
        sel = [c for c in Cs if c["ns"] == ns]
        assert all(pc.geom(256, c["nblocks"], c["nch"], ns, c["K"])["rows_per_workgroup"] >= 32 for c in sel)
        assert {c["dst_off"] is None for c in sel} == {True, False}
    assert {pc.geom(256, 2, 3, ns, 5)["lanes"] for ns in pc.ROW_NS} == {1, 2, 4, 8, 16, 32, 64, 128, 256}
    for K in pc.ROW_KS:  # every tap count in both modes, and on the wide path (16-byte aligned rows) as on the dword path
        sel = [c for c in Cs if c["K"] == K]
        assert {c["dst_off"] is None for c in sel} == {True, False}, K
    wide = [c for c in Cs if c["src_off"] == 0 and c["dst_off"] in (None, 0) and c["ns"] % 4 == 0]
    for ns in (pc.CHUNK, pc.LONG_NS):  # 16-byte aligned rows: a chunk that reaches in front of the row, and chunks that do not
        assert {c["dst_off"] is None for c in wide if c["ns"] == ns} == {True, False}
    assert any(c["ns"] < pc.CHUNK for c in wide)
    for c in Cs:  # at least two blocks; every channel its own samples
        P = c["planar"]
        assert P.dtype == np.int32 and c["nblocks"] >= 2 and all(not np.array_equal(P[0, 0], P[0, ch]) for ch in range(1, c["nch"]))
    assert any(c["nch"] > 1 for c in Cs)


def test_span_cases_are_split_and_the_span_rule_limits_the_longest_kernel():
    for cu in (8, 256, 304):
        for K in pc.SPAN_KS:
            g = pc.geom(cu, 1, 2, 40000, K)
            assert g["nsplit"] > 1 and g["span"] >= 4 * (K - 1) and g["span"] % pc.CHUNK == 0
    # 9 whole chunks -> 9 spans of 4445 samples, in whole chunks: 5 spans of two chunks; with 4 (K - 1) = 8192: 4 spans of three
    assert [pc.geom(256, 1, 2, 40000, K)["nsplit"] for K in pc.SPAN_KS] == [5, 5, 4]
    assert {c["K"] for c in pc.span_cases()} == set(pc.SPAN_KS) and all(c["dst_off"] is None and c["ns"] == 40000 for c in pc.span_cases())


def test_stream_cases_reach_into_earlier_blocks_earlier_calls_and_past_a_call():
    Cs = pc.stream_cases()
    assert {c["ns"] for c in Cs} == set(pc.STREAM_NS) and {c["calls"] for c in Cs} == set(pc.STREAM_CUTS)
    for ns in pc.STREAM_NS:
        sel = [c for c in Cs if c["ns"] == ns]
        below, blocks_back, past_call = pc.stream_taps(ns)
        assert 1 < below - 1 < ns and 2 * ns < blocks_back - 1 < 3 * ns and past_call - 1 > 5 * ns
        assert {c["K"] for c in sel} == {below, blocks_back, past_call}
        for K in (below, blocks_back, past_call):
            assert {c["dst_off"] is None for c in sel if c["K"] == K} == {True, False}, (ns, K)
    assert all(len(c["calls"]) == 3 and sum(c["calls"]) == c["nblocks"] for c in Cs)  # the first call on a fresh state, two on a started one
    assert {c["nch"] for c in Cs} >= {1, 3, 64, 65}


def test_width_cases_hold_values_and_answers_outside_the_sample_width():
    W = pc.width_cases()
    assert {c["bps"] for c in W} == {1, 2, 3} and {bool(c["calls"]) for c in W} == {True, False}
    for c in W:
        P, bps = c["planar"], c["bps"]
        assert (P == 1 << (8 * bps)).any() and (P == pc.FULL).any() and (P == -pc.FULL - 1).any()
        want = pc.expected(c)[0]
        lim = 1 << (8 * bps - 1)
        assert ((want >= lim) | (want < -lim)).mean() > 0.5, c["name"]  # cutting the output would show


def test_overflow_cases_hold_int32_min_from_overflow_and_from_nan():
    nan, gain = pc.overflow_cases()
    for c in (nan, gain):
        y = fc.fir_i32(pc.rows_of(c["planar"]), c["kernel"])
        assert ((np.abs(y) >= 2.0 ** 31) | ~np.isfinite(y)).sum() > 100
        assert (pc.expected(c)[0] == fc.INT32_MIN).sum() > 100
    assert np.isnan(fc.fir_i32(pc.rows_of(nan["planar"]), nan["kernel"])).sum() > 100
    assert list(nan["kernel"]) == [1e308, -1e308, 0.5, 1e308]


def test_the_planar_filter_kernel_rounds_every_product_and_sum_on_its_own(asm):
    """k_fir_planar<wide>: two instantiations, no fp FMA and no f64 MFMA, separate v_mul_f64 / v_add_f64, wide loads and stores on
    the aligned one; the movers hold no fp arithmetic"""
    names = df.rounds_separately(asm, r"12k_fir_planarIL", 2)
    for n in names:
        text = "".join(asm[n])
        assert not re.search(r"^\s+scratch_", text, re.M), n
        assert re.search(r"global_load_dwordx4", text), n  # a lane's tap group is contiguous on either path
    assert len([n for n in names if re.search(r"global_store_dwordx4", "".join(asm[n]))]) == 1  # the aligned instantiation
    movers = [n for n in asm if re.search(r"k_firp_(head|save|front)", n)]
    assert len(movers) == 3
    for n in movers:
        assert not re.search(r"^\s+v_\w+_f(16|32|64)\b", "".join(asm[n]), re.M), n


def test_header_table_and_library_agree_on_the_planar_entries():
    df.check_entries(("int rspt_hip_fir_prefilter_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, "
                      "const double* kernel, size_t kernel_size, void* stream);",
                      "int rspt_hip_fir_planar_state_bytes(rspt_hip_packer* p, size_t kernel_size, size_t* bytes);",
                      "int rspt_hip_fir_prefilter_planar_stream_dev(rspt_hip_packer* p, const int32_t* d_src, int32_t* d_dst, size_t nblocks, "
                      "const double* kernel, size_t kernel_size, void* d_state, void* stream);"),
                     ENTRIES, native_of={n: n.replace("planar_", "") for n in ENTRIES})  # pointer types as the native siblings


def test_argument_checks_that_need_no_device():
    from rspt_amd import api

    L = api.lib()
    k = (C.c_double * 3)(0.25, 0.5, 0.25)
    buf = C.create_string_buffer(4096)
    sp = (C.addressof(buf) + 15) & ~15
    n = C.c_size_t(12345)
    assert L.rspt_hip_fir_planar_state_bytes(None, 5, C.byref(n)) == ERR_ARG and n.value == 12345
    assert L.rspt_hip_fir_prefilter_planar_batch_dev(None, sp, sp, 1, k, 3, None) == ERR_ARG
    assert L.rspt_hip_fir_prefilter_planar_stream_dev(None, sp, sp, 1, k, 3, sp, None) == ERR_ARG


# ---- GPU ----

def _what(c):
    return df.what(c, hide=("planar", "kernel"))


def _check(api, c, want=None, tail=None, calls="own"):
    """c through the planar entry between guards (devframe.planar_window), against the restatement -> the output"""
    if want is None:
        want, tail = pc.expected(c)
    K, kernel = len(c["kernel"]), c["kernel"]
    return df.planar_window(api, c, lambda pk, src, **kw: pk.fir_prefilter_planar_batch(src, kernel, **kw), lambda pk: pk.fir_planar_state_bytes(K),
                            pc.state_bytes(K, c["nch"]), want, None if tail is None else pc.state_image(K, c["nch"], tail), calls, hide=("planar", "kernel"))[0]


@pytest.mark.gpu
def test_gpu_stateless_row_ends(api):
    for c in pc.row_cases():
        _check(api, c)


@pytest.mark.gpu
def test_gpu_several_spans_per_row_in_place(api):
    import torch

    cu = torch.cuda.get_device_properties(0).multi_processor_count
    for c in pc.span_cases():
        assert pc.geom(cu, c["nblocks"], c["nch"], c["ns"], c["K"])["nsplit"] > 1
        _check(api, c)


@pytest.mark.gpu
def test_gpu_stream_bit_exact_with_its_state(api):
    for c in pc.stream_cases():
        _check(api, c)
        if c["K"] == pc.stream_taps(c["ns"])[1] and c["calls"] == pc.STREAM_CUTS[0]:  # however it is cut: one call
            _check(api, c, calls=(c["nblocks"],))


@pytest.mark.gpu
def test_gpu_stream_on_a_zeroed_state_equals_the_stateless_entry_on_one_long_row(api):
    import torch

    for c in [c for c in pc.stream_cases() if c["calls"] == pc.STREAM_CUTS[1]]:
        got = _check(api, c, calls=(c["nblocks"],))
        nb, nch, ns = c["planar"].shape
        long_ = pc.planar_of(pc.rows_of(c["planar"]), 1, nch, nb * ns)
        pk = api.new_hzr(4, nch, nb * ns)
        out = pk.fir_prefilter_planar_batch(torch.from_numpy(np.array(long_)).cuda(), c["kernel"])
        torch.cuda.synchronize()
        assert np.array_equal(pc.rows_of(out.cpu().numpy()), pc.rows_of(got)), _what(c)
        pk.close()


@pytest.mark.gpu
def test_gpu_zeroing_a_used_state_starts_afresh_and_two_states_interleave(api):
    import torch

    c = next(c for c in pc.stream_cases() if c["ns"] == 48 and c["nch"] > 1 and c["K"] == pc.stream_taps(48)[1])
    P, k, nch = c["planar"], c["kernel"], c["nch"]
    nb = P.shape[0]
    Q = np.ascontiguousarray(P[::-1] // 3)  # a second recording
    wp, wq = pc.stream_expected(P, k)[0], pc.stream_expected(Q, k)[0]
    pk = api.new_hzr(4, nch, c["ns"])
    sa, sb = pk.fir_planar_state(len(k)), pk.fir_planar_state(len(k))
    a, b = torch.from_numpy(P.copy()).cuda(), torch.from_numpy(Q).cuda()
    for b0 in range(nb):  # block by block, the two recordings in turn on one handle
        pk.fir_prefilter_planar_batch(a[b0 : b0 + 1], k, state=sa)
        pk.fir_prefilter_planar_batch(b[b0 : b0 + 1], k, state=sb)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), wp) and np.array_equal(b.cpu().numpy(), wq)
    # the used state continues the recording: P again behind P is not P from a fresh state ...
    a2 = torch.from_numpy(P.copy()).cuda()
    pk.fir_prefilter_planar_batch(a2, k, state=sa)
    torch.cuda.synchronize()
    twice = pc.stream_expected(np.concatenate([P, P]), k)[0][nb:]
    assert np.array_equal(a2.cpu().numpy(), twice) and not np.array_equal(twice, wp)
    # ... and zeroed it is a fresh object
    sa.zero_()
    a3 = torch.from_numpy(P.copy()).cuda()
    pk.fir_prefilter_planar_batch(a3, k, state=sa)
    torch.cuda.synchronize()
    assert np.array_equal(a3.cpu().numpy(), wp)
    pk.close()


@pytest.mark.gpu
def test_gpu_native_and_planar_calls_alternate_on_one_state(api):
    """bps = 4: one recording in three calls -- native, planar, native -- gives the all-native run's output and state; and the
    sizes: equal at bps = 4, rows of int32 on a 2-byte handle"""
    import torch

    nch, ns, cuts, K = 3, 40, (2, 3, 2), 101  # K - 1 = 100 rows: two and a half blocks
    nb = sum(cuts)
    P = pc.block(nb, nch, ns, 1501, 1 << 26)
    k = pc.kernel(K, 1502)
    pk = api.new_hzr(4, nch, ns)
    bb = pk.block_bytes
    assert pk.fir_planar_state_bytes(K) == pk.fir_state_bytes(K) == 8 + (K - 1) * nch * 4
    p2 = api.new_hzr(2, nch, ns)
    assert p2.fir_planar_state_bytes(K) == 8 + ((K - 1) * nch * 4 + 7) // 8 * 8 != p2.fir_state_bytes(K)
    assert p2.fir_planar_state_bytes(2) == 8 + 16 and p2.fir_planar_state(2).numel() == 24
    p2.close()

    def drive(plan):
        rec = pc.native_of(P).reshape(nb, bb).copy()
        state = pk.fir_state(K)
        b0 = 0
        for n, layout in zip(cuts, plan):
            if layout == "native":
                buf = torch.from_numpy(rec[b0 : b0 + n]).cuda()
                pk.fir_prefilter_batch(buf, k, state=state)
                torch.cuda.synchronize()
                rec[b0 : b0 + n] = buf.cpu().numpy()
            else:
                rows = rec[b0 : b0 + n].reshape(-1).view("<i4").reshape(n * ns, nch)
                raw, view = df.guarded_matrix(pc.planar_of(rows, n, nch, ns), 4)
                pk.fir_prefilter_planar_batch(view, k, state=state)
                torch.cuda.synchronize()
                assert df.guards_untouched(raw, 4, view.numel() * 4)
                rec[b0 : b0 + n] = pc.native_of(view.cpu().numpy()).reshape(n, bb)
            b0 += n
        return rec, state.cpu().numpy()

    want, want_state = drive(["native"] * 3)
    model, tail = pc.stream_expected(P, k)
    assert np.array_equal(want.reshape(-1), pc.native_of(model)) and np.array_equal(want_state, pc.state_image(K, nch, tail))
    for plan in (["native", "planar", "native"], ["planar", "native", "planar"]):
        got, got_state = drive(plan)
        assert np.array_equal(got, want) and np.array_equal(got_state, want_state), plan
    pk.close()


@pytest.mark.gpu
def test_gpu_values_outside_the_sample_width_are_filtered_whole_and_stored_uncut(api):
    for c in pc.width_cases():
        _check(api, c)


@pytest.mark.gpu
def test_gpu_overflow_inf_and_nan_become_int32_min(api):
    for c in pc.overflow_cases():
        got = _check(api, c)
        assert (got == fc.INT32_MIN).sum() > 100


CROSS = ("rand7x1001_i8_k2", "synth5x3000_i16_lowpass31", "ds3x20000_i24_k1_gain", "rand3x700_i24_k4097", "synth4x2500_i32_differentiator")


def _streams(d_dst, d_sizes):
    import torch

    torch.cuda.synchronize()
    sizes = d_sizes.cpu().numpy().astype(np.uint64)
    dst = d_dst.cpu().numpy()
    assert not any(int(s) >> 63 for s in sizes)
    return [dst[i, : int(s)].tobytes() for i, s in enumerate(sizes)]


@pytest.mark.gpu
def test_gpu_cross_identities_with_the_native_entry_and_the_planar_packer(api, orc):
    """from_planar_i32(fir_planar(to_planar_i32(X))) == fir_prefilter_batch(X), and compress_planar_batch(fir_planar(to_planar_i32(X)))
    gives the oracle's streams of the restatement's output"""
    import torch

    by = {c["name"]: c for c in fc.fir_cases()}
    assert {by[n]["bps"] for n in CROSS} == {1, 2, 3, 4}
    for name in CROSS:
        c = by[name]
        bps, nch, ns, k = c["bps"], c["nch"], c["ns"], np.asarray(c["kernel"])
        X = np.stack([c["data"], c["data"][::-1].copy()])  # two blocks
        want_blocks = [fc.fir_prefilter(X[b], bps, nch, ns, k) for b in range(2)]
        pk = api.new_xdelta_hzr(bps, nch, ns, 3)
        native = pk.fir_prefilter_batch(torch.from_numpy(X).cuda(), k)
        P = pk.fir_prefilter_planar_batch(pk.to_planar_i32(torch.from_numpy(X).cuda()), k)
        back = pk.from_planar_i32(P)
        torch.cuda.synchronize()
        assert np.array_equal(back.cpu().numpy().reshape(2, -1), native.cpu().numpy().reshape(2, -1)), name
        assert np.array_equal(native.cpu().numpy().reshape(2, -1), np.stack(want_blocks)), name
        po = orc.packer("xdelta_hzr", bps, nch, ns, 3)
        want = [po.compress(np.frombuffer(want_blocks[b].tobytes(), dtype=np.uint8)) for b in range(2)]
        assert _streams(*pk.compress_planar_batch(P)) == want, name
        pk.close()


@pytest.mark.gpu
def test_gpu_random_sweep(api):
    """about 200 random small cases against the restatement: shapes, taps, offsets, in and out of place, stateless or cut into calls"""
    S = pc.sweep_cases()
    assert len(S) == 200 and {bool(c["calls"]) for c in S} == {True, False} and {c["dst_off"] is None for c in S} == {True, False}
    for c in S:
        want, tail = pc.stream_expected(c["planar"], c["kernel"]) if c["calls"] else (pc.stateless_expected(c["planar"], c["kernel"]), None)
        _check(api, c, want, tail)


@pytest.mark.gpu
def test_gpu_back_to_back_calls_without_host_sync(api):
    """two in-place calls on one handle and one stream with no host synchronisation between them, the second with more taps (the
    staged fronts and the head grow while the first may be in flight), the caller's arrays overwritten as soon as each call
    returns: each call filters with its own coefficients.  2 x (2 ch x 40000): the rows are split, so both calls stage fronts."""
    import torch

    P = pc.block(2, 2, 40000, 1601)
    k1, k2 = pc.kernel(9, 1602), pc.kernel(257, 1603)
    w1, w2 = pc.stateless_expected(P, k1), pc.stateless_expected(P, k2)
    s1, s2 = pc.stream_expected(P, k1)[0], pc.stream_expected(P, k2)[0]
    pk = api.new_hzr(4, 2, 40000)
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert pc.geom(cu, 2, 2, 40000, 9)["nsplit"] > 1 and pc.geom(cu, 2, 2, 40000, 257)["nsplit"] > 1
    a, b, c, d = (torch.from_numpy(P.copy()).cuda() for _ in range(4))
    st1, st2 = pk.fir_planar_state(9), pk.fir_planar_state(257)
    torch.cuda.synchronize()
    ka, kb = k1.copy(), k2.copy()
    pk.fir_prefilter_planar_batch(a, ka)
    ka[:] = np.nan
    pk.fir_prefilter_planar_batch(b, kb)
    kb[:] = np.nan
    ka, kb = k1.copy(), k2.copy()
    pk.fir_prefilter_planar_batch(c, ka, state=st1)
    ka[:] = np.nan
    pk.fir_prefilter_planar_batch(d, kb, state=st2)
    kb[:] = np.nan
    torch.cuda.synchronize()
    for got, want, what in ((a, w1, "k9"), (b, w2, "k257"), (c, s1, "k9 stream"), (d, s2, "k257 stream")):
        assert np.array_equal(got.cpu().numpy(), want), what
    pk.close()


@pytest.mark.gpu
def test_gpu_planar_entries_refuse_bad_arguments_and_write_nothing(api):
    import torch

    L = api.lib()
    nch, ns = 3, 100
    pk = api.new_hzr(2, nch, ns)
    P = pc.block(4, nch, ns, 1701)
    raw, view = df.guarded_matrix(P, 0)
    before = raw.clone()
    n = P.size * 4 // 2  # bytes of two blocks
    h, st = pk._h, torch.cuda.current_stream().cuda_stream
    straw, state = df.guarded(pk.fir_planar_state_bytes(65536) + 8, 8, fill=0)
    sbefore = straw.clone()
    dp = C.POINTER(C.c_double)
    k3 = np.array([0.25, 0.5, 0.25])
    base = view.data_ptr()
    NULL = object()

    def call(stream_form, handle=h, s=base, d=base, nblocks=2, k=k3, size=None, state_ptr=state.data_ptr()):
        kk = None if k is NULL else np.ascontiguousarray(k, dtype=np.float64).ctypes.data_as(dp)
        a = [handle, s, d, nblocks, kk, (0 if k is NULL else len(k)) if size is None else size]
        if stream_form:
            return L.rspt_hip_fir_prefilter_planar_stream_dev(*a, state_ptr, st)
        return L.rspt_hip_fir_prefilter_planar_batch_dev(*a, st)

    too_many = (1 << 31) // nch + 1  # nblocks * nch >= 2^31
    too_long = ((1 << 31) - (1 << 17)) // ns + 1  # a stream call of 2^31 - 2^17 rows and more
    for sf in (False, True):
        assert call(sf, handle=None) == ERR_ARG and call(sf, s=None) == ERR_ARG and call(sf, d=None) == ERR_ARG and call(sf, k=NULL, size=3) == ERR_ARG
        assert call(sf, nblocks=0) == ERR_ARG and call(sf, nblocks=too_many) == ERR_ARG
        assert call(sf, size=0) == ERR_ARG and call(sf, k=np.zeros(65537)) == ERR_ARG
        for off in (1, 2, 3):  # off the 4-byte alignment, either buffer
            assert call(sf, s=base + off, d=base + off) == ERR_ARG and call(sf, s=base + off, d=base + n) == ERR_ARG and call(sf, d=base + n + off) == ERR_ARG
        assert call(sf, d=base + 16) == ERR_ARG and call(sf, d=base + n // 2) == ERR_ARG and call(sf, s=base + n // 2, d=base) == ERR_ARG  # partial overlap
    assert call(True, state_ptr=None) == ERR_ARG and call(True, state_ptr=state.data_ptr() + 4) == ERR_ARG
    assert call(True, nblocks=too_long) == ERR_UNSUPPORTED
    nb = C.c_size_t(777)
    assert L.rspt_hip_fir_planar_state_bytes(h, 3, None) == ERR_ARG
    assert L.rspt_hip_fir_planar_state_bytes(h, 0, C.byref(nb)) == ERR_ARG and L.rspt_hip_fir_planar_state_bytes(h, 65537, C.byref(nb)) == ERR_ARG
    assert nb.value == 777
    wide = api.new_hzr(1, 8192, 4)  # more than 8191 channels
    wbuf = torch.zeros(8192 * 4, dtype=torch.int32, device="cuda")
    wstate = torch.zeros(8 + 2 * 8192 * 4, dtype=torch.uint8, device="cuda")
    assert call(False, handle=wide._h, s=wbuf.data_ptr(), d=wbuf.data_ptr(), nblocks=1) == ERR_UNSUPPORTED
    assert call(True, handle=wide._h, s=wbuf.data_ptr(), d=wbuf.data_ptr(), nblocks=1, state_ptr=wstate.data_ptr()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(raw, before) and torch.equal(straw, sbefore) and int(wbuf.count_nonzero()) == 0 and int(wstate.count_nonzero()) == 0
    wide.close()
    with pytest.raises(AssertionError):
        pk.fir_prefilter_planar_batch(view.view(torch.uint8), k3)  # (not an int32 tensor)
    # accepted: the largest kernel, apart, on a handle whose bps is not 4, stateless and on a state
    assert call(False, k=np.ones(65536) / 65536, d=base + n) == 0
    assert call(True, k=np.ones(65536) / 65536) == 0
    torch.cuda.synchronize()
    got = view.cpu().numpy()
    want = pc.stream_expected(P[:2], np.ones(65536) / 65536)[0]
    assert np.array_equal(got[:2], want) and np.array_equal(got[2:], pc.stateless_expected(P[:2], np.ones(65536) / 65536))
    assert df.guards_untouched(raw, 0, P.size * 4) and df.guards_untouched(straw, 8, state.numel())
    pk.close()


@pytest.mark.gpu
def test_gpu_planar_entries_run_on_a_foreign_stream(api):
    import torch

    s = torch.cuda.Stream()
    picks = [next(c for c in pc.row_cases() if c["ns"] == 257 and c["nch"] > 1), pc.span_cases()[0],
             next(c for c in pc.stream_cases() if c["ns"] == 100 and c["dst_off"] is None),
             next(c for c in pc.stream_cases() if c["ns"] == 100 and c["dst_off"] is not None)]
    for c in picks:
        want = pc.expected(c)[0]
        pk = api.new_hzr(4, c["nch"], c["ns"])
        raw, src = df.guarded_matrix(c["planar"], c["src_off"])
        draw, dst = (raw, src) if c["dst_off"] is None else df.guarded_matrix(c["planar"], c["dst_off"], fill=0)
        state = pk.fir_planar_state(len(c["kernel"])) if c["calls"] else None
        s.wait_stream(torch.cuda.current_stream())
        b0 = 0
        for k in c["calls"] or [c["nblocks"]]:
            pk.fir_prefilter_planar_batch(src[b0 : b0 + k], c["kernel"], d_out=None if dst is src else dst[b0 : b0 + k], state=state, stream=s.cuda_stream)
            b0 += k
        s.synchronize()
        off = c["src_off"] if dst is src else c["dst_off"]
        assert np.array_equal(dst.cpu().numpy(), want) and df.guards_untouched(draw, off, dst.numel() * 4), _what(c)
        pk.close()
