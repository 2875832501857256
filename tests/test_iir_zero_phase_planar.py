"""The zero-phase IIR stage on the planar int32 matrix (rspt_hip_iir_zero_phase_planar_batch_dev, DESIGN.md 4b;
tests/iir_zero_phase_planar_cases.py).

CPU: the native record's cases taken as matrices -- the planar expectation cut to the case's sample width is the compiled
reference's record --, the numpy restatement against the reference's answers on int32 matrices
(tests/golden/iir_zero_phase_planar_record.json), what the case lists cover, the C ABI, no fused multiply-add in the planar
kernels, and the argument checks that need no device.
GPU (-m gpu): every case bit-exact in place and out of place (the source unchanged), the matrix 0, 4, 8 and 12 bytes off a
16-byte boundary between guards, neighbouring rows, values outside the handle's sample width, the unstable filters, a workspace
of 0xFF bytes, a repeated call, both routes on the same data, the identity with the native entry through the converters for every
width and byte order, the pipeline into compress_planar_batch, the refusals, a foreign stream."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import cases
import devframe as df
import iir_zero_phase_planar_cases as zp
from cases import digest
from devframe import ERR_ARG, ERR_UNSUPPORTED, api, asm  # noqa: F401

ENTRY = "rspt_hip_iir_zero_phase_planar_batch_dev"
INT32_MIN = -(1 << 31)

RECORDED, NATIVE = zp.recorded_cases(), zp.native_cases()
RECORDED_NAMES, NATIVE_NAMES = [c["name"] for c in RECORDED], [c["name"] for c in NATIVE]


@functools.lru_cache(maxsize=None)
def _record(which):
    return df.golden("iir_zero_phase_%srecord.json" % which)["cases"]


@functools.lru_cache(maxsize=None)
def _case(name):
    """the case with its record's exact coefficients: a recorded planar case, or a case of the native record as a matrix"""
    for C_, names, which in ((RECORDED, RECORDED_NAMES, "planar_"), (NATIVE, NATIVE_NAMES, "")):
        if name in names:
            i = names.index(name)
            r = _record(which)[i]
            assert r["name"] == name
            return zp.with_record_coefficients(C_[i], r)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _want(name):
    """the restatement's uncut answer [nblocks][nch][ns], computed once per process (read-only)"""
    y = zp.expected(_case(name))
    y.setflags(write=False)
    return y


def _matrix_bytes(P):
    return np.ascontiguousarray(P, dtype="<i4").view(np.uint8).reshape(-1)


def _same_as_record(c, got):
    """got [nblocks][nch][ns] against the compiled reference: a planar record holds the matrix, the native one its cut"""
    y = _matrix_bytes(got) if c["name"] in RECORDED_NAMES else zp.cut(got, c["bps"])
    return digest(y) == c["rec"]["digest"] and zp.crc(y) == c["rec"]["crc32"]


# ---- CPU ----

def test_record_inputs_have_not_drifted():
    rec = _record("planar_")
    assert len(RECORDED) == len(rec)
    for c, r in zip(RECORDED, rec):
        assert (c["name"], c["bps"], c["nch"], c["ns"], c["nblocks"]) == (r["name"], r["bps"], r["nch"], r["ns"], r["nblocks"])
        assert zp.crc(_matrix_bytes(c["planar"])) == r["in_crc32"], c["name"]
        assert zp.to_record(c) == {k: r[k] for k in ("n", "d", "init", "backward_init")}, c["name"]


@pytest.mark.parametrize("name", NATIVE_NAMES)
def test_planar_expectation_cut_to_the_sample_width_is_the_reference_record(name):
    c, want = _case(name), _want(name)
    assert want.shape == (c["nblocks"], c["nch"], c["ns"]) and want.dtype == np.int32
    assert _same_as_record(c, want)
    assert zp.crc(zp.cut(c["planar"], c["bps"])) == c["rec"]["in_crc32"]  # (the layout helpers are inverse to each other)


def test_restatement_matches_the_reference_on_int32_matrices():
    for name in RECORDED_NAMES:
        assert _same_as_record(_case(name), _want(name)), name


def test_the_cases_cover_every_length_row_count_route_order_and_history():
    S = zp.shape_cases()
    assert {c["ns"] for c in S} >= {1, 2, 5, 63, 64, 65, 67, 127, 128, 129, 191, 200}
    assert {c["nblocks"] * c["nch"] for c in S} == {1, 3, 64, 65, 130}
    assert any(c["nblocks"] > 1 and c["nch"] > 1 for c in S) and any(c["nblocks"] == 1 for c in S) and any(c["nch"] == 1 for c in S)
    assert {c["off"] for c in S} == set(zp.OFFSETS) and all(c["bps"] == 4 for c in S)
    pipe, plain = [c for c in S if zp.route(c) == "pipe"], [c for c in S if zp.route(c) == "plain"]
    # the pipelined kernel: every residue of the 16-sample part, rows of whole chunks and rows that end one sample into a chunk
    # or one short of it, every order, every backward history, rows that start off a 16-byte boundary, several workgroups
    assert {c["ns"] % zp.PART for c in pipe} == set(range(16))
    assert {c["ns"] % zp.CHUNK for c in pipe} >= {0, 1, 63} and {c["ns"] // zp.CHUNK for c in pipe} >= {1, 2, 3}
    assert any(c["ns"] % 4 and c["nblocks"] * c["nch"] > 64 for c in pipe)
    for sel in (pipe, plain):
        assert {len(c["n"]) for c in sel} == {2, 3, 4, 5}
        assert {c["binit"] for c in sel} == {0, 1, 2000}
        assert {c["nblocks"] * c["nch"] for c in sel} >= {1, 3, 64, 65, 130}
    # the histories: none, one short of the ring's tail, the tail, the harness's -- for every order
    for nc in (2, 3, 4, 5):
        assert {c["init"] for c in S if len(c["n"]) == nc} == set(zp.inits(nc)), nc
    assert {c["init"] for c in pipe} >= {1, 2, 3, 4, 2000}
    # the plain kernel below a chunk, and at a chunk and more behind a history shorter than the ring's tail
    assert {c["ns"] for c in plain} >= {1, 2, 5, 63} and any(c["ns"] >= zp.CHUNK and c["init"] < len(c["n"]) - 1 for c in plain)
    assert any(c["ns"] >= zp.CHUNK and c["init"] == len(c["n"]) - 2 and len(c["n"]) >= 3 for c in plain)
    n = _case(zp.NEIGHBOURS)
    assert (n["nblocks"] * n["nch"], n["ns"], zp.route(n)) == (130, 67, "pipe")
    for c in S:  # every row its own samples
        R = c["planar"].reshape(-1, c["ns"])
        assert R.dtype == np.int32 and (c["ns"] < 3 or all(not np.array_equal(R[0], R[r]) for r in range(1, len(R)))), c["name"]
    # fewer backward steps than the ring is long on the pipelined kernel: forward inputs stay in the x ring behind w[ns-1]
    assert any(0 < 4 * c["binit"] < len(c["n"]) for c in pipe)


def test_the_width_and_native_cases_cover_what_they_are_for():
    W = zp.width_cases()
    assert {(c["bps"], zp.route(c)) for c in W} == {(b, r) for b in (1, 2, 3) for r in ("pipe", "plain")}
    for c in W:
        P, bps = c["planar"], c["bps"]
        assert (P == 1 << (8 * bps)).any() and (P == zp.FULL).any() and (P == -zp.FULL - 1).any()
        want = _want(c["name"])
        lim = 1 << (8 * bps - 1)
        assert ((want >= lim) | (want < -lim)).mean() > 0.5, c["name"]  # cutting the output would show
        assert (want != INT32_MIN).mean() > 0.8, c["name"]  # (and it is the filter's output, not the truncation's overflow)
    assert {c["bps"] for c in NATIVE} == {1, 2, 3, 4}
    assert {zp.route(_case(n)) for n in zp.UNSTABLE_NAMES} == {"plain", "pipe"}
    assert tuple(zp.route(_case(n)) for n in zp.SAME_DATA_PAIR) == ("plain", "pipe")
    for n in zp.UNSTABLE_NAMES:  # the poisoned channel is INT32_MIN whole, not its low bytes
        assert (_want(n)[0, 1] == INT32_MIN).all() and (_want(n)[0, 0] != INT32_MIN).any()


def test_header_table_and_library_agree_on_the_entry():
    from rspt_amd import api

    df.check_entries(("int rspt_hip_iir_zero_phase_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, int32_t* d_out, size_t nblocks, "
                      "const double* n, const double* d, size_t nr_coefficients, int init_nr_samples, int backward_init_nr_samples, void* d_work, "
                      "size_t work_bytes, void* stream);",), (ENTRY,), methods=("iir_zero_phase_planar_batch",))
    # the native entry's arguments with (source, destination) in place of the buffer; no sizing entry of its own
    native = api.C_ABI["rspt_hip_iir_zero_phase_batch_dev"]
    assert api.C_ABI[ENTRY] == (native[0], native[1][:1] + [C.c_void_p, C.c_void_p] + native[1][2:])
    assert not [s for s in api.C_ABI_SYMBOLS if "zero_phase_planar" in s and s != ENTRY]


def test_the_planar_zero_phase_kernels_hold_no_fused_multiply_add(asm):
    """k_iir_zp_planar and k_iir_zp_pipe_planar, one instantiation per order"""
    for pat in (r"15k_iir_zp_planarIL", r"20k_iir_zp_pipe_planarIL"):
        names = [n for n in asm if re.search(pat, n)]
        assert len(names) == 4, (pat, sorted(names))
        for n in names:
            assert not [ln for ln in asm[n] if df.FUSED_F64_F32.match(ln)], n
            assert [ln for ln in asm[n] if re.match(r"^\s+v_mul_f64\b", ln)], n  # (the recurrence is in there, unfused)


def test_argument_checks_that_need_no_device():
    """a NULL handle is refused before anything touches a device"""
    from rspt_amd import api

    L = api.lib()
    k = (C.c_double * 3)(1.0, 0.5, 0.25)
    work = C.create_string_buffer(4096)
    wp = (C.addressof(work) + 7) & ~7
    assert L.rspt_hip_iir_zero_phase_planar_batch_dev(None, wp, None, 1, k, k, 3, 0, 0, wp, 2048, None) == ERR_ARG
    assert L.rspt_hip_iir_zero_phase_planar_batch_dev(None, wp, wp + 1024, 1, k, k, 3, 0, 0, wp, 2048, None) == ERR_ARG


# ---- GPU ----

def _what(c):
    return df.what(c, hide=("planar", "rec"))


def _differ(got, want):
    bad = np.argwhere(got != want)
    return "%d differ, first at [block, channel, sample] %s" % (len(bad), bad[:1].tolist()) if bad.size else ""


def _call(pk, c, view, out=None, work=None, stream=None):
    return pk.iir_zero_phase_planar_batch(view, c["n"], c["d"], init_nr_samples=c["init"], backward_init_nr_samples=c["binit"], out=out, work=work, stream=stream)


def _check(api, c, off=None, out_off=None, pk=None):
    """c in place (out_off None) or into a matrix of its own at out_off, both between guards; -> the output"""
    import torch

    off = c["off"] if off is None else off
    want, n = _want(c["name"]), c["planar"].size * 4
    own = pk is None
    pk = pk or api.new_hzr(c["bps"], c["nch"], c["ns"])
    raw, view = df.guarded_matrix(c["planar"], off)
    if out_off is None:
        res = _call(pk, c, view)
        assert res is view
    else:
        oraw, out = df.guarded_matrix(c["planar"], out_off, fill=df.FILL)
        res = _call(pk, c, view, out=out)
        assert res is out
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    assert df.guards_untouched(raw, off, n), ("guards", _what(c))
    if out_off is not None:
        assert df.guards_untouched(oraw, out_off, n), ("guards of the destination", _what(c))
        assert np.array_equal(view.cpu().numpy(), c["planar"]), ("the source changed", _what(c))
    assert not _differ(got, want), (_differ(got, want), _what(c))
    assert _same_as_record(c, got), ("record", _what(c))
    if own:
        pk.close()
    return got


@pytest.mark.gpu
def test_gpu_shape_cases_bit_exact_in_place_and_out_of_place(api):
    """every recorded shape, the matrix at its case's offset from a 16-byte boundary; out of place the destination sits at another
    offset and the source is unchanged afterwards"""
    for i, c in enumerate(_case(n) for n in RECORDED_NAMES if n.startswith("shape_")):
        _check(api, c)
        _check(api, c, out_off=zp.OFFSETS[(i + 1) % 4])


@pytest.mark.gpu
def test_gpu_native_record_cases_as_matrices(api):
    """the native record's cases, README band-pass included, through the planar entry; cut to their width they are the record"""
    for i, c in enumerate(_case(n) for n in NATIVE_NAMES):
        _check(api, c, out_off=None if i % 2 else zp.OFFSETS[(i // 2) % 4])


@pytest.mark.gpu
@pytest.mark.parametrize("off", [4, 8, 12])
def test_gpu_matrix_base_off_a_16_byte_boundary(api, off):
    """rows of both routes and of lengths with ns % 4 in {0, 1, 3}, source and destination at the same odd offset"""
    for name in ("ns129_i32_130ch_x2_nc5_init2000_b1", "ns200_i32_3ch_x4_nc5_init2000_b2000", "ns103_i32_3ch_x2_nc5_init3_b0_plain", zp.NEIGHBOURS):
        _check(api, _case(name), off=off)
        _check(api, _case(name), off=off, out_off=off)


@pytest.mark.gpu
def test_gpu_neighbouring_rows_and_guards(api):
    """130 rows of 67 samples: every row but the first starts off a 16-byte boundary, ends 3 samples into a part, and has another
    lane's or another workgroup's row directly behind it.  A store past a row's end or a load clamped by address shows in the
    neighbour (every row has a seed of its own); the guards around the matrix stay as they were"""
    c = _case(zp.NEIGHBOURS)
    for off in zp.OFFSETS:
        _check(api, c, off=off)
    _check(api, c, off=0, out_off=8)


@pytest.mark.gpu
def test_gpu_values_outside_the_sample_width_are_filtered_whole_and_stored_uncut(api):
    for c in (_case(n) for n in RECORDED_NAMES if n.startswith("width_")):
        assert c["bps"] < 4
        _check(api, c)
        _check(api, c, out_off=0)
    two = [c for c in zp.width_cases() if c["bps"] == 2]
    assert {zp.route(c) for c in two} == {"pipe", "plain"}  # (a bps = 2 handle through both kernels)


@pytest.mark.gpu
@pytest.mark.parametrize("name", zp.UNSTABLE_NAMES)
def test_gpu_the_unstable_filter_gives_int32_min_as_the_record_says(api, name):
    """NaN and inf through the turn: the poisoned channel of block 0 is INT32_MIN whole (the native entry stores its low bytes)"""
    c = _case(name)
    got = _check(api, c)
    assert (got[0, 1] == INT32_MIN).all() and (got[0, 0] != INT32_MIN).any()
    _check(api, c, out_off=4)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ns129_i32_130ch_x2_nc5_init2000_b1", "ns103_i32_3ch_x2_nc5_init3_b0_plain", zp.NEIGHBOURS])
def test_gpu_nothing_of_the_workspace_is_read_before_it_is_written(api, name):
    """a workspace of exactly the native entry's bound, full of 0xFF bytes (NaNs), gives the same output; the bytes behind it stay"""
    import torch

    c = _case(name)
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    nb = pk.iir_zero_phase_work_bytes(c["nblocks"])
    assert nb == (c["nblocks"] * c["nch"] + 63) // 64 * 64 * c["ns"] * 8
    raw = torch.full((nb + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    assert raw.data_ptr() % 8 == 0
    _, view = df.guarded_matrix(c["planar"], c["off"])
    _call(pk, c, view, work=raw[:nb])
    torch.cuda.synchronize()
    assert not _differ(view.cpu().numpy(), _want(name)), _what(c)
    assert int((raw[nb:] != 0xFF).count_nonzero()) == 0
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ns200_i32_3ch_x4_nc5_init2000_b2000", "ns5_i24_1ch_x5_nc4_init0_b2000"])
def test_gpu_a_repeated_call_gives_the_same_output(api, name):
    """the same handle and the same workspace, a fresh copy of the input: nothing of the first call is left for the second"""
    import torch

    c = _case(name)
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    work = torch.empty(pk.iir_zero_phase_work_bytes(c["nblocks"]) // 8, dtype=torch.float64, device="cuda")
    outs = []
    for _ in range(2):
        _, view = df.guarded_matrix(c["planar"], c["off"])
        _call(pk, c, view, work=work)
        torch.cuda.synchronize()
        outs.append(view.cpu().numpy())
    assert not _differ(outs[0], _want(name)) and np.array_equal(outs[0], outs[1])
    pk.close()


@pytest.mark.gpu
def test_gpu_the_plain_and_the_pipelined_route_on_the_same_data(api):
    """init below nc - 1 selects the plain kernel, init = nc - 1 the pipelined one; each agrees with its record"""
    a, b = (_case(n) for n in zp.SAME_DATA_PAIR)
    assert np.array_equal(a["planar"], b["planar"]) and (a["n"], a["d"], a["binit"]) == (b["n"], b["d"], b["binit"])
    assert (zp.route(a), zp.route(b)) == ("plain", "pipe")
    pk = api.new_hzr(a["bps"], a["nch"], a["ns"])
    for c in (a, b):
        _check(api, c, pk=pk)
        _check(api, c, out_off=12, pk=pk)
    pk.close()


@pytest.mark.gpu
def test_gpu_identity_with_the_native_entry_for_every_width_and_byte_order(api):
    """from_planar_i32(zp_planar(to_planar_i32(X))) == iir_zero_phase_batch(X), byte for byte.  The native entry reads
    little-endian samples whatever the handle's byte order; a big-endian handle's converters see the same samples reversed"""
    import torch

    nch, ns, B = 5, 131, 3
    n, d = cases.IIR_BANDPASS
    for bps in (1, 2, 3, 4):
        X = np.array(cases._rand_native(nch, B * ns, bps, 8100 + bps, 1 << (8 * bps - 3), walk=True), dtype=np.uint8)
        for init, binit in ((2000, 0), (1, 1)):  # (the pipelined and the plain route)
            pk = api.new_hzr(bps, nch, ns)
            want = pk.iir_zero_phase_batch(torch.from_numpy(X.copy()).cuda().reshape(B, -1), n, d, init_nr_samples=init, backward_init_nr_samples=binit)
            torch.cuda.synchronize()
            want = want.cpu().numpy().reshape(-1)
            assert not np.array_equal(want, X)
            for be in (False, True):
                pk.set_byte_order(be)
                src = cases.reverse_samples(X, bps) if be else X
                P = pk.to_planar_i32(torch.from_numpy(np.ascontiguousarray(src)).cuda().reshape(B, -1))
                res = pk.iir_zero_phase_planar_batch(P, n, d, init_nr_samples=init, backward_init_nr_samples=binit)
                got = pk.from_planar_i32(res)
                torch.cuda.synchronize()
                got = got.cpu().numpy().reshape(-1)
                assert np.array_equal(cases.reverse_samples(got, bps) if be else got, want), (bps, init, binit, be)
            pk.close()


def _streams(d_dst, d_sizes):
    import torch

    torch.cuda.synchronize()
    sizes = d_sizes.cpu().numpy().astype(np.uint64)
    dst = d_dst.cpu().numpy()
    assert not any(int(s) >> 63 for s in sizes)
    return [dst[i, : int(s)].tobytes() for i, s in enumerate(sizes)]


@pytest.mark.gpu
def test_gpu_pipeline_to_planar_zero_phase_compress_planar(api):
    """to_planar_i32 -> iir_zero_phase_planar_batch -> compress_planar_batch gives the streams of iir_zero_phase_batch ->
    compress_batch, with the README's band-pass on the two recordings"""
    import torch

    from rspt_amd import synth

    ns, B = 2048, 3
    n, d = cases.IIR_BANDPASS
    new = {"xdelta_hzr": lambda bps, nch: api.new_xdelta_hzr(bps, nch, ns, 3), "hzr": lambda bps, nch: api.new_hzr(bps, nch, ns)}
    for bps, nch, data in ((3, 3, np.frombuffer(synth.data_stream_3ch_i24(), dtype=np.uint8)), (4, 12, np.frombuffer(synth.ecg_12ch_i32(), dtype=np.uint8))):
        bb = bps * nch * ns
        X = np.array(data[: B * bb]).reshape(B, bb)
        for kind in ("xdelta_hzr", "hzr"):
            pn, pp = new[kind](bps, nch), new[kind](bps, nch)
            native = _streams(*pn.compress_batch(pn.iir_zero_phase_batch(torch.from_numpy(X).cuda(), n, d, init_nr_samples=2000)))
            P = pp.to_planar_i32(torch.from_numpy(X).cuda())
            Q = torch.empty_like(P)
            assert pp.iir_zero_phase_planar_batch(P, n, d, init_nr_samples=2000, out=Q) is Q
            out_of_place = _streams(*pp.compress_planar_batch(Q))
            pp.iir_zero_phase_planar_batch(P, n, d, init_nr_samples=2000)
            assert _streams(*pp.compress_planar_batch(P)) == native and out_of_place == native, (kind, bps, nch)
            pn.close()
            pp.close()


@pytest.mark.gpu
def test_gpu_the_entry_refuses_before_anything_is_launched(api):
    import torch

    L = api.lib()
    nch, ns = 3, 100
    pk = api.new_hzr(2, nch, ns)
    P = zp.block(2, nch, ns, 77)
    raw, view = df.guarded_matrix(P, 0)
    oraw, out = df.guarded_matrix(P, 4, fill=df.FILL)
    h, st = pk._h, torch.cuda.current_stream().cuda_stream
    need = pk.iir_zero_phase_work_bytes(2)
    assert need == 64 * ns * 8
    work = torch.full((need + 8,), 0xFF, dtype=torch.uint8, device="cuda")
    before, obefore = raw.clone(), oraw.clone()
    NULL = object()
    coef = np.array([1.0, -0.5, 0.1, 0.0, 0.0])
    dcoef = np.array([0.5, 0.25, 0.125, 0.0, 0.0])
    cp, dp = coef.ctypes.data_as(C.POINTER(C.c_double)), dcoef.ctypes.data_as(C.POINTER(C.c_double))

    def call(hh=h, p=view.data_ptr(), o=None, nblocks=2, n=cp, d=dp, nc=3, init=2, binit=0, w=work.data_ptr(), wb=need):
        return L.rspt_hip_iir_zero_phase_planar_batch_dev(hh, p, o, nblocks, None if n is NULL else n, None if d is NULL else d, nc, init, binit, w, wb, st)

    # everything the native entry refuses
    assert call(hh=None) == ERR_ARG and call(p=None) == ERR_ARG and call(n=NULL) == ERR_ARG and call(d=NULL) == ERR_ARG
    assert call(nc=1) == ERR_ARG and call(nc=6) == ERR_ARG
    assert call(init=-1) == ERR_ARG and call(init=(1 << 28) + 1) == ERR_ARG
    assert call(nblocks=0) == ERR_ARG and call(nblocks=(1 << 31) // nch + 1) == ERR_ARG  # nblocks * nch >= 2^31
    assert call(binit=-1) == ERR_ARG and call(binit=(1 << 28) + 1) == ERR_ARG
    assert call(w=None) == ERR_ARG and call(w=work.data_ptr() + 4) == ERR_ARG
    assert call(wb=need - 1) == ERR_ARG and call(wb=0) == ERR_ARG
    # the matrix and the destination off their 4-byte alignment
    for k in (1, 2, 3):
        assert call(p=view.data_ptr() + k) == ERR_ARG and call(o=out.data_ptr() + k) == ERR_ARG
        assert call(p=view.data_ptr() + k, o=view.data_ptr() + k) == ERR_ARG
    # partial overlap, from either side and by one sample; the destination behind the source's last byte is none
    nbytes = P.size * 4
    assert call(o=view.data_ptr() + 4, nblocks=1) == ERR_ARG and call(o=view.data_ptr() + nbytes // 2 - 4, nblocks=1) == ERR_ARG  # (one block: half the matrix)
    assert call(p=view.data_ptr() + 4, o=view.data_ptr(), nblocks=1) == ERR_ARG and call(p=view.data_ptr() + nbytes // 2 - 4, o=view.data_ptr(), nblocks=1) == ERR_ARG
    wide = api.new_hzr(1, 8192, 4)  # more than 8191 channels
    wbuf = torch.ones(8192 * 4, dtype=torch.int32, device="cuda")
    wwork = torch.full((8192 * 4 * 8,), 0xFF, dtype=torch.uint8, device="cuda")
    assert call(hh=wide._h, p=wbuf.data_ptr(), nblocks=1, w=wwork.data_ptr(), wb=wwork.numel()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    # nothing ran: a launch would have filtered the samples and written doubles over the 0xFF bytes
    assert torch.equal(raw, before) and torch.equal(oraw, obefore) and int((wbuf != 1).count_nonzero()) == 0
    assert int((work != 0xFF).count_nonzero()) == 0 and int((wwork != 0xFF).count_nonzero()) == 0
    wide.close()
    with pytest.raises(AssertionError):
        pk.iir_zero_phase_planar_batch(view.view(torch.uint8), [1.0, 0.5], [1.0, 0.5])  # (not an int32 tensor)
    with pytest.raises(AssertionError):
        pk.iir_zero_phase_planar_batch(view, [1.0, 0.5], [1.0, 0.5], out=out[:1])  # (not the matrix's shape)
    # accepted, on a handle whose bps is not 4: d_out the matrix itself; one block into the other half of the matrix (the ranges
    # touch and do not overlap); a workspace of exactly the bound, 8 bytes further on; both kernels
    assert call(o=view.data_ptr(), nc=2, init=0) == 0
    assert call(o=view.data_ptr() + nbytes // 2, nblocks=1) == 0
    assert call(o=out.data_ptr(), nc=5, init=1 << 14, binit=1 << 14, w=work.data_ptr() + 8) == 0
    torch.cuda.synchronize()
    assert not torch.equal(raw, before) and not torch.equal(oraw, obefore)  # (and a call that runs does show)
    assert df.guards_untouched(raw, 0, nbytes) and df.guards_untouched(oraw, 4, nbytes)
    pk.close()


@pytest.mark.gpu
def test_gpu_the_entry_runs_on_a_foreign_stream(api):
    import torch

    s = torch.cuda.Stream()
    for name, out_off in ((zp.NEIGHBOURS, None), ("ns103_i32_3ch_x2_nc5_init3_b0_plain", 8)):
        c = _case(name)
        pk = api.new_hzr(4, c["nch"], c["ns"])
        raw, view = df.guarded_matrix(c["planar"], c["off"])
        out = None if out_off is None else df.guarded_matrix(c["planar"], out_off, fill=df.FILL)[1]
        s.wait_stream(torch.cuda.current_stream())
        res = _call(pk, c, view, out=out, stream=s.cuda_stream)
        s.synchronize()
        assert not _differ(res.cpu().numpy(), _want(name)) and df.guards_untouched(raw, c["off"], view.numel() * 4), _what(c)
        pk.close()
