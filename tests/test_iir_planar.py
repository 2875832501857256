"""The IIR pre-filter and the IIR cascade on the planar int32 matrix (rspt_hip_iir_prefilter_planar_batch_dev / _stream_dev,
rspt_hip_iir_cascade_planar_batch_dev / _stream_dev; tests/iir_planar_cases.py).

CPU: the planar expectation of every sweep case (tests/iir_sweep_cases.py), cut to the case's sample width, is the compiled
reference's record; what the planar case lists cover; no fused multiply-add in the planar kernels.
GPU (-m gpu): the sweep through the planar entries; row ends, stream boundaries and routes of the planar addressing; values
outside the handle's sample width; native and planar calls on one state; the reference pipeline to_planar_i32 -> IIR ->
compress_planar_batch against the oracle and the native path; refusals; a foreign stream.  Every buffer sits between guards."""
import ctypes as C

import numpy as np
import pytest

import cases
import devframe as df
import iir_planar_cases as pc
import iir_sweep_cases as sw
from cases import digest
from devframe import ERR_ARG, ERR_UNSUPPORTED, api, asm  # noqa: F401
from iir_model import same_doubles, state_rings

BANDPASS = cases.IIR_BANDPASS  # the harness's band-pass (rspt_test.cpp:116-136), init_nr_samples 2000


# ---- CPU ----

@pytest.mark.parametrize("leg", pc.SWEEP_LEGS)
def test_planar_expectation_cut_to_the_sample_width_is_the_reference_record(leg):
    for c in sw.sweep_cases()[leg]:
        want, r = pc.sweep_expected(c), sw.record()[c["name"]]
        assert want.shape == (c["nblocks"], c["nch"], c["ns"]) and want.dtype == np.int32
        y = pc.cut(want, c["bps"])
        assert digest(y) == r["digest"] and sw.crc(y) == r["crc32"], c["name"]
        assert sw.crc(pc.cut(pc.sweep_planar(c), c["bps"])) == r["in_crc32"], c["name"]  # (the layout helpers are inverse to each other)


def test_some_sweep_answer_differs_from_its_cut():
    """the sweep's narrow cases hold outputs outside their sample width: 'uncut' is observable there"""
    for leg in pc.SWEEP_LEGS:
        wide = 0
        for c in sw.sweep_cases()[leg]:
            if c["bps"] < 4:
                want = pc.sweep_expected(c)
                lim = 1 << (8 * c["bps"] - 1)
                wide += bool(((want >= lim) | (want < -lim)).any())
        assert wide >= 4, leg


def test_row_cases_cover_every_length_offset_mode_and_stage():
    C = pc.row_cases()
    for kind, shared in (("single", False), ("single", True), ("cascade", None)):
        sel = [c for c in C if c["kind"] == kind and c.get("shared") == shared]
        assert {(c["ns"], c["off"]) for c in sel} == {(ns, off) for ns in pc.ROW_NS for off in pc.OFFSETS}, (kind, shared)
        assert {c["nch"] for c in sel} == set(pc.NCH), (kind, shared)
        assert all(pc.route(c) == "pipe" for c in sel)
        assert any(c["nblocks"] > 1 and c["nch"] > 1 for c in sel)  # rows of two blocks and of two channels side by side
    assert {len(c["n"]) for c in C if c["kind"] == "single"} == {2, 3, 4, 5}
    assert all(c["sections"] is pc.README_PAIR for c in C if c["kind"] == "cascade")
    # a row's last chunk: empty, one sample, a part and one sample, all but one sample; and the same for the cascade's chunk
    assert {ns % 64 for ns in pc.ROW_NS} >= {0, 1, 2, 3, 15, 16, 63} and {ns % 32 for ns in pc.ROW_NS} >= {0, 1, 15, 16, 31}
    for c in C:  # every channel its own samples
        P = c["planar"]
        assert P.dtype == np.int32 and all(not np.array_equal(P[0, 0], P[0, ch]) for ch in range(1, c["nch"]))


def test_stream_cases_put_block_boundaries_everywhere():
    C = pc.stream_cases()
    assert {c["ns"] for c in C} == set(pc.STREAM_NS) and {c["nch"] for c in C} == set(pc.NCH)
    for kind, chunk in (("single", pc.SINGLE_CHUNK), ("cascade", pc.CASCADE_CHUNK)):
        sel = [c for c in C if c["kind"] == kind]
        where = set()
        for c in sel:
            assert len(c["calls"]) == 3 and sum(c["calls"]) == c["nblocks"] and all(1 <= k <= 5 for k in c["calls"])
            for k in c["calls"]:
                if pc.route(c, k * c["ns"]) != "pipe":
                    continue
                if k == 1:
                    where.add("none")
                for b in range(1, k):  # the boundaries inside the call's run
                    at = b * c["ns"]
                    where.add("chunk" if at % chunk == 0 else "part" if at % pc.PART == 0 else "inside")
        assert where == {"none", "chunk", "part", "inside"}, (kind, where)
        assert {k for c in sel for k in c["calls"]} == {1, 2, 3, 4, 5}
        first = {pc.route(c, c["calls"][0] * c["ns"]) for c in sel}
        assert first == {"pipe", "plain"}, kind  # a fresh channel starts in either kernel
        if kind == "single":  # the plain kernel over a boundary (the cascade's takes fewer than 32 rows: the sweep's handles of 1 to 16)
            assert any(pc.route(c, k * c["ns"]) == "plain" and k > 1 for c in sel for k in c["calls"])
    assert {len(c["n"]) for c in C if c["kind"] == "single"} == {2, 3, 4, 5}
    assert {len(c["sections"]) for c in C if c["kind"] == "cascade"} >= {1, 2, 3}
    assert any(s[3] for c in C if c["kind"] == "cascade" for s in c["sections"][:1])  # a section 0 through filter()


def test_route_and_width_cases_cover_what_they_are_for():
    R = pc.route_cases()
    assert all(pc.route(c) == "plain" for c in R)
    single = [c for c in R if c["kind"] == "single"]
    assert {c["shared"] for c in single} == {False, True}
    assert any(c["ns"] >= 64 and 4 * c["init"] < len(c["n"]) - 1 and c["shared"] == s for c in single for s in (False, True))
    assert {c["ns"] for c in single if c["ns"] < 64} >= {1, 15, 16, 17, 63} and {c["ns"] for c in R if c["kind"] == "cascade"} >= {1, 31}
    W = pc.width_cases()
    assert {c["bps"] for c in W} == {1, 2, 3}
    for c in W:
        P, bps = c["planar"], c["bps"]
        assert (P == 1 << (8 * bps)).any() and (P == pc.FULL).any() and (P == -pc.FULL - 1).any()
        want = pc.expected(c)[0]
        lim = 1 << (8 * bps - 1)
        assert ((want >= lim) | (want < -lim)).mean() > 0.5, c["name"]  # cutting the output would show
    assert {(c["kind"], bool(c["calls"]), c.get("shared")) for c in W} == {("single", False, False), ("single", False, True), ("cascade", False, None),
                                                                            ("single", True, False), ("cascade", True, None)}


def test_the_planar_kernels_hold_no_fused_multiply_add(asm):
    """k_iir_planar (order x mode), k_iir_planar_carry (order), k_iir_pipe_planar (order x (per channel, shared, carried)),
    k_iir_cascade_planar and k_iir_cascade_pipe_planar (stateless, carried)"""
    want = {r"12k_iir_planarIL": 8, r"18k_iir_planar_carryIL": 4, r"17k_iir_pipe_planarIL": 12, r"20k_iir_cascade_planarIL": 2, r"25k_iir_cascade_pipe_planarIL": 2}
    for pat, count in want.items():
        df.rounds_separately(asm, pat, count)


def test_header_table_and_library_agree_on_the_planar_entries():
    native_of = {"rspt_hip_iir_%s_planar_%s_dev" % (stage, form): "rspt_hip_iir_%s_%s_dev" % (stage, form) for stage in ("prefilter", "cascade") for form in ("batch", "stream")}
    single = "int rspt_hip_iir_prefilter_planar_%s_dev(rspt_hip_packer* p, int32_t* d_planar, size_t nblocks, const double* n, const double* d, size_t nr_coefficients, int init_nr_samples, %svoid* stream);"
    cascade = ("int rspt_hip_iir_cascade_planar_%s_dev(rspt_hip_packer* p, int32_t* d_planar, size_t nblocks, size_t nsections, const double* n, const double* d, "
               "const uint32_t* nr_coefficients, const int32_t* init_nr_samples, const uint8_t* use_filter, %svoid* stream);")
    df.check_entries((single % ("batch", "int per_channel, "), single % ("stream", "void* d_state, "), cascade % ("batch", ""), cascade % ("stream", "void* d_state, ")),
                     list(native_of), native_of)


def test_argument_checks_that_need_no_device():
    from rspt_amd import api

    L = api.lib()
    k = (C.c_double * 10)(*([1.0, 0.5, 0.25, 0.0, 0.0] * 2))
    nc, init = (C.c_uint32 * 2)(3, 3), (C.c_int32 * 2)(0, 0)
    buf = C.create_string_buffer(4096)
    sp = (C.addressof(buf) + 7) & ~7
    assert L.rspt_hip_iir_prefilter_planar_batch_dev(None, sp, 1, k, k, 3, 1, 1, None) == ERR_ARG
    assert L.rspt_hip_iir_prefilter_planar_stream_dev(None, sp, 1, k, k, 3, 1, sp, None) == ERR_ARG
    assert L.rspt_hip_iir_cascade_planar_batch_dev(None, sp, 1, 2, k, k, nc, init, None, None) == ERR_ARG
    assert L.rspt_hip_iir_cascade_planar_stream_dev(None, sp, 1, 2, k, k, nc, init, None, sp, None) == ERR_ARG


# ---- GPU ----

def _what(c):
    return df.what(c, hide=("data", "planar"))


def _call(pk, c, view, state=None, stream=None):
    """the case's stage through its planar entry on the blocks of `view`"""
    if "n" in c:  # the single stage (a cascade case holds its sections only)
        pk.iir_prefilter_planar_batch(view, c["n"], c["d"], init_nr_samples=c["init"], per_channel=state is not None or not c["shared"], state=state, stream=stream)
    else:
        pk.iir_cascade_planar_batch(view, c["sections"], state=state, stream=stream)


def _run(api, c, P, want, rings, calls, off, what):
    """c on P through `calls` (None: one stateless call; else blocks per call on a fresh state) -> (output, x, y rings or None)"""
    import torch

    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    raw, view = df.guarded_matrix(P, off)
    state, S = None, len(pc.sections_of(c))
    if calls is None:
        _call(pk, c, view)
    else:
        state = pk.iir_state() if "n" in c else pk.iir_cascade_state(S)
        assert state.numel() == 88 * c["nch"] * S and int(state.count_nonzero()) == 0
        b0 = 0
        for k in calls:
            _call(pk, c, view[b0 : b0 + k], state=state)
            b0 += k
        assert b0 == P.shape[0]
    torch.cuda.synchronize()
    got = view.cpu().numpy()
    assert df.guards_untouched(raw, off, P.size * 4), (what, "guards", _what(c))
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, "output: %d differ, first at [block, channel, sample] %s" % (len(bad), bad[:1].tolist()), _what(c))
    out = (got, None, None)
    if state is not None:
        x, y, started = state_rings(state, c["nch"], S)
        assert (started == 1).all(), (what, "started", _what(c))
        for k, (mx, my) in enumerate(rings):
            nc = mx.shape[0]
            assert same_doubles(x[:, k, :nc].T, mx), (what, "x ring of section %d" % k, _what(c))
            assert same_doubles(y[:, k, :nc].T, my), (what, "y ring of section %d" % k, _what(c))
        out = (got, x, y)
    pk.close()
    return out


def _sweep_leg(api, leg):
    for c in sw.sweep_cases()[leg]:
        want, rec, P = pc.sweep_expected(c), sw.record()[c["name"]], pc.sweep_planar(c)
        off = 4 * c["off"]
        if leg in sw.STREAM_LEGS:
            rings = sw.want(leg, c["name"])[1]
            assert all(L % c["ns"] == 0 for L in c["calls"])
            cutup = _run(api, c, P, want, rings, [L // c["ns"] for L in c["calls"]], off, "cut")
            whole = _run(api, c, P, want, rings, [c["nblocks"]], off, "one_call")
            for k, (mx, _) in enumerate(rings):  # however it is cut: the same first nc places
                nc = mx.shape[0]
                assert same_doubles(cutup[1][:, k, :nc], whole[1][:, k, :nc]) and same_doubles(cutup[2][:, k, :nc], whole[2][:, k, :nc]), ("cut invariance", _what(c))
            got = cutup[0]
        else:
            got = _run(api, c, P, want, None, None, off, "stateless")[0]
        assert digest(pc.cut(got, c["bps"])) == rec["digest"], ("record", _what(c))


@pytest.mark.gpu
def test_gpu_single_sweep_planar(api):
    _sweep_leg(api, "single")


@pytest.mark.gpu
def test_gpu_cascade_sweep_planar(api):
    _sweep_leg(api, "cascade")


@pytest.mark.gpu
def test_gpu_single_stream_sweep_planar(api):
    _sweep_leg(api, "single_stream")


@pytest.mark.gpu
def test_gpu_cascade_stream_sweep_planar(api):
    _sweep_leg(api, "cascade_stream")


def _cases(api, C):
    for c in C:
        want, rings = pc.expected(c)
        if c["calls"]:
            cutup = _run(api, c, c["planar"], want, rings, c["calls"], c["off"], "cut")
            whole = _run(api, c, c["planar"], want, rings, [c["nblocks"]], c["off"], "one_call")
            for k, (mx, _) in enumerate(rings):
                nc = mx.shape[0]
                assert same_doubles(cutup[1][:, k, :nc], whole[1][:, k, :nc]) and same_doubles(cutup[2][:, k, :nc], whole[2][:, k, :nc]), ("cut invariance", _what(c))
        else:
            _run(api, c, c["planar"], want, None, None, c["off"], "stateless")


@pytest.mark.gpu
def test_gpu_stateless_row_ends(api):
    _cases(api, pc.row_cases())


@pytest.mark.gpu
def test_gpu_stream_block_boundaries(api):
    _cases(api, pc.stream_cases())


@pytest.mark.gpu
def test_gpu_plain_kernel_routes(api):
    _cases(api, pc.route_cases())


@pytest.mark.gpu
def test_gpu_values_outside_the_sample_width_are_filtered_whole_and_stored_uncut(api):
    _cases(api, pc.width_cases())


@pytest.mark.gpu
def test_gpu_native_and_planar_calls_alternate_on_one_state(api):
    """bps = 4: one recording in four calls -- native, planar, planar, native -- gives the all-native run's output and rings; with
    one section the state moves between the single and the cascade entries as well"""
    import torch

    nch, ns, cuts = 3, 40, (1, 2, 3, 2)  # 40 rows (the plain kernels), then 80, 120, 80
    nb = sum(cuts)
    P = pc.block(nb, nch, ns, 1001, 1 << 28)
    n, d = BANDPASS
    sections = [(n, d, 7, False)]
    pk = api.new_hzr(4, nch, ns)
    bb = pk.block_bytes

    def drive(plan):
        """plan: per call (layout, entry); the recording lives in the native layout and a planar call converts on the host"""
        rec = pc.native_of(P).reshape(nb, bb).copy()
        state = pk.iir_state()
        b0 = 0
        for k, (layout, entry) in zip(cuts, plan):
            if layout == "native":
                buf = torch.from_numpy(rec[b0 : b0 + k]).cuda()
                if entry == "single":
                    pk.iir_prefilter_batch(buf, n, d, init_nr_samples=7, per_channel=True, state=state)
                else:
                    pk.iir_cascade_batch(buf, sections, state=state)
                torch.cuda.synchronize()
                rec[b0 : b0 + k] = buf.cpu().numpy()
            else:
                rows = rec[b0 : b0 + k].reshape(-1).view("<i4").reshape(k * ns, nch)
                raw, view = df.guarded_matrix(pc.planar_of(rows, k, nch, ns), 4)
                if entry == "single":
                    pk.iir_prefilter_planar_batch(view, n, d, init_nr_samples=7, per_channel=True, state=state)
                else:
                    pk.iir_cascade_planar_batch(view, sections, state=state)
                torch.cuda.synchronize()
                assert df.guards_untouched(raw, 4, view.numel() * 4)
                rec[b0 : b0 + k] = pc.native_of(view.cpu().numpy()).reshape(k, bb)
            b0 += k
        return rec, state.cpu().numpy()

    want, want_state = drive([("native", "single")] * 4)
    c = dict(kind="single", name="alternate", nch=nch, ns=ns, nblocks=nb, planar=P, calls=cuts, n=n, d=d, init=7, shared=False)
    model = pc.stream_expected(c)[0]
    assert np.array_equal(want.reshape(-1), pc.native_of(model))  # (the all-native run is the model's)
    for plan in ([("native", "single"), ("planar", "single"), ("planar", "single"), ("native", "single")],
                 [("planar", "single"), ("planar", "cascade"), ("native", "cascade"), ("planar", "single")],
                 [("planar", "cascade"), ("native", "single"), ("planar", "single"), ("planar", "cascade")]):
        got, got_state = drive(plan)
        assert np.array_equal(got, want), plan
        assert np.array_equal(got_state, want_state), plan
    pk.close()


def _streams(d_dst, d_sizes):
    import torch

    torch.cuda.synchronize()
    sizes = d_sizes.cpu().numpy().astype(np.uint64)
    dst = d_dst.cpu().numpy()
    assert not any(int(s) >> 63 for s in sizes)
    return [dst[i, : int(s)].tobytes() for i, s in enumerate(sizes)]


@pytest.mark.gpu
def test_gpu_reference_pipeline_to_planar_iir_compress_planar(api, orc):
    """compress_planar_batch(iir_prefilter_planar_batch(to_planar_i32(X))) with the harness's band-pass: shared mode against the
    oracle's filter and packer, per-channel mode against the GPU's own native path, byte for byte"""
    import torch

    from rspt_amd import synth

    ns = 2048
    recordings = [(3, 3, np.frombuffer(synth.data_stream_3ch_i24(), dtype=np.uint8)), (4, 12, np.frombuffer(synth.ecg_12ch_i32(), dtype=np.uint8)),
                  (1, 5, cases._rand_native(5, 3 * ns, 1, 4242, 100, walk=True)), (2, 7, cases._rand_native(7, 3 * ns, 2, 4243, 20000, walk=True))]
    n, d = BANDPASS
    new = {"xdelta_hzr": lambda bps, nch: api.new_xdelta_hzr(bps, nch, ns, 3), "hzr": lambda bps, nch: api.new_hzr(bps, nch, ns)}
    for bps, nch, data in recordings:
        bb = bps * nch * ns
        for kind in ("xdelta_hzr", "hzr"):
            for B in (1, 3):
                X = np.array(data[: B * bb]).reshape(B, bb)
                what = (kind, bps, nch, B)
                # shared mode (the harness): the oracle's filter, then its packer, block after block on one packer object
                po = orc.packer(kind, bps, nch, ns, 3)
                want = [po.compress(np.frombuffer(orc.iir_prefilter(X[b], bps, nch, ns, n, d, 2000, shared_state=True), dtype=np.uint8)) for b in range(B)]
                pk = new[kind](bps, nch)
                P = pk.to_planar_i32(torch.from_numpy(X).cuda())
                pk.iir_prefilter_planar_batch(P, n, d, init_nr_samples=2000, per_channel=False)
                assert _streams(*pk.compress_planar_batch(P)) == want, ("shared", what)
                pk.close()
                # per channel: the GPU's own native path
                pn, pp = new[kind](bps, nch), new[kind](bps, nch)
                native = _streams(*pn.compress_batch(pn.iir_prefilter_batch(torch.from_numpy(X).cuda(), n, d, init_nr_samples=2000, per_channel=True)))
                P = pp.to_planar_i32(torch.from_numpy(X).cuda())
                pp.iir_prefilter_planar_batch(P, n, d, init_nr_samples=2000, per_channel=True)
                assert _streams(*pp.compress_planar_batch(P)) == native, ("per_channel", what)
                pn.close()
                pp.close()


@pytest.mark.gpu
def test_gpu_planar_entries_refuse_what_the_native_ones_refuse(api):
    import torch

    L = api.lib()
    nch, ns = 3, 100
    pk = api.new_hzr(2, nch, ns)
    P = pc.block(2, nch, ns, 77)
    raw, view = df.guarded_matrix(P, 0)
    before = raw.clone()
    h, st = pk._h, torch.cuda.current_stream().cuda_stream
    state = torch.zeros(88 * nch * 4 + 8, dtype=torch.uint8, device="cuda")
    NULL = object()
    dp = C.POINTER(C.c_double)
    coef = np.tile(np.array([1.0, -0.5, 0.1, 0.0, 0.0]), 4)

    def single(nc=3, init=2, nblocks=2, p=view.data_ptr(), state_ptr=None, stream_form=False, n=None, d=None, handle=h):
        a = [handle, p, nblocks, None if n is NULL else coef.ctypes.data_as(dp), None if d is NULL else coef.ctypes.data_as(dp), nc, init]
        if stream_form:
            return L.rspt_hip_iir_prefilter_planar_stream_dev(*a, state_ptr, st)
        return L.rspt_hip_iir_prefilter_planar_batch_dev(*a, 1, st)

    def cascade(S=2, nc=(3, 3, 3, 3), init=(2, 0, 0, 0), nblocks=2, p=view.data_ptr(), state_ptr=None, stream_form=False, n=None, d=None, ncp=None, initp=None, handle=h):
        ncs, inits = np.array(nc, dtype=np.uint32), np.array(init, dtype=np.int32)
        a = [handle, p, nblocks, S, None if n is NULL else coef.ctypes.data_as(dp), None if d is NULL else coef.ctypes.data_as(dp),
             None if ncp is NULL else ncs.ctypes.data_as(C.POINTER(C.c_uint32)), None if initp is NULL else inits.ctypes.data_as(C.POINTER(C.c_int32)), None]
        if stream_form:
            return L.rspt_hip_iir_cascade_planar_stream_dev(*a, state_ptr, st)
        return L.rspt_hip_iir_cascade_planar_batch_dev(*a, st)

    too_many = (1 << 31) // nch + 1  # nblocks * nch >= 2^31
    too_long = ((1 << 31) - (1 << 17)) // ns + 1  # a stream call of 2^31 - 2^17 rows and more
    for sf, sp in ((False, None), (True, state.data_ptr())):
        kw = dict(stream_form=sf, state_ptr=sp)
        for call in (single, cascade):
            assert call(p=None, **kw) == ERR_ARG and call(n=NULL, **kw) == ERR_ARG and call(d=NULL, **kw) == ERR_ARG
            assert call(nblocks=0, **kw) == ERR_ARG and call(nblocks=too_many, **kw) == ERR_ARG
            assert call(handle=None, **kw) == ERR_ARG
            for k in (1, 2, 3):  # off the 4-byte alignment
                assert call(p=view.data_ptr() + k, **kw) == ERR_ARG
        assert single(nc=1, **kw) == ERR_ARG and single(nc=6, **kw) == ERR_ARG
        assert single(init=-1, **kw) == ERR_ARG and single(init=(1 << 28) + 1, **kw) == ERR_ARG
        assert cascade(S=0, **kw) == ERR_ARG and cascade(S=5, **kw) == ERR_ARG
        assert cascade(nc=(3, 1, 3, 3), **kw) == ERR_ARG and cascade(nc=(6, 3, 3, 3), **kw) == ERR_ARG
        assert cascade(init=(0, -1, 0, 0), **kw) == ERR_ARG and cascade(init=((1 << 28) + 1, 0, 0, 0), **kw) == ERR_ARG
        assert cascade(ncp=NULL, **kw) == ERR_ARG and cascade(initp=NULL, **kw) == ERR_ARG
    for call in (single, cascade):
        assert call(stream_form=True, state_ptr=None) == ERR_ARG and call(stream_form=True, state_ptr=state.data_ptr() + 4) == ERR_ARG
        assert call(stream_form=True, state_ptr=state.data_ptr(), nblocks=too_long) == ERR_UNSUPPORTED
    wide = api.new_hzr(1, 8192, 4)  # more than 8191 channels
    wbuf = torch.zeros(8192 * 4, dtype=torch.int32, device="cuda")
    wstate = torch.zeros(88 * 8192 * 2, dtype=torch.uint8, device="cuda")
    for call in (single, cascade):
        assert call(handle=wide._h, p=wbuf.data_ptr(), nblocks=1) == ERR_UNSUPPORTED
        assert call(handle=wide._h, p=wbuf.data_ptr(), nblocks=1, stream_form=True, state_ptr=wstate.data_ptr()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(raw, before) and int(state.count_nonzero()) == 0 and int(wbuf.count_nonzero()) == 0 and int(wstate.count_nonzero()) == 0
    wide.close()
    with pytest.raises(ValueError):
        pk.iir_prefilter_planar_batch(view, [1.0, 0.5], [1.0, 0.5], per_channel=False, state=state)
    with pytest.raises(ValueError):
        pk.iir_cascade_planar_batch(view, [])
    with pytest.raises(AssertionError):
        pk.iir_prefilter_planar_batch(view.view(torch.uint8), [1.0, 0.5], [1.0, 0.5])  # (not an int32 tensor)
    # accepted: the extremes, on a handle whose bps is not 4
    assert single(nc=2) == 0 and single(nc=5, init=0) == 0 and cascade(S=4, nc=(5, 2, 5, 2), stream_form=True, state_ptr=state.data_ptr()) == 0
    torch.cuda.synchronize()
    assert df.guards_untouched(raw, 0, P.size * 4)
    pk.close()


@pytest.mark.gpu
def test_gpu_planar_entries_run_on_a_foreign_stream(api):
    import torch

    s = torch.cuda.Stream()
    picks = [next(c for c in pc.row_cases() if c["kind"] == "single" and not c["shared"] and c["ns"] == 129),
             next(c for c in pc.row_cases() if c["kind"] == "cascade" and c["ns"] == 129),
             next(c for c in pc.stream_cases() if c["kind"] == "single" and c["ns"] == 100),
             next(c for c in pc.stream_cases() if c["kind"] == "cascade" and c["ns"] == 100)]
    for c in picks:
        want = pc.expected(c)[0]
        pk = api.new_hzr(4, c["nch"], c["ns"])
        raw, view = df.guarded_matrix(c["planar"], c["off"])
        state = None
        if c["calls"]:
            state = pk.iir_state() if c["kind"] == "single" else pk.iir_cascade_state(len(c["sections"]))
        s.wait_stream(torch.cuda.current_stream())
        b0 = 0
        for k in c["calls"] or [c["nblocks"]]:
            _call(pk, c, view[b0 : b0 + k], state=state, stream=s.cuda_stream)
            b0 += k
        s.synchronize()
        assert np.array_equal(view.cpu().numpy(), want) and df.guards_untouched(raw, c["off"], view.numel() * 4), _what(c)
        pk.close()
