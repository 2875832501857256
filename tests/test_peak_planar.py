"""Both R-peak detectors on the planar int32 matrix: rspt_hip_peak_detect_planar_batch_dev and
rspt_hip_peak_detect_offline_planar_batch_dev.

CPU: the record's inputs, the numpy restatements (tests/peak_cases.py, tests/peak_offline_cases.py) against the compiled
reference's answers on int32 matrices (tests/golden/peak_planar_record.json), the native records' cases as matrices, what the
cases cover, the C ABI, and the planar kernels' ISA (no fused multiply-add).
GPU (-m gpu): bit-exact against the record on every case, the identity with the native entries, guards, base offsets, options,
carried state, the workspace, streams, refusals and the pipeline behind the planar zero-phase filter."""
import ctypes as C
import functools

import numpy as np
import pytest

import cases
import devframe as df
import peak_cases as pc
import peak_offline_cases as oc
import peak_planar_cases as pp
from devframe import ERR_ARG, ERR_UNSUPPORTED, api, asm  # noqa: F401

ONLINE_ENTRY, OFFLINE_ENTRY = "rspt_hip_peak_detect_planar_batch_dev", "rspt_hip_peak_detect_offline_planar_batch_dev"

CASES = pp.recorded_cases()
NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def _golden(which):
    return {r["name"]: r for r in df.golden(which)["cases"]}


def _rec(name):
    """a case of the record, the marker -1.0 events filled in where the record says they are the marker 1.0 run's (null)"""
    r = dict(_golden("peak_planar_record.json")[name])
    for k in ("count", "index"):
        if r[k + "_m1"] is None:
            r[k + "_m1"] = r[k]
    return r


@functools.lru_cache(maxsize=None)
def _restated(name, marker):
    return pp.expected(BY_NAME[name], marker)


def _mismatch(got, want):
    return [k for k in pp.RECORD_KEYS if got[k] != want[k]]


# ---- CPU ----

def test_record_inputs_have_not_drifted():
    rec = _golden("peak_planar_record.json")
    assert list(rec) == NAMES and len(set(NAMES)) == len(NAMES)
    for c in CASES:
        r = rec[c["name"]]
        assert (c["kind"], c["variant"], c["fs"], c["bps"], c["nch"], c["ns"], c["nblocks"], c["stateful"], c["calls"]) == (
            r["kind"], r["variant"], r["fs"], r["bps"], r["nch"], r["ns"], r["nblocks"], r["stateful"], r["calls"]), c["name"]
        assert pp.crc(pp.matrix_bytes(c["planar"])) == r["in_crc32"], c["name"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_reference_on_int32_matrices(name):
    got = pp.summarize(_restated(name, 1.0), _restated(name, -1.0))
    assert not _mismatch(got, _rec(name)), (name, _mismatch(got, _rec(name)))


def test_native_record_cases_as_matrices_are_the_native_records_inputs():
    """a native case's matrix is its samples transposed: back in the native layout it has the crc the native record was taken on,
    so that record's results are what the planar entries must give on the matrix"""
    seen = set()
    for c, rec in pp.native_cases():
        r = _golden(rec)[c["name"]]
        X = pp.rows_of(c["planar"])
        back = np.concatenate([pc.i32_to_native(X[b], c["bps"]) for b in range(c["nblocks"])])
        assert pc.crc(back) == r["in_crc32"] and c["planar"].shape == (r["nblocks"], r["nch"], r["ns"]), c["name"]
        seen.add((c["kind"], r["fs"], r["ns"]))
    assert {("online", 2000.0, 34199), ("offline", 250.0, 34199), ("offline", 1000.0, 6000)} <= seen


def test_the_cases_cover_what_they_must():
    def of(group):
        return [c for c in CASES if c["group"] == group]

    for kind in ("online", "offline"):
        assert {c["ns"] for c in of("len") if c["kind"] == kind} == set(pp.ROW_LENGTHS)
        assert {c["nblocks"] * c["nch"] for c in of("rows") if c["kind"] == kind} == set(pp.ROW_COUNTS)
        assert {c["ns"] % 4 for c in of("rows") if c["kind"] == kind} == {0, 1}
        st = {(c["nch"], c["nblocks"]) for c in of("state") if c["kind"] == kind and c["calls"] is None}
        assert st == {(n, b) for n in pp.STATE_NCH for b in pp.STATE_NBLOCKS}
        assert all(c["stateful"] for c in of("state")) and not any(c["stateful"] for c in of("len") + of("rows"))
        assert {c["bps"] for c in of("width") if c["kind"] == kind} == {1, 2, 3}
        assert {c["off"] for c in CASES if c["kind"] == kind and c["ns"] % 4 == 0} == set(pp.BASE_OFFSETS)
        assert {c["off"] for c in CASES if c["kind"] == kind and c["ns"] % 4} == set(pp.BASE_OFFSETS)
    assert {r % 4 for r in pp.ROW_LENGTHS} == {0, 1, 2, 3} and {15, 16, 17} <= set(pp.ROW_LENGTHS)
    for g in ("len", "rows", "state", "events"):
        assert {c["variant"] for c in of(g) if c["kind"] == "online"} == set(pc.VARIANTS.values()), g
    assert {c["name"].split("1x")[0] for c in of("moved")} == {"trispikes", "burst", "ramps"} and all(c["kind"] == "offline" for c in of("moved"))
    assert any(c["calls"] and {"fw", "detect"} == set(c["calls"]) for c in of("state"))
    # events on the long rows, at the native cases' rates; events on rows of every short length too
    assert {250.0, 360.0, 500.0, 1000.0, 2000.0} <= {c["fs"] for c in of("events")}
    assert all(sum(_rec(c["name"])["count"]) >= 2 * c["nblocks"] * c["nch"] - 4 for c in of("events"))  # (about two a row or more)
    assert all(sum(_rec(c["name"])["count"]) > 0 for c in of("len") if c["kind"] == "online" and c["ns"] > 3)
    assert all(sum(_rec(c["name"])["count"]) > 0 for c in of("rows") + of("moved") + of("width"))
    # the widths: values outside the handle's width, both ends of int32 among them
    for c in of("width"):
        lim = 1 << (8 * c["bps"] - 1)
        assert c["planar"].max() == pp.INT32_MAX and c["planar"].min() == pp.INT32_MIN and (np.abs(c["planar"].astype(np.int64)) >= lim).mean() > 0.01
    # the options of the GPU runs
    assert set(pp.MARKERS) == {1.0, -1.0} and set(pp.MAX_PEAKS) == {0, 1, None} and set(pp.TRACES) == {True, False}
    assert set(pp.BASE_OFFSETS) == {0, 4, 8, 12}


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["group"] == "width"])
def test_cut_to_the_handles_width_the_answer_is_another(name):
    """what from_planar_i32 + the native entry would see: without this difference the width cases would prove nothing"""
    c = BY_NAME[name]
    cut = pp.cut_to_width(c["planar"], c["bps"])
    assert not np.array_equal(cut, c["planar"])
    got = pp.summarize(pp.expected(c, 1.0, cut), pp.expected(c, -1.0, cut))
    assert {"sig", "thr"} <= set(_mismatch(got, _rec(name))) and (got["index"] != _rec(name)["index"] or got["values_m1"] != _rec(name)["values_m1"])


def test_header_table_and_library_agree_on_both_entries():
    df.check_entries(("int rspt_hip_peak_detect_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, int variant, double sampling_rate, "
                      "double marker_val, void* d_state, uint32_t* d_count, int32_t* d_index, double* d_value, size_t max_peaks, double* d_sig, "
                      "double* d_threshold, void* stream);",
                      "int rspt_hip_peak_detect_offline_planar_batch_dev(rspt_hip_packer* p, const int32_t* d_planar, size_t nblocks, double sampling_rate, "
                      "double marker_val, void* d_state, void* d_work, uint32_t* d_count, int32_t* d_index, double* d_value, size_t max_peaks, "
                      "double* d_sig, double* d_threshold, void* stream);"),
                     (ONLINE_ENTRY, OFFLINE_ENTRY),  # (the native sibling's arguments, the matrix in place of the batch)
                     native_of={ONLINE_ENTRY: "rspt_hip_peak_detect_batch_dev", OFFLINE_ENTRY: "rspt_hip_peak_detect_offline_batch_dev"},
                     methods=("peak_detect_planar_batch", "peak_detect_offline_planar_batch"))
    assert "stay native-only" not in df.header().replace("(compress, _many, the feed) stay native-only", "")


def test_argument_checks_that_need_no_device():
    """a NULL handle is refused before anything touches a device, whatever else is passed"""
    from rspt_amd import api

    L = api.lib()
    buf = C.create_string_buffer(4096)
    b = (C.addressof(buf) + 15) & ~15
    assert L.rspt_hip_peak_detect_planar_batch_dev(None, b, 1, 0, 500.0, 1.0, None, b + 1024, b + 2048, b + 3072, 1, None, None, None) == ERR_ARG
    assert L.rspt_hip_peak_detect_offline_planar_batch_dev(None, b, 1, 500.0, 1.0, None, b + 512, b + 1024, b + 2048, b + 3072, 1, None, None, None) == ERR_ARG
    assert buf.raw == bytes(4096)


def test_the_planar_peak_kernels_hold_no_fused_multiply_add(asm):
    """k_peak_planar (3 variants x traces on / off) and k_peak_offline_planar (traces on / off): every product and sum with
    v_mul_f64 and v_add_f64, as in the native kernels"""
    for pat, n in ((r"13k_peak_planarIL", 6), (r"21k_peak_offline_planarIL", 2)):
        df.rounds_separately(asm, pat, n, fused=df.FUSED_F64)


# ---- GPU ----

def _run(api, pk, c, view, marker=1.0, max_peaks=None, traces=True, state=None, work_fill=0xFF, stream=None, kind=None, variant=None,
         trace_off=8):
    """One call of a planar entry through the C ABI on buffers of the test's own, every one between guards (the traces 8 bytes
    past a 16-byte boundary): the guards are checked, and the result comes back as peak_cases.detect returns it, the traces
    transposed to [nblocks][ns][nch].  kind / variant: of the call, where they are not the case's."""
    import torch

    kind = kind or c["kind"]
    variant = c["variant"] if variant is None else variant
    nblocks, nch, ns = view.shape
    rows = nblocks * nch
    mp = ns if max_peaks is None else max_peaks
    L = api.lib()
    st = torch.cuda.current_stream().cuda_stream if stream is None else stream
    craw, count = df.guarded(rows * 4)
    iraw, index = df.guarded(rows * mp * 4)
    vraw, value = df.guarded(rows * mp * 8)
    sraw, sig = df.guarded(rows * ns * 8 if traces else 0, trace_off)
    hraw, thr = df.guarded(rows * ns * 8 if traces else 0, trace_off)
    ptr = lambda t: t.data_ptr() if t.numel() else None  # noqa: E731
    sp = state.data_ptr() if state is not None else None
    if kind == "online":
        rc = L.rspt_hip_peak_detect_planar_batch_dev(pk._h, view.data_ptr(), nblocks, variant, c["fs"], marker, sp, count.data_ptr(), ptr(index),
                                                     ptr(value), mp, ptr(sig), ptr(thr), st)
    else:
        wb = pk.peak_offline_work_bytes(nblocks, state is not None)
        wraw, work = df.guarded(wb, 0, work_fill)
        rc = L.rspt_hip_peak_detect_offline_planar_batch_dev(pk._h, view.data_ptr(), nblocks, c["fs"], marker, sp, work.data_ptr(), count.data_ptr(),
                                                             ptr(index), ptr(value), mp, ptr(sig), ptr(thr), st)
    assert rc == 0, (rc, c["name"])
    if stream is None:
        torch.cuda.synchronize()
    else:
        torch.cuda.ExternalStream(stream).synchronize()
    what = (c["name"], kind, marker, max_peaks, traces)
    assert df.guards_untouched(craw, 0, rows * 4) and df.guards_untouched(iraw, 0, rows * mp * 4) and df.guards_untouched(vraw, 0, rows * mp * 8), what
    assert df.guards_untouched(sraw, trace_off, sig.numel()) and df.guards_untouched(hraw, trace_off, thr.numel()), what
    if kind == "offline":
        assert df.guards_untouched(wraw, 0, wb), what
    out = [count.view(torch.int32).reshape(nblocks, nch), index.view(torch.int32).reshape(nblocks, nch, mp), value.view(torch.float64).reshape(nblocks, nch, mp)]
    if traces:
        out += [t.view(torch.float64).reshape(nblocks, nch, ns).transpose(1, 2).contiguous() for t in (sig, thr)]
    return pc.to_result(out, mp, traces)


def _check_case(api, c, want, off=None, keys=pp.RECORD_KEYS):
    """c on a matrix at `off`, marker 1.0 with traces and marker -1.0 without, against the record fields `want`"""
    off = c["off"] if off is None else off
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    raw, view = df.guarded_matrix(c["planar"], off)
    before = raw.clone()
    new_state = (lambda: pk.peak_state()) if c["stateful"] else (lambda: None)
    if c["calls"] is None:
        r = _run(api, pk, c, view, 1.0, state=new_state())
        m = _run(api, pk, c, view, -1.0, traces=False, state=new_state())
    else:
        r, m = (_alternating(api, pk, c, view, marker, tr) for marker, tr in ((1.0, True), (-1.0, False)))
    import torch

    assert torch.equal(raw, before), ("the matrix changed", c["name"])
    assert all(v == 1.0 for v in pc.flat(r["value"])), c["name"]
    got = dict(pp.summarize(r, dict(m, sig=r["sig"], thr=r["thr"])))
    bad = [k for k in keys if got[k] != want[k]]
    assert not bad, (c["name"], off, bad)
    pk.close()


def _alternating(api, pk, c, view, marker, traces):
    """a stateful offline case with calls: block b through the online entry (OFFLINE_FW) or the offline one, on one state"""
    st = pk.peak_state()
    parts = [_run(api, pk, c, view[b : b + 1], marker, traces=traces, state=st, kind="online" if k == "fw" else "offline", variant=pc.OFFLINE_FW)
             for b, k in enumerate(c["calls"])]
    return _join(parts, traces)


def _join(parts, traces=True):
    r = {k: [row for p in parts for row in p[k]] for k in ("count", "index", "value")}
    if traces:
        r["sig"], r["thr"] = (np.concatenate([p[k] for p in parts]) for k in ("sig", "thr"))
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_every_case_matches_the_record(api, name):
    _check_case(api, BY_NAME[name], _rec(name))


@pytest.mark.gpu
def test_gpu_native_record_cases_as_matrices(api):
    """the planar entries on the native records' inputs, transposed: the native records' events, values and trace digests"""
    for k, (c, rec) in enumerate(pp.native_cases()):
        want = _golden(rec)[c["name"]]
        keys = [key for key in pp.RECORD_KEYS if key in want]
        _check_case(api, c, want, off=pp.BASE_OFFSETS[k % 4], keys=keys)


@pytest.mark.gpu
def test_gpu_identity_with_the_native_entry_for_every_width_and_byte_order(api):
    """peak_planar(to_planar_i32(X)) == peak_native(X), the traces transposed.  The native entry reads little-endian samples
    whatever the handle's byte order; a big-endian handle's converter sees the same samples reversed"""
    import torch

    nch, ns, B, fs = 5, 1031, 3, 250.0
    for bps in (1, 2, 3, 4):
        X = np.array(cases._rand_native(nch, B * ns, bps, 8300 + bps, 1 << (8 * bps - 3), walk=True), dtype=np.uint8)
        pk = api.new_hzr(bps, nch, ns)
        src = torch.from_numpy(X).cuda().reshape(B, -1)
        for variant in sorted(pc.VARIANTS) + ["offline"]:
            for stateful in (False, True):
                st = (lambda: pk.peak_state()) if stateful else (lambda: None)
                if variant == "offline":
                    want = pk.peak_detect_offline_batch(src, fs, marker_val=-1.0, max_peaks=ns, state=st(), traces=True)
                else:
                    want = pk.peak_detect_batch(src, variant=variant, sampling_rate=fs, marker_val=-1.0, max_peaks=ns, state=st(), traces=True)
                for be in (False, True):
                    pk.set_byte_order(be)
                    P = pk.to_planar_i32(torch.from_numpy(np.ascontiguousarray(cases.reverse_samples(X, bps) if be else X)).cuda().reshape(B, -1))
                    if variant == "offline":
                        got = pk.peak_detect_offline_planar_batch(P, fs, marker_val=-1.0, max_peaks=ns, state=st(), traces=True)
                    else:
                        got = pk.peak_detect_planar_batch(P, variant=variant, sampling_rate=fs, marker_val=-1.0, max_peaks=ns, state=st(), traces=True)
                    torch.cuda.synchronize()
                    what = (bps, variant, stateful, be)
                    assert got[3].shape == (B, nch, ns) and want[3].shape == (B, ns, nch), what
                    assert torch.equal(got[0], want[0]) and int(got[0].sum()) > 0, what
                    a, b = pc.to_result(got[:3], ns, False), pc.to_result(want[:3], ns, False)
                    pc.events_equal(a, b)
                    for t in (3, 4):
                        assert np.array_equal(pc.canon(got[t].transpose(1, 2).cpu().numpy()), pc.canon(want[t].cpu().numpy())), what
                pk.set_byte_order(False)
        pk.close()


OPTION_CASES = ["len2x3x65_online_fs50", "len2x3x33_online_1st_fs50", "len2x3x200_online_1st_fs50", "len2x3x200_offline_fw_fs50", "ecg2x3x2500_offline_fs250",
                "ecgstate4x3x1000_offline_fs360", "wide1x3x1500_bps2_offline_fs250"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", OPTION_CASES)
def test_gpu_markers_max_peaks_and_traces(api, name):
    """every marker x max_peaks x traces on / off: exact counts whatever is stored, the first max_peaks events, the traces
    whether or not events are stored"""
    c = BY_NAME[name]
    assert c["calls"] is None
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    raw, view = df.guarded_matrix(c["planar"], c["off"])
    for marker in pp.MARKERS:
        want = _restated(name, marker)
        assert max(pc.flat([want["count"]])) > 1
        for mp in pp.MAX_PEAKS:
            for traces in pp.TRACES:
                r = _run(api, pk, c, view, marker, max_peaks=mp, traces=traces, state=pk.peak_state() if c["stateful"] else None)
                pc.events_equal(r, want, c["ns"] if mp is None else mp)
                if traces:
                    assert pc.tdigest(r["sig"]) == _rec(name)["sig"] and pc.tdigest(r["thr"]) == _rec(name)["thr"], (name, marker, mp)
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("off", pp.BASE_OFFSETS)
def test_gpu_matrix_base_at_every_offset_from_a_16_byte_boundary(api, off):
    """rows on 16-byte boundaries only at offset 0 with ns % 4 == 0; every other combination starts rows on other residues"""
    for name in ("rows2x65x48_online_1st_fs150", "rows2x65x37_offline_fw_fs150", "len2x3x64_online_fs50", "len2x3x17_offline_fw_fs50", "rows9x7x48_offline_fs150",
                 "rows9x7x37_offline_fs150", "len2x3x129_offline_fs50", "ecg2x3x2500_online_fs250"):
        _check_case(api, BY_NAME[name], _rec(name), off=off)


@pytest.mark.gpu
def test_gpu_a_row_run_alone_leaves_its_neighbouring_trace_rows_untouched(api):
    """row r of a matrix as a one-row call whose traces go to row r of filled trace matrices: that row is the whole call's, every
    other row and the guards keep the fill -- for rows whose traces start on and off a 16-byte boundary"""
    import torch

    L = api.lib()
    for name in ("len2x3x33_online_fs50", "len2x3x17_offline_fw_fs50", "len2x3x64_online_1st_fs50", "len2x3x15_offline_fs250", "len2x3x200_offline_fs250"):
        c = BY_NAME[name]
        ns, rows = c["ns"], c["nblocks"] * c["nch"]
        whole = _restated(name, 1.0)
        pk = api.new_hzr(4, 1, ns)
        raw, view = df.guarded_matrix(c["planar"], c["off"])
        for toff in (0, 8):
            traws = [df.guarded(rows * ns * 8, toff) for _ in range(2)]
            for r in range(rows):
                b, ch = divmod(r, c["nch"])
                craw, count = df.guarded(4)
                src = view.reshape(rows, ns)[r].data_ptr()
                sp, hp = (t[1].data_ptr() + r * ns * 8 for t in traws)
                st = torch.cuda.current_stream().cuda_stream
                if c["kind"] == "online":
                    rc = L.rspt_hip_peak_detect_planar_batch_dev(pk._h, src, 1, c["variant"], c["fs"], 1.0, None, count.data_ptr(), None, None, 0, sp, hp, st)
                else:
                    work = torch.empty(pk.peak_offline_work_bytes(1), dtype=torch.uint8, device="cuda")
                    rc = L.rspt_hip_peak_detect_offline_planar_batch_dev(pk._h, src, 1, c["fs"], 1.0, None, work.data_ptr(), count.data_ptr(), None, None, 0,
                                                                         sp, hp, st)
                torch.cuda.synchronize()
                assert rc == 0 and df.guards_untouched(craw, 0, 4) and int(count.view(torch.int32)[0]) == whole["count"][b][ch], (name, r)
                for (traw, t), key in zip(traws, ("sig", "thr")):
                    got = t.view(torch.float64).reshape(rows, ns)
                    assert df.guards_untouched(traw, toff, rows * ns * 8), (name, r, toff)
                    assert np.array_equal(pc.canon(got[r].cpu().numpy()), pc.canon(whole[key][b, :, ch])), (name, r, toff, key)
                    later = t.reshape(rows, ns * 8)[r + 1 :]
                    assert int((later != df.FILL).count_nonzero()) == 0, (name, r, toff, key)  # (earlier rows hold their own traces)
        pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(pc.VARIANTS))
def test_gpu_any_cut_of_a_recording_equals_the_uncut_run(api, variant):
    """one recording of 3 channels x 240 samples as one block, as blocks of 120, 48, 15 and 1 samples, in one call or several: the
    same events (indices counted from the recording's start) and the same traces, and the state left behind is the same.
    OFFLINE_FW runs its band-pass history at the head of every block (every detect_fw call), so there the blocks matter and the
    calls do not: the restatement on the same blocks, and one state whatever the calls"""
    import torch

    nch, total, fs = 3, 240, 5.0 if variant != "online" else 50.0
    R = pp._walk(1, nch, total, 4242)[0]  # [nch][total]
    c = dict(name="cut_%s" % variant, kind="online", variant=pc.VARIANTS[variant], fs=fs)
    uncut = pc.detect(pp.rows_of(R[None]), pc.VARIANTS[variant], fs, -1.0, stateful=True)
    assert sum(uncut["count"][0]) > 3
    states = {}
    for ns, calls in ((240, (1,)), (120, (2,)), (120, (1, 1)), (48, (5,)), (48, (2, 3)), (15, (16,)), (15, (7, 1, 8)), (1, (240,)), (1, (100, 140))):
        nb = total // ns
        P = np.ascontiguousarray(R.reshape(nch, nb, ns).transpose(1, 0, 2))
        want = uncut
        if variant == "offline_fw":  # (the same blocks, as one recording)
            w = pc.detect(pp.rows_of(P), pc.OFFLINE_FW, fs, -1.0, stateful=True)
            want = dict(index=[[[b * ns + i for b in range(nb) for i in w["index"][b][ch]] for ch in range(nch)]],
                        value=[[[v for b in range(nb) for v in w["value"][b][ch]] for ch in range(nch)]], sig=w["sig"].reshape(1, total, nch),
                        thr=w["thr"].reshape(1, total, nch))
        pk = api.new_hzr(2, nch, ns)
        raw, view = df.guarded_matrix(P, 4 * (ns % 4))
        st, parts, b0 = pk.peak_state(), [], 0
        for n in calls:
            parts.append(_run(api, pk, c, view[b0 : b0 + n], -1.0, state=st))
            b0 += n
        torch.cuda.synchronize()
        r = _join(parts)
        for ch in range(nch):
            idx = [b * ns + i for b in range(nb) for i in r["index"][b][ch]]
            val = [v for b in range(nb) for v in r["value"][b][ch]]
            assert idx == want["index"][0][ch] and pc.vhex(val) == pc.vhex(want["value"][0][ch]), (variant, ns, calls, ch)
        for key in ("sig", "thr"):
            assert np.array_equal(pc.canon(r[key].reshape(total, nch)), pc.canon(want[key][0])), (variant, ns, calls, key)
        states.setdefault(ns if variant == "offline_fw" else 0, set()).add(st.cpu().numpy().tobytes())
        pk.close()
    assert all(len(v) == 1 for v in states.values())


@pytest.mark.gpu
def test_gpu_one_state_alternates_between_native_and_planar_calls(api):
    """a bps = 4 handle: block b through the native entry (even b) or the planar one (odd b) on one state, online and offline;
    the record's events and traces"""
    import torch

    for name in ("state5x3x33_offline_fw_fs50", "state5x3x33_offline_fs50", "state5x65x33_online_fs150"):
        c = BY_NAME[name]
        nb, nch, ns = c["planar"].shape
        pk = api.new_hzr(4, nch, ns)
        raw, view = df.guarded_matrix(c["planar"], c["off"])
        X = pp.rows_of(c["planar"])
        for marker in (1.0, -1.0):
            st, parts = pk.peak_state(), []
            for b in range(nb):
                if b % 2:
                    parts.append(_run(api, pk, c, view[b : b + 1], marker, state=st))
                    continue
                src = torch.from_numpy(pc.i32_to_native(X[b], 4)).cuda()
                if c["kind"] == "online":
                    out = pk.peak_detect_batch(src, variant=c["variant"], sampling_rate=c["fs"], marker_val=marker, max_peaks=ns, state=st, traces=True)
                else:
                    out = pk.peak_detect_offline_batch(src, c["fs"], marker_val=marker, max_peaks=ns, state=st, traces=True)
                torch.cuda.synchronize()
                parts.append(pc.to_result(out, ns, True))
            r = _join(parts)
            got = pp.summarize(r, r)
            keys = ("count", "index", "sig", "thr") if marker == 1.0 else ("count_m1", "index_m1", "values_m1", "sig", "thr")
            assert [k for k in keys if got[k] != _rec(name)[k]] == [], (name, marker)
        pk.close()


@pytest.mark.gpu
def test_gpu_the_offline_workspace_needs_no_initialisation(api):
    """NaN bytes, zeros and another call's leftovers in the workspace: the same answer"""
    for name in ("rows2x65x37_offline_fs150", "trispikes1x4x4000_offline_fs250", "state2x65x50_offline_fs150"):
        c = BY_NAME[name]
        pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
        raw, view = df.guarded_matrix(c["planar"], c["off"])
        for fill in (0xFF, 0x00, 0x7F):
            r = _run(api, pk, c, view, 1.0, state=pk.peak_state() if c["stateful"] else None, work_fill=fill)
            got = pp.summarize(r, r)
            assert [k for k in ("count", "index", "sig", "thr") if got[k] != _rec(name)[k]] == [], (name, fill)
        pk.close()


@pytest.mark.gpu
def test_gpu_a_repeated_call_gives_the_same_output(api):
    import torch

    for name in ("rows2x65x48_online_1st_fs150", "burst1x3x3000_offline_fs1000"):
        c = BY_NAME[name]
        pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
        raw, view = df.guarded_matrix(c["planar"], c["off"])
        call = pk.peak_detect_planar_batch if c["kind"] == "online" else pk.peak_detect_offline_planar_batch
        kw = dict(variant=c["variant"]) if c["kind"] == "online" else {}
        outs = [call(view, sampling_rate=c["fs"], marker_val=-1.0, max_peaks=c["ns"], traces=True, **kw) for _ in range(3)]
        torch.cuda.synchronize()
        got = pc.to_result([outs[0][0], outs[0][1], outs[0][2]], c["ns"], False)
        pc.events_equal(got, _restated(name, -1.0))
        for o in outs[1:]:
            assert torch.equal(o[0], outs[0][0])
            for t in (3, 4):
                assert o[t].shape == (c["nblocks"], c["nch"], c["ns"]) and np.array_equal(pc.canon(o[t].cpu().numpy()), pc.canon(outs[0][t].cpu().numpy()))
            a, b = pc.to_result(o[:3], c["ns"], False), got
            pc.events_equal(a, b)
        pk.close()


@pytest.mark.gpu
def test_gpu_the_entries_run_on_a_foreign_stream(api):
    import torch

    s = torch.cuda.Stream()
    for name in ("rows5x13x37_online_1st_fs150", "rows5x13x48_offline_fs150"):
        c = BY_NAME[name]
        pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
        raw, view = df.guarded_matrix(c["planar"], c["off"])
        s.wait_stream(torch.cuda.current_stream())
        r = _run(api, pk, c, view, 1.0, stream=s.cuda_stream)
        got = pp.summarize(r, r)
        assert [k for k in ("count", "index", "sig", "thr") if got[k] != _rec(name)[k]] == [], name
        call = pk.peak_detect_planar_batch if c["kind"] == "online" else pk.peak_detect_offline_planar_batch
        kw = dict(variant=c["variant"]) if c["kind"] == "online" else {}
        out = call(view, sampling_rate=c["fs"], max_peaks=c["ns"], stream=s.cuda_stream, **kw)
        s.synchronize()
        assert [v for row in out[0].cpu().numpy().tolist() for v in row] == _rec(name)["count"]
        pk.close()


@pytest.mark.gpu
def test_gpu_values_outside_the_width_go_in_whole_and_the_converter_route_differs(api):
    """handles of bps 1, 2, 3: the planar entries give the record's answer on the int32 values; from_planar_i32 + the native
    entry, which cuts them to the width, gives another"""
    import torch

    for c in (c for c in CASES if c["group"] == "width"):
        pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
        raw, view = df.guarded_matrix(c["planar"], c["off"])
        r = _run(api, pk, c, view, -1.0)
        got = pp.summarize(r, r)
        assert [k for k in ("count_m1", "index_m1", "values_m1", "sig", "thr") if got[k] != _rec(c["name"])[k]] == [], c["name"]
        native = pk.from_planar_i32(view.contiguous())
        if c["kind"] == "online":
            out = pk.peak_detect_batch(native, variant=c["variant"], sampling_rate=c["fs"], marker_val=-1.0, max_peaks=c["ns"], traces=True)
        else:
            out = pk.peak_detect_offline_batch(native, c["fs"], marker_val=-1.0, max_peaks=c["ns"], traces=True)
        torch.cuda.synchronize()
        cutr = pc.to_result(out, c["ns"], True)
        assert pc.tdigest(cutr["sig"]) != _rec(c["name"])["sig"] and pc.vhex(pc.flat(cutr["value"])) != _rec(c["name"])["values_m1"], c["name"]
        pk.close()


@pytest.mark.gpu
def test_gpu_pipeline_behind_the_planar_zero_phase_filter_on_an_int16_handle(api):
    """to_planar_i32 -> iir_zero_phase_planar_batch -> peak_detect_planar_batch / peak_detect_offline_planar_batch on an int16
    handle: the restatement run on the filtered matrix, whose values the filter stored whole (some outside int16)"""
    import torch

    from rspt_amd import synth

    nch, ns, B, fs = 3, 3000, 2, 500.0
    X = np.concatenate([synth.synth_native(nch, ns, 40 + b, bps=2, ecg=True).numpy() for b in range(B)])
    pk = api.new_hzr(2, nch, ns)
    P = pk.to_planar_i32(torch.from_numpy(X).cuda().reshape(B, -1))
    n, d = [1.0, -1.5, 0.7], [4.0, 0.0, -4.0]  # (a resonant band-pass with gain: the output leaves int16)
    pk.iir_zero_phase_planar_batch(P, n, d, init_nr_samples=100)
    torch.cuda.synchronize()
    F = P.cpu().numpy()
    assert (np.abs(F.astype(np.int64)) > 32767).any()
    on = pk.peak_detect_planar_batch(P, variant="online", sampling_rate=fs, marker_val=-1.0, max_peaks=ns, traces=True)
    off = pk.peak_detect_offline_planar_batch(P, fs, marker_val=-1.0, max_peaks=ns, traces=True)
    torch.cuda.synchronize()
    assert np.array_equal(P.cpu().numpy(), F)
    for out, want in ((on, pc.detect(pp.rows_of(F), pc.ONLINE, fs, -1.0)), (off, oc.detect(pp.rows_of(F), fs, -1.0))):
        assert sum(map(sum, want["count"])) > 0
        got = pc.to_result([out[0], out[1], out[2], out[3].transpose(1, 2).contiguous(), out[4].transpose(1, 2).contiguous()], ns, True)
        pc.events_equal(got, want)
        assert pc.tdigest(got["sig"]) == pc.tdigest(want["sig"]) and pc.tdigest(got["thr"]) == pc.tdigest(want["thr"])
    pk.close()


@pytest.mark.gpu
def test_gpu_every_refusal_returns_its_code_and_writes_nothing(api):
    import torch

    L = api.lib()
    nch, ns = 3, 100
    pk = api.new_hzr(2, nch, ns)
    P = pp._walk(2, nch, ns, 77)
    raw, view = df.guarded_matrix(P, 0)
    bufs = {k: df.guarded(n, 8 if k in ("sig", "thr") else 0) for k, n in (("count", 2 * nch * 4), ("index", 2 * nch * 4 * 4), ("value", 2 * nch * 4 * 8),
                                                                         ("sig", 2 * nch * ns * 8), ("thr", 2 * nch * ns * 8), ("state", 208 * nch),
                                                                         ("work", pk.peak_offline_work_bytes(2) + 8))}
    befores = {k: r.clone() for k, (r, _) in bufs.items()}
    mbefore = raw.clone()
    a = {k: v.data_ptr() for k, (_, v) in bufs.items()}
    st = torch.cuda.current_stream().cuda_stream
    h = pk._h

    def on(hh=h, p=view.data_ptr(), nblocks=2, variant=0, fs=500.0, state=None, count=a["count"], index=a["index"], value=a["value"], mp=4,
           sig=a["sig"], thr=a["thr"]):
        return L.rspt_hip_peak_detect_planar_batch_dev(hh, p, nblocks, variant, fs, 1.0, state, count, index, value, mp, sig, thr, st)

    def off(hh=h, p=view.data_ptr(), nblocks=2, fs=500.0, state=None, work=a["work"], count=a["count"], index=a["index"], value=a["value"], mp=4,
            sig=a["sig"], thr=a["thr"]):
        return L.rspt_hip_peak_detect_offline_planar_batch_dev(hh, p, nblocks, fs, 1.0, state, work, count, index, value, mp, sig, thr, st)

    common = (dict(hh=None), dict(p=None), dict(fs=float("nan")), dict(fs=float("inf")), dict(fs=0.0), dict(fs=-5.0), dict(fs=float(1 << 20) * 1.0000001),
              dict(count=None), dict(index=None), dict(value=None), dict(nblocks=0), dict(nblocks=(1 << 31) // nch + 1), dict(sig=None), dict(thr=None),
              dict(mp=(1 << 32) + 1), dict(p=view.data_ptr() + 1), dict(p=view.data_ptr() + 2), dict(p=view.data_ptr() + 3))
    for kw in common:
        assert on(**kw) == ERR_ARG and off(**kw) == ERR_ARG, kw
    assert on(variant=-1) == ERR_ARG and on(variant=3) == ERR_ARG
    assert off(work=None) == ERR_ARG and off(work=a["work"] + 4) == ERR_ARG
    assert off(fs=9.0) == ERR_ARG  # nr_slope_samples 0
    short = api.new_hzr(2, nch, 4)
    assert off(hh=short._h, fs=500.0, nblocks=1) == ERR_ARG  # ns below the relocation radius
    wide = api.new_hzr(1, 8192, 4)  # more than 8191 channels
    wbuf = torch.ones(8192 * 4, dtype=torch.int32, device="cuda")
    wcount = torch.full((8192,), 7, dtype=torch.int32, device="cuda")
    wwork = torch.full((wide.peak_offline_work_bytes(1),), 0xFF, dtype=torch.uint8, device="cuda")
    kw = dict(hh=wide._h, p=wbuf.data_ptr(), nblocks=1, count=wcount.data_ptr(), mp=0, index=None, value=None, sig=None, thr=None)
    assert on(**kw) == ERR_UNSUPPORTED and off(work=wwork.data_ptr(), fs=50.0, **kw) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    # nothing ran: a launch would have written counts, events, traces, a state or the workspace
    assert torch.equal(raw, mbefore) and all(torch.equal(bufs[k][0], befores[k]) for k in bufs)
    assert int((wcount != 7).count_nonzero()) == 0 and int((wwork != 0xFF).count_nonzero()) == 0
    with pytest.raises(AssertionError):
        pk.peak_detect_planar_batch(view.view(torch.uint8), sampling_rate=500.0)  # (not an int32 tensor)
    with pytest.raises(api.RsptHipError) as e:
        pk.peak_detect_planar_batch(view, variant=7, sampling_rate=500.0)
    assert e.value.status == ERR_ARG
    # accepted: the largest rate with counts only; the workspace 8 bytes further on; and a call that runs does show
    assert on(fs=float(1 << 20), mp=0, index=None, value=None, sig=None, thr=None) == 0
    assert off(work=a["work"] + 8) == 0 and on() == 0
    torch.cuda.synchronize()
    assert torch.equal(raw, mbefore) and not torch.equal(bufs["count"][0], befores["count"]) and not torch.equal(bufs["sig"][0], befores["sig"])
    assert torch.equal(bufs["state"][0], befores["state"])
    for k, n in (("count", 2 * nch * 4), ("index", 2 * nch * 4 * 4), ("value", 2 * nch * 4 * 8), ("sig", 2 * nch * ns * 8), ("thr", 2 * nch * ns * 8)):
        assert df.guards_untouched(bufs[k][0], 8 if k in ("sig", "thr") else 0, n), k
    short.close()
    wide.close()
    pk.close()
