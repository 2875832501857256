"""The R-peak detector stage: peak_detector / peak_detector_1st_order / peak_detector_offline::detect_fw of the
reference (lib_rspt/peak_detector.h) on the GPU (rspt_hip_peak_detect_batch_dev), and the Butterworth designer it is built on
(create_filter_iir, lib_rspt/lib_filter/iir_filter_design.cpp) on the host (rspt_hip_design_iir).

CPU: the record's inputs, the numpy restatement (tests/peak_cases.py) against the reference's answers
(tests/golden/peak_record.json), the designer through ctypes, the C ABI, and the kernels' ISA (no fused multiply-add).
GPU (-m gpu): bit-exact against the record and the restatement, fresh and stateful, with and without traces."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import devasm
import devframe as df
import peak_cases as pc
from devframe import ERR_ARG, api  # noqa: F401


@pytest.fixture(scope="module")
def record():
    return df.golden("peak_record.json")


@pytest.fixture(scope="module")
def pcases(record):
    out = {}
    for c, r in zip(pc.peak_cases(), record["cases"]):
        assert c["name"] == r["name"]
        out[c["name"]] = dict(c, rec=r)
    return out


NAMES = [c["name"] for c in pc.peak_cases()]


def summary(r):
    """what the record holds of a restated or GPU result (events of a marker-1.0 run; values_m1: s at the events)"""
    vals = [r["sig"][b, i, c] for b in range(len(r["index"])) for c in range(len(r["index"][b])) for i in r["index"][b][c]]
    return dict(count=[v for row in r["count"] for v in row], index=pc.flat(r["index"]), values_m1=pc.vhex(vals), sig=pc.tdigest(r["sig"]),
                thr=pc.tdigest(r["thr"]))


# ---- CPU ----

def test_record_inputs_have_not_drifted(record):
    assert len(pc.peak_cases()) == len(record["cases"])
    for c, r in zip(pc.peak_cases(), record["cases"]):
        assert (c["name"], c["variant"], c["fs"], c["bps"], c["nch"], c["ns"], c["nblocks"], c["stateful"]) == (
            r["name"], r["variant"], r["fs"], r["bps"], r["nch"], r["ns"], r["nblocks"], r["stateful"])
        assert pc.crc(c["data"]) == r["in_crc32"], c["name"]
    assert [(d["type"], d["order"], d["fs"], d["lo"], d["hi"]) for d in record["designs"]] == [tuple(g) for g in pc.design_grid()]


def test_the_record_covers_what_it_must(record):
    rs = record["cases"]
    assert {r["variant"] for r in rs} == {pc.ONLINE, pc.ONLINE_1ST, pc.OFFLINE_FW}
    assert {r["bps"] for r in rs} == {1, 2, 3, 4}
    assert {500.0, 1000.0, 2000.0, 5.0, 15.0} <= {r["fs"] for r in rs}
    assert {1, 2, 63} <= {r["ns"] for r in rs} and any(r["ns"] % 16 and r["ns"] > 1000 for r in rs)
    assert any(r["stateful"] and r["nblocks"] > 1 for r in rs) and any(not r["stateful"] and r["nblocks"] > 1 for r in rs)
    ecg = {(r["variant"], r["fs"]): sum(r["count"][:1]) for r in rs if r["name"].startswith("ecg12x34199")}
    assert ecg[(pc.ONLINE, 2000.0)] == 26 and ecg[(pc.ONLINE_1ST, 2000.0)] == 25  # channel 0 at 2 kHz
    assert any(sum(r["count"]) > r["nch"] * r["ns"] // 2 for r in rs if r["fs"] == 5.0)  # nr_slope 0: fires often
    assert all(sum(r["count"]) == 0 for r in rs if r["fs"] == 15.0)  # nr_slope 1: never fires
    ds = record["designs"]
    assert {d["n"] for d in ds} == {-1, 2, 3, 5}
    assert any(d["type"] == pc.BAND_STOP and d["order"] == 1 and d["n"] == 3 for d in ds)  # the band_stop quirk
    assert all(d["n"] == -1 for d in ds if d["type"] == pc.BAND_STOP and d["order"] == 2)
    assert all(d["n"] == -1 for d in ds if d["order"] not in (1, 2))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(pcases, name):
    c = pcases[name]
    r = pc.detect(pc.case_i32(c), c["variant"], c["fs"], 1.0, c["stateful"])
    got, want = summary(r), c["rec"]
    for k in ("count", "index", "values_m1", "sig", "thr"):
        assert got[k] == want[k], (name, k)
    assert all(v == 1.0 for v in pc.flat(r["value"]))


def test_restatement_of_the_marker_values():
    """marker -1.0 returns s, any other marker itself -- and a marker of 0.0 is still an event"""
    x = pc.case_i32(pc.peak_cases()[0])[:, :6000, :2]
    base = pc.detect(x, pc.ONLINE, 2000.0, 1.0)
    assert sum(map(sum, base["count"])) > 0
    for m in (-1.0, 0.0, 2.5):
        r = pc.detect(x, pc.ONLINE, 2000.0, m)
        assert r["index"] == base["index"]
        want = [base["sig"][0, i, c] for c in range(2) for i in base["index"][0][c]] if m == -1.0 else [m] * len(pc.flat(base["index"]))
        assert pc.flat(r["value"]) == want


def test_restated_designer_matches_reference(record):
    for d in record["designs"]:
        r = pc.design_iir(d["type"], d["order"], d["fs"], d["lo"], d["hi"])
        if d["n"] < 0:
            assert r is None, d
            continue
        num, den = r
        assert len(num) == d["n"] and pc.vhex(num) == pc.vhex(np.frombuffer(bytes.fromhex(d["num"])))
        assert pc.vhex(den) == pc.vhex(np.frombuffer(bytes.fromhex(d["den"]))), d


def test_c_designer_matches_reference_bit_for_bit(record):
    """rspt_hip_design_iir through ctypes: host only, no device needed; refusals leave the outputs untouched"""
    from rspt_amd import api

    L = api.lib()
    dp = C.POINTER(C.c_double)
    for d in record["designs"]:
        num, den, n = np.full(5, 7.0), np.full(5, 7.0), C.c_size_t(99)
        rc = L.rspt_hip_design_iir(d["type"], d["order"], d["fs"], d["lo"], d["hi"], num.ctypes.data_as(dp), den.ctypes.data_as(dp), C.byref(n))
        if d["n"] < 0:
            assert rc == ERR_ARG and n.value == 99 and (num == 7.0).all() and (den == 7.0).all(), d
        else:
            assert rc == 0 and n.value == d["n"], d
            assert num[: n.value].tobytes().hex() == d["num"] and den[: n.value].tobytes().hex() == d["den"], d
    for t in (-1, 4):
        assert L.rspt_hip_design_iir(t, 1, 500.0, 10.0, 20.0, num.ctypes.data_as(dp), den.ctypes.data_as(dp), C.byref(n)) == ERR_ARG
    assert L.rspt_hip_design_iir(1, 2, 500.0, 10.0, 0.0, None, den.ctypes.data_as(dp), C.byref(n)) == ERR_ARG


def test_api_design_iir():
    from rspt_amd import api

    num, den = api.design_iir("band_pass", 2, 2000.0, 10.0, 20.0)
    want = pc.design_iir(pc.BAND_PASS, 2, 2000.0, 10.0, 20.0)
    assert num.tolist() == want[0] and den.tolist() == want[1] and den[0] == 1.0
    assert [len(a) for a in api.design_iir(0, 1, 500.0, 3.0)] == [2, 2]
    assert [len(a) for a in api.design_iir("band_stop", 1, 500.0, 3.0, 40.0)] == [3, 3]
    with pytest.raises(api.RsptHipError) as e:
        api.design_iir("band_stop", 2, 500.0, 3.0, 40.0)
    assert e.value.status == ERR_ARG


def test_header_declares_the_entries_and_the_library_exports_them():
    df.check_entries([
        re.compile(r"int\s+rspt_hip_design_iir\s*\(\s*int\s+type\s*,\s*int\s+order\s*,\s*double\s+sampling_rate\s*,\s*double\s+cutoff_low\s*,"
                   r"\s*double\s+cutoff_high\s*,\s*double\s*\*\s*num\s*,\s*double\s*\*\s*den\s*,\s*size_t\s*\*\s*nr_coefficients\s*\)"),
        re.compile(r"int\s+rspt_hip_peak_state_bytes\s*\(\s*rspt_hip_packer\s*\*\s*p\s*,\s*size_t\s*\*\s*bytes\s*\)"),
        re.compile(r"int\s+rspt_hip_peak_detect_batch_dev\s*\(\s*rspt_hip_packer\s*\*\s*p\s*,\s*const\s+void\s*\*\s*d_src\s*,\s*size_t\s+nblocks\s*,"
                   r"\s*int\s+variant\s*,\s*double\s+sampling_rate\s*,\s*double\s+marker_val\s*,\s*void\s*\*\s*d_state\s*,\s*uint32_t\s*\*\s*d_count\s*,"
                   r"\s*int32_t\s*\*\s*d_index\s*,\s*double\s*\*\s*d_value\s*,\s*size_t\s+max_peaks\s*,\s*double\s*\*\s*d_sig\s*,"
                   r"\s*double\s*\*\s*d_threshold\s*,\s*void\s*\*\s*stream\s*\)"),
    ], ("rspt_hip_design_iir", "rspt_hip_peak_state_bytes", "rspt_hip_peak_detect_batch_dev"))


@pytest.fixture(scope="module")
def peak_asm():
    if not os.path.exists(devasm.HIPCC):
        pytest.skip("hipcc not found")
    return {n: body for n, body in devasm.functions().items() if re.search(r"k_peak|IirState|PeakDet|peak_block", n)}


def test_peak_kernels_round_every_product_and_sum_on_their_own(peak_asm):
    """no fused multiply-add and no f64 MFMA in any k_peak kernel (or device function of it); each multiplies and adds with
    v_mul_f64 and v_add_f64"""
    df.rounds_separately(peak_asm, r"6k_peakIL", 24, fused=df.FUSED_F64)  # 4 widths x 3 variants x traces on / off
    for n, body in peak_asm.items():
        assert not [ln for ln in body if df.FUSED_F64.match(ln)], n


# ---- GPU ----

def gpu_result(pk, src, variant, fs, marker=1.0, max_peaks=None, state=None, traces=True):
    """run the stage and bring back what pc.detect returns (index / value lists cut at max_peaks)"""
    import torch

    if max_peaks is None:
        max_peaks = pk.ns  # (room for every event)
    out = pk.peak_detect_batch(src, variant=variant, sampling_rate=fs, marker_val=marker, max_peaks=max_peaks, state=state, traces=traces)
    torch.cuda.synchronize()
    return pc.to_result(out, max_peaks, traces)


VNAME = {v: k for k, v in pc.VARIANTS.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_peak_bit_exact(api, pcases, name):
    """against the record: events and trace digests with marker 1.0 and traces; marker -1.0 without traces gives the same
    events with the values s"""
    c = pcases[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    src = pc.dev(c["data"])
    st = pk.peak_state() if c["stateful"] else None
    r = gpu_result(pk, src, VNAME[c["variant"]], c["fs"], 1.0, state=st)
    got, want = summary(r), c["rec"]
    for k in ("count", "index", "values_m1", "sig", "thr"):
        assert got[k] == want[k], (name, k)
    assert all(v == 1.0 for v in pc.flat(r["value"]))
    st = pk.peak_state() if c["stateful"] else None
    m = gpu_result(pk, src, VNAME[c["variant"]], c["fs"], -1.0, state=st, traces=False)
    assert [v for row in m["count"] for v in row] == want["count"] and pc.flat(m["index"]) == want["index"]
    assert pc.vhex(pc.flat(m["value"])) == want["values_m1"]
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(pc.VARIANTS))
def test_gpu_peak_max_peaks_keeps_exact_counts(api, pcases, variant):
    """fs = 5 (nr_slope 0: an event on most samples): max_peaks 3 and 0 store fewer, count all"""
    c = pcases["walk3x400_i16_fs5_%s_fs5" % variant]
    want = pc.detect(pc.case_i32(c), c["variant"], c["fs"], 0.0)
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    src = pc.dev(c["data"])
    assert min(pc.flat([want["count"]])) > 3
    pc.events_equal(gpu_result(pk, src, variant, c["fs"], 0.0, max_peaks=3, traces=False), want, 3)
    count, index, value = pk.peak_detect_batch(src, variant=variant, sampling_rate=c["fs"], max_peaks=0)
    assert count.cpu().numpy().tolist() == want["count"] and index.numel() == 0 and value.numel() == 0
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(pc.VARIANTS))
def test_gpu_peak_stateful_calls_chain(api, variant):
    """one call of B blocks = B calls of one block on one state; a zeroed state on block 0 = fresh mode; against the restatement"""
    import torch

    bps, nch, ns, B, fs = 4, 12, 3000, 4, 1000.0
    data = np.frombuffer(pc.synth.ecg_12ch_i32(), dtype=np.uint8)[: B * bps * nch * ns]
    pk = api.new_hzr(bps, nch, ns)
    src = pc.dev(data)
    whole = gpu_result(pk, src, variant, fs, -1.0, state=pk.peak_state())
    st = pk.peak_state()
    parts = [pk.peak_detect_batch(src[b * pk.block_bytes : (b + 1) * pk.block_bytes], variant=variant, sampling_rate=fs, marker_val=-1.0,
                                  max_peaks=ns, state=st, traces=True) for b in range(B)]
    torch.cuda.synchronize()
    for b in range(B):
        count = parts[b][0].cpu().numpy()[0]
        assert count.tolist() == whole["count"][b], b
        for c in range(nch):
            assert parts[b][1][0, c, : count[c]].cpu().numpy().tolist() == whole["index"][b][c], (b, c)
            assert parts[b][2][0, c, : count[c]].cpu().numpy().tobytes() == np.asarray(whole["value"][b][c]).tobytes(), (b, c)
        assert np.array_equal(pc.canon(parts[b][3][0].cpu().numpy()), pc.canon(whole["sig"][b]))
    fresh = gpu_result(pk, src[: pk.block_bytes], variant, fs, -1.0)
    assert fresh["count"][0] == whole["count"][0] and fresh["index"][0] == whole["index"][0]
    assert np.array_equal(fresh["sig"][0], whole["sig"][0])
    want = pc.detect(pc.native_to_i32(data, bps, nch, B * ns).reshape(B, ns, nch), pc.VARIANTS[variant], fs, -1.0, stateful=True)
    pc.events_equal(whole, want)
    assert pc.tdigest(whole["sig"]) == pc.tdigest(want["sig"]) and pc.tdigest(whole["thr"]) == pc.tdigest(want["thr"])
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [0, 1])
def test_gpu_peak_odd_block_bytes_and_narrow_shapes(api, misalign):
    """3 ch x int24 x an odd sample count (odd block_bytes: blocks start off any 2- or 4-byte boundary), 1 ch, 12 ch; batches
    one byte off; against the restatement"""
    import torch

    for bps, nch, ns, fs, variant in ((3, 3, 1001, 250.0, "online"), (1, 1, 777, 360.0, "online_1st"), (2, 12, 999, 500.0, "offline_fw"),
                                      (4, 1, 2003, 1000.0, "online"), (2, 3, 1501, 250.0, "offline_fw")):
        nb = 3
        data = np.concatenate([pc.cases._rand_native(nch, ns, bps, 700 + b, 1 << (8 * bps - 3), walk=bps > 2) for b in range(nb)])
        pk = api.new_hzr(bps, nch, ns)
        raw = torch.zeros(data.size + 64, dtype=torch.uint8, device="cuda")
        src = raw[misalign : misalign + data.size]
        src.copy_(torch.from_numpy(data))
        before = raw.clone()
        r = gpu_result(pk, src, variant, fs, -1.0)
        assert torch.equal(raw, before)  # (d_src is only read)
        want = pc.detect(np.stack([pc.native_to_i32(data[b * pk.block_bytes : (b + 1) * pk.block_bytes], bps, nch, ns) for b in range(nb)]),
                         pc.VARIANTS[variant], fs, -1.0)
        pc.events_equal(r, want)
        assert pc.tdigest(r["sig"]) == pc.tdigest(want["sig"]) and pc.tdigest(r["thr"]) == pc.tdigest(want["thr"]), (bps, nch, ns)
        pk.close()


@pytest.mark.gpu
def test_gpu_peak_full_size_block(api):
    """one 64 ch x 65536 int32 block, ONLINE at 2 kHz, fresh and stateful, against the restatement"""
    bps, nch, ns, fs = 4, 64, 65536, 2000.0
    data = pc.synth.synth_native(nch, ns, 5, bps=bps, ecg=True).numpy()
    want = pc.detect(pc.native_to_i32(data, bps, nch, ns)[None], pc.ONLINE, fs, 1.0)
    assert sum(map(sum, want["count"])) > 64
    pk = api.new_xdelta_hzr(bps, nch, ns, 3)
    src = pc.dev(data)
    for st in (None, pk.peak_state()):
        r = gpu_result(pk, src, "online", fs, 1.0, max_peaks=256, state=st)
        pc.events_equal(r, want)
        assert pc.tdigest(r["sig"]) == pc.tdigest(want["sig"]) and pc.tdigest(r["thr"]) == pc.tdigest(want["thr"])
    pk.close()


@pytest.mark.gpu
def test_gpu_peak_back_to_back_without_host_sync(api, pcases):
    """calls of every variant, rate and mode on one handle and stream, no synchronisation in between"""
    import torch

    names = ["ecg12x34199_i32_%s_fs%g" % (v, fs) for v in ("online", "online_1st", "offline_fw") for fs in (500, 2000)]
    pk = api.new_hzr(4, 12, 34199)
    src = pc.dev(pcases[names[0]]["data"])
    outs = [pk.peak_detect_batch(src, variant=VNAME[pcases[n]["variant"]], sampling_rate=pcases[n]["fs"], max_peaks=64) for n in names]
    torch.cuda.synchronize()
    for n, (count, index, _) in zip(names, outs):
        rec = pcases[n]["rec"]
        cnt = count.cpu().numpy()[0]
        assert cnt.tolist() == rec["count"], n
        assert [i for c in range(12) for i in index[0, c, : cnt[c]].cpu().numpy().tolist()] == rec["index"], n
    pk.close()


@pytest.mark.gpu
def test_gpu_peak_rejects_bad_arguments(api):
    import torch

    pk = api.new_hzr(4, 3, 100)
    buf = torch.zeros(2 * pk.block_bytes, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(64, dtype=torch.int32, device="cuda")
    idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    val = torch.zeros(64, dtype=torch.float64, device="cuda")
    tr = torch.zeros(1000, dtype=torch.float64, device="cuda")
    L = api.lib()
    st = torch.cuda.current_stream().cuda_stream
    s, c, i, v, t = buf.data_ptr(), cnt.data_ptr(), idx.data_ptr(), val.data_ptr(), tr.data_ptr()

    def call(src=s, nblocks=1, variant=0, fs=500.0, count=c, index=i, value=v, max_peaks=4, sig=None, thr=None):
        return L.rspt_hip_peak_detect_batch_dev(pk._h, src, nblocks, variant, fs, 1.0, None, count, index, value, max_peaks, sig, thr, st)

    assert call() == 0
    for kw in (dict(variant=-1), dict(variant=3), dict(fs=float("nan")), dict(fs=float("inf")), dict(fs=0.0), dict(fs=-5.0),
               dict(fs=float(1 << 20) * 1.0000001), dict(count=None), dict(index=None), dict(value=None), dict(nblocks=0),
               dict(nblocks=(1 << 31) // 3 + 1), dict(src=None), dict(sig=t), dict(thr=t), dict(max_peaks=(1 << 32) + 1)):
        assert call(**kw) == ERR_ARG, kw
    assert call(fs=float(1 << 20), nblocks=1, max_peaks=0, index=None, value=None) == 0  # the largest rate; counts only
    assert call(sig=t, thr=t, nblocks=1) == 0
    with pytest.raises(api.RsptHipError) as e:
        pk.peak_detect_batch(buf, variant=7, sampling_rate=500.0)
    assert e.value.status == ERR_ARG
    n = C.c_size_t()
    assert L.rspt_hip_peak_state_bytes(pk._h, C.byref(n)) == 0 and n.value == 3 * 208 == pk.peak_state().numel()
    assert L.rspt_hip_peak_state_bytes(None, C.byref(n)) == ERR_ARG and L.rspt_hip_peak_state_bytes(pk._h, None) == ERR_ARG
    torch.cuda.synchronize()
    pk.close()


def _sweep_cases(n=60, seed=20261016):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        bps = int(rng.integers(1, 5))
        nch = int(rng.choice([1, 2, 3, 5, 12, 33, 64]))
        ns = int(rng.integers(1, 2500 if nch <= 12 else 600))
        fs = float(rng.choice([5.0, 12.0, 19.5, 100.0, 250.0, 360.0, 500.0, 999.9, 2000.0]))
        variant = str(rng.choice(sorted(pc.VARIANTS)))
        marker = float(rng.choice([1.0, -1.0, 0.0, 3.25]))
        max_peaks = int(rng.choice([0, 1, 2, 5, 50]))
        nb = int(rng.integers(1, 4))
        stateful = bool(rng.integers(0, 2))
        traces = bool(rng.integers(0, 2))
        amp = min(int(rng.choice([1 << (8 * bps - 1), 1 << max(1, 8 * bps - 5), 7])), (1 << 31) - 1)
        out.append((k, bps, nch, ns, fs, variant, marker, max_peaks, nb, stateful, traces, amp))
    return out


@pytest.mark.gpu
def test_gpu_peak_random_sweep(api):
    """60 random shapes, widths, variants, rates (below 20 Hz too), markers, max_peaks, state on / off, against the restatement"""
    for k, bps, nch, ns, fs, variant, marker, max_peaks, nb, stateful, traces, amp in _sweep_cases():
        data = np.concatenate([pc.cases._rand_native(nch, ns, bps, 8000 + 7 * k + b, amp, walk=bool(k % 2)) for b in range(nb)])
        pk = api.new_hzr(bps, nch, ns)
        r = gpu_result(pk, pc.dev(data), variant, fs, marker, max_peaks=max_peaks, state=pk.peak_state() if stateful else None, traces=traces)
        bb = pk.block_bytes
        want = pc.detect(np.stack([pc.native_to_i32(data[b * bb : (b + 1) * bb], bps, nch, ns) for b in range(nb)]), pc.VARIANTS[variant], fs,
                         marker, stateful)
        case = (k, bps, nch, ns, fs, variant, marker, max_peaks, nb, stateful, traces)
        assert r["count"] == want["count"], case
        pc.events_equal(r, want, max_peaks)
        if traces:
            assert pc.tdigest(r["sig"]) == pc.tdigest(want["sig"]) and pc.tdigest(r["thr"]) == pc.tdigest(want["thr"]), case
        pk.close()


@pytest.mark.gpu
def test_gpu_designed_coefficients_feed_the_iir_prefilter(api):
    """design_iir's (num, den), passed as iir_prefilter_batch(n=den, d=num), filter exactly as the same numbers typed in"""
    import torch

    num, den = api.design_iir("band_pass", 2, 2000.0, 0.4, 200.0)
    typed_num = [float.fromhex(v.hex()) for v in num]
    typed_den = [float.fromhex(v.hex()) for v in den]
    want_num, want_den = pc.design_iir(pc.BAND_PASS, 2, 2000.0, 0.4, 200.0)
    assert typed_num == want_num and typed_den == want_den
    data = np.frombuffer(pc.synth.ecg_12ch_i32(), dtype=np.uint8)[: 4 * 12 * 5000]
    pk = api.new_hzr(4, 12, 5000)
    a, b = pc.dev(data), pc.dev(data)
    pk.iir_prefilter_batch(a, n=den, d=num, init_nr_samples=2000, per_channel=True)
    pk.iir_prefilter_batch(b, n=typed_den, d=typed_num, init_nr_samples=2000, per_channel=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, pc.dev(data))
    pk.close()
