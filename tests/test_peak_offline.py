"""The zero-phase offline R-peak detector: peak_detector_offline::detect of the reference
(lib_rspt/peak_detector.h) on the GPU (rspt_hip_peak_detect_offline_batch_dev).

CPU: the record's inputs, the numpy restatement (tests/peak_offline_cases.py) against the reference's answers
(tests/golden/peak_offline_record.json), the C ABI, and the kernel's ISA (no fused multiply-add).
GPU (-m gpu): bit-exact against the record and the restatement, fresh and stateful, with and without traces."""
import os
import re

import numpy as np
import pytest

import devasm
import devframe as df
import peak_cases as pc
import peak_offline_cases as oc
from devframe import ERR_ARG, api  # noqa: F401


@pytest.fixture(scope="module")
def record():
    return df.golden("peak_offline_record.json")


@pytest.fixture(scope="module")
def ocases(record):
    out = {}
    for c, r in zip(oc.offline_cases(), record["cases"]):
        assert c["name"] == r["name"]
        out[c["name"]] = dict(c, rec=r)
    return out


NAMES = [c["name"] for c in oc.offline_cases()]


def summary(r, r_m1):
    """what the record holds of a restated or GPU result, from its marker 1.0 and -1.0 runs"""
    return dict(count=pc.flat([r["count"]]), index=pc.flat(r["index"]), count_m1=pc.flat([r_m1["count"]]), index_m1=pc.flat(r_m1["index"]),
                values_m1=pc.vhex(pc.flat(r_m1["value"])), sig=pc.tdigest(r["sig"]), thr=pc.tdigest(r["thr"]))


KEYS = ("count", "index", "count_m1", "index_m1", "values_m1", "sig", "thr")


# ---- CPU ----

def test_record_inputs_have_not_drifted(record):
    assert len(oc.offline_cases()) == len(record["cases"])
    for c, r in zip(oc.offline_cases(), record["cases"]):
        assert (c["name"], c["fs"], c["bps"], c["nch"], c["ns"], c["nblocks"], c["stateful"], c["calls"]) == (
            r["name"], r["fs"], r["bps"], r["nch"], r["ns"], r["nblocks"], r["stateful"], r["calls"])
        assert pc.crc(c["data"]) == r["in_crc32"], c["name"]


def test_the_record_covers_what_it_must(record):
    rs = {r["name"]: r for r in record["cases"]}
    ecg = [rs["ecg12x34199_i32_fs%d" % fs] for fs in (250, 500, 1000, 2000)]
    assert [sum(r["count"]) for r in ecg] == [405, 286, 275, 275]  # (the whole recording, every channel)
    assert {1, 2, 3, 4} <= {r["bps"] for r in rs.values()}
    assert any(not r["stateful"] and r["nblocks"] > 1 for r in rs.values())
    assert any(r["stateful"] and r["nblocks"] == 4 and r["calls"] is None for r in rs.values())
    alt = [r for r in rs.values() if r["calls"] is not None]
    assert alt and all(r["stateful"] and "fw" in r["calls"] and "detect" in r["calls"] for r in alt)
    r50 = rs["synth3x2000_i16_fs50_fs50"]  # radius 0: every peak ends on index 0
    assert sum(r50["count"]) == r50["nch"] and set(r50["index"]) == {0} and r50["collisions"] > 0
    assert sum(rs["walk2x500_i16_fs15_fs15"]["count"]) == 0  # nr_slope 1: no events
    assert any(r["values_m1"] and r["count_m1"] for r in rs.values())
    assert rs["ramps2x6000_i32_fs1000"]["revisit_moves"] > 0  # a relocated peak visited again and moved on
    assert sum(r["revisit_moves"] > 0 for r in rs.values()) >= 3
    # collisions at a radius above 0, a peak moved ahead onto a live one not yet visited among them (the constructed input)
    coll = [r for r in rs.values() if int((10.0 * r["fs"]) / 1000.0) > 0 and r["collisions"] > 0]
    assert "trispikes4x4000_i32_fs250" in [r["name"] for r in coll]
    assert any(r["collisions_ahead"] > 0 and r["revisit_moves"] > 0 for r in coll)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(ocases, name):
    c = ocases[name]
    x = oc.case_i32(c)
    st = {}
    r = oc.detect(x, c["fs"], 1.0, c["stateful"], c["calls"], st)
    m = oc.detect(x, c["fs"], -1.0, c["stateful"], c["calls"])
    got, want = summary(r, m), c["rec"]
    for k in KEYS:
        assert got[k] == want[k], (name, k)
    assert (st["revisit_moves"], st["collisions"], st["collisions_ahead"]) == (want["revisit_moves"], want["collisions"], want["collisions_ahead"])
    assert all(v == 1.0 for v in pc.flat(r["value"]))


def test_header_declares_the_entries_and_the_library_exports_them():
    df.check_entries([
        re.compile(r"int\s+rspt_hip_peak_offline_work_bytes\s*\(\s*rspt_hip_packer\s*\*\s*p\s*,\s*size_t\s+nblocks\s*,\s*int\s+stateful\s*,"
                   r"\s*size_t\s*\*\s*bytes\s*\)"),
        re.compile(r"int\s+rspt_hip_peak_detect_offline_batch_dev\s*\(\s*rspt_hip_packer\s*\*\s*p\s*,\s*const\s+void\s*\*\s*d_src\s*,"
                   r"\s*size_t\s+nblocks\s*,\s*double\s+sampling_rate\s*,\s*double\s+marker_val\s*,\s*void\s*\*\s*d_state\s*,"
                   r"\s*void\s*\*\s*d_work\s*,\s*uint32_t\s*\*\s*d_count\s*,\s*int32_t\s*\*\s*d_index\s*,\s*double\s*\*\s*d_value\s*,"
                   r"\s*size_t\s+max_peaks\s*,\s*double\s*\*\s*d_sig\s*,\s*double\s*\*\s*d_threshold\s*,\s*void\s*\*\s*stream\s*\)"),
    ], ("rspt_hip_peak_offline_work_bytes", "rspt_hip_peak_detect_offline_batch_dev"))


def test_work_bytes_refuses_a_null_handle():
    """host only: no device is needed to be told no (the sizes themselves are checked on a handle, in the GPU tests)"""
    import ctypes as C

    from rspt_amd import api

    L = api.lib()
    n = C.c_size_t()
    assert L.rspt_hip_peak_offline_work_bytes(None, 1, 0, C.byref(n)) == ERR_ARG


@pytest.fixture(scope="module")
def offline_asm():
    if not os.path.exists(devasm.HIPCC):
        pytest.skip("hipcc not found")
    return {n: body for n, body in devasm.functions().items() if re.search(r"k_peak_offline|peak_offline_block", n)}


def test_offline_kernels_round_every_product_and_sum_on_their_own(offline_asm):
    """no fused multiply-add and no f64 MFMA in any k_peak_offline kernel; each multiplies and adds with v_mul_f64 and
    v_add_f64, and nothing spills to scratch"""
    kernels = df.rounds_separately(offline_asm, r"14k_peak_offlineIL", 8, fused=df.FUSED_F64)  # 4 widths x traces on / off
    for n, body in offline_asm.items():
        assert not [ln for ln in body if df.FUSED_F64.match(ln)], n
    for n in kernels:
        assert not re.search(r"^\s+scratch_store", "".join(offline_asm[n]), re.M), n


# ---- GPU ----

def gpu_result(pk, src, fs, marker=1.0, max_peaks=None, state=None, traces=True):
    import torch

    if max_peaks is None:
        max_peaks = pk.ns
    out = pk.peak_detect_offline_batch(src, fs, marker_val=marker, max_peaks=max_peaks, state=state, traces=traces)
    torch.cuda.synchronize()
    return pc.to_result(out, max_peaks, traces)


def run_alternating(pk, src, c, marker, traces=True):
    """one state through the blocks: peak_detect_batch("offline_fw") where the case says fw, the offline entry elsewhere"""
    import torch

    st = pk.peak_state()
    parts = []
    for b, k in enumerate(c["calls"]):
        blk = src[b * pk.block_bytes : (b + 1) * pk.block_bytes]
        if k == "fw":
            parts.append(pk.peak_detect_batch(blk, variant="offline_fw", sampling_rate=c["fs"], marker_val=marker, max_peaks=pk.ns, state=st, traces=traces))
        else:
            parts.append(pk.peak_detect_offline_batch(blk, c["fs"], marker_val=marker, max_peaks=pk.ns, state=st, traces=traces))
    torch.cuda.synchronize()
    out = [torch.cat([p[i] for p in parts]) for i in range(5 if traces else 3)]
    return pc.to_result(out, pk.ns, traces)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_offline_bit_exact(api, ocases, name):
    """against the record: events and trace digests with marker 1.0 and traces; marker -1.0 without traces"""
    c = ocases[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    src = pc.dev(c["data"])
    if c["calls"] is not None:
        r = run_alternating(pk, src, c, 1.0)
        m = run_alternating(pk, src, c, -1.0, traces=False)
    else:
        r = gpu_result(pk, src, c["fs"], 1.0, state=pk.peak_state() if c["stateful"] else None)
        m = gpu_result(pk, src, c["fs"], -1.0, state=pk.peak_state() if c["stateful"] else None, traces=False)
    m["sig"], m["thr"] = r["sig"], r["thr"]
    got, want = summary(r, m), c["rec"]
    for k in KEYS:
        assert got[k] == want[k], (name, k)
    pk.close()


@pytest.mark.gpu
def test_gpu_offline_max_peaks_keeps_exact_counts(api, ocases):
    c = ocases["ecg12x34199_i32_fs250"]
    want = oc.detect(oc.case_i32(c), c["fs"], -1.0)
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    src = pc.dev(c["data"])
    assert max(pc.flat([want["count"]])) > 3
    pc.events_equal(gpu_result(pk, src, c["fs"], -1.0, max_peaks=3, traces=False), want, 3)
    count, index, value = pk.peak_detect_offline_batch(src, c["fs"], max_peaks=0)
    assert count.cpu().numpy().tolist() == want["count"] and index.numel() == 0 and value.numel() == 0
    pk.close()


@pytest.mark.gpu
def test_gpu_offline_stateful_calls_chain(api):
    """one call of B blocks = B calls of one block on one state; a zeroed state on block 0 = fresh mode; against the restatement"""
    import torch

    bps, nch, ns, B, fs = 4, 12, 3000, 4, 1000.0
    data = np.frombuffer(pc.synth.ecg_12ch_i32(), dtype=np.uint8)[: B * bps * nch * ns]
    pk = api.new_hzr(bps, nch, ns)
    src = pc.dev(data)
    whole = gpu_result(pk, src, fs, -1.0, state=pk.peak_state())
    st = pk.peak_state()
    parts = [pk.peak_detect_offline_batch(src[b * pk.block_bytes : (b + 1) * pk.block_bytes], fs, marker_val=-1.0, max_peaks=ns, state=st,
                                          traces=True) for b in range(B)]
    torch.cuda.synchronize()
    for b in range(B):
        count = parts[b][0].cpu().numpy()[0]
        assert count.tolist() == whole["count"][b], b
        for c in range(nch):
            assert parts[b][1][0, c, : count[c]].cpu().numpy().tolist() == whole["index"][b][c], (b, c)
            assert parts[b][2][0, c, : count[c]].cpu().numpy().tobytes() == np.asarray(whole["value"][b][c]).tobytes(), (b, c)
        assert np.array_equal(pc.canon(parts[b][3][0].cpu().numpy()), pc.canon(whole["sig"][b]))
    fresh = gpu_result(pk, src[: pk.block_bytes], fs, -1.0)
    assert fresh["count"][0] == whole["count"][0] and fresh["index"][0] == whole["index"][0]
    assert np.array_equal(fresh["sig"][0], whole["sig"][0])
    want = oc.detect(pc.native_to_i32(data, bps, nch, B * ns).reshape(B, ns, nch), fs, -1.0, stateful=True)
    pc.events_equal(whole, want)
    assert pc.tdigest(whole["sig"]) == pc.tdigest(want["sig"]) and pc.tdigest(whole["thr"]) == pc.tdigest(want["thr"])
    pk.close()


@pytest.mark.gpu
def test_gpu_offline_full_size_block(api):
    """one 64 ch x 65536 int32 block at 2 kHz, fresh and stateful, against the restatement"""
    bps, nch, ns, fs = 4, 64, 65536, 2000.0
    data = pc.synth.synth_native(nch, ns, 5, bps=bps, ecg=True).numpy()
    want = oc.detect(pc.native_to_i32(data, bps, nch, ns)[None], fs, 1.0)
    assert sum(map(sum, want["count"])) > 64
    pk = api.new_xdelta_hzr(bps, nch, ns, 3)
    src = pc.dev(data)
    for st in (None, pk.peak_state()):
        r = gpu_result(pk, src, fs, 1.0, max_peaks=256, state=st)
        pc.events_equal(r, want)
        assert pc.tdigest(r["sig"]) == pc.tdigest(want["sig"]) and pc.tdigest(r["thr"]) == pc.tdigest(want["thr"])
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [0, 1])
def test_gpu_offline_odd_block_bytes_and_narrow_shapes(api, misalign):
    """odd block_bytes (blocks off any 2- or 4-byte boundary), 1 ch, 12 ch, 65 ch (two waves); batches one byte off; against
    the restatement; d_src is only read"""
    import torch

    for bps, nch, ns, fs in ((3, 3, 1001, 250.0), (1, 1, 777, 360.0), (2, 12, 999, 500.0), (4, 1, 2003, 1000.0), (2, 65, 301, 250.0)):
        nb = 3
        data = np.concatenate([pc.cases._rand_native(nch, ns, bps, 700 + b, 1 << (8 * bps - 3), walk=bps > 2) for b in range(nb)])
        pk = api.new_hzr(bps, nch, ns)
        raw = torch.zeros(data.size + 64, dtype=torch.uint8, device="cuda")
        src = raw[misalign : misalign + data.size]
        src.copy_(torch.from_numpy(data))
        before = raw.clone()
        r = gpu_result(pk, src, fs, -1.0)
        assert torch.equal(raw, before)
        want = oc.detect(np.stack([pc.native_to_i32(data[b * pk.block_bytes : (b + 1) * pk.block_bytes], bps, nch, ns) for b in range(nb)]), fs, -1.0)
        pc.events_equal(r, want)
        assert pc.tdigest(r["sig"]) == pc.tdigest(want["sig"]) and pc.tdigest(r["thr"]) == pc.tdigest(want["thr"]), (bps, nch, ns)
        pk.close()


@pytest.mark.gpu
def test_gpu_offline_back_to_back_without_host_sync(api, ocases):
    """calls at every rate, fresh and stateful, on one handle and stream, no synchronisation in between"""
    import torch

    names = ["ecg12x34199_i32_fs%d" % fs for fs in (250, 500, 1000, 2000)]
    pk = api.new_hzr(4, 12, 34199)
    src = pc.dev(ocases[names[0]]["data"])
    outs = [pk.peak_detect_offline_batch(src, ocases[n]["fs"], max_peaks=256, state=pk.peak_state() if k % 2 else None) for k, n in enumerate(names)]
    torch.cuda.synchronize()
    for n, (count, index, _) in zip(names, outs):
        rec = ocases[n]["rec"]
        cnt = count.cpu().numpy()[0]
        assert cnt.tolist() == rec["count"], n
        assert [i for c in range(12) for i in index[0, c, : cnt[c]].cpu().numpy().tolist()] == rec["index"], n
    pk.close()


@pytest.mark.gpu
def test_gpu_offline_rejects_bad_arguments(api):
    import ctypes as C

    import torch

    pk = api.new_hzr(4, 3, 100)
    buf = torch.zeros(2 * pk.block_bytes, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(64, dtype=torch.int32, device="cuda")
    idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    val = torch.zeros(64, dtype=torch.float64, device="cuda")
    tr = torch.zeros(1000, dtype=torch.float64, device="cuda")
    work = torch.zeros(pk.peak_offline_work_bytes(2) // 8 + 1, dtype=torch.float64, device="cuda")
    L = api.lib()
    st = torch.cuda.current_stream().cuda_stream
    s, c, i, v, t, w = buf.data_ptr(), cnt.data_ptr(), idx.data_ptr(), val.data_ptr(), tr.data_ptr(), work.data_ptr()

    def call(src=s, nblocks=1, fs=500.0, count=c, index=i, value=v, max_peaks=4, sig=None, thr=None, work=w):
        return L.rspt_hip_peak_detect_offline_batch_dev(pk._h, src, nblocks, fs, 1.0, None, work, count, index, value, max_peaks, sig, thr, st)

    assert call() == 0
    for kw in (dict(fs=float("nan")), dict(fs=float("inf")), dict(fs=0.0), dict(fs=-5.0), dict(fs=float(1 << 20) * 1.0000001),
               dict(count=None), dict(index=None), dict(value=None), dict(nblocks=0), dict(nblocks=(1 << 31) // 3 + 1), dict(src=None),
               dict(sig=t), dict(thr=t), dict(max_peaks=(1 << 32) + 1), dict(work=None), dict(work=w + 4),
               dict(fs=9.99), dict(fs=5.0), dict(fs=10100.0)):  # (fs < 10: nr_slope 0; 10100 Hz: radius 101 > ns = 100)
        assert call(**kw) == ERR_ARG, kw
    assert call(fs=10.0) == 0 and call(fs=10099.0, max_peaks=0, index=None, value=None) == 0  # (radius 100 = ns)
    assert call(sig=t, thr=t) == 0
    n = C.c_size_t()
    assert L.rspt_hip_peak_offline_work_bytes(pk._h, 2, 0, C.byref(n)) == 0 and n.value == 100 * 64 * 28
    assert L.rspt_hip_peak_offline_work_bytes(pk._h, 0, 0, C.byref(n)) == ERR_ARG
    assert L.rspt_hip_peak_offline_work_bytes(pk._h, 1, 0, None) == ERR_ARG
    pk2 = api.new_hzr(4, 65, 10)
    assert L.rspt_hip_peak_offline_work_bytes(pk2._h, 3, 0, C.byref(n)) == 0 and n.value == 4 * 10 * 64 * 28
    assert L.rspt_hip_peak_offline_work_bytes(pk2._h, 3, 1, C.byref(n)) == 0 and n.value == 2 * 10 * 64 * 28
    # the existing entry still refuses a fourth variant
    assert L.rspt_hip_peak_detect_batch_dev(pk._h, s, 1, 3, 500.0, 1.0, None, c, i, v, 4, None, None, st) == ERR_ARG
    torch.cuda.synchronize()
    pk2.close()
    pk.close()


def _sweep_cases(n=100, seed=20261017):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        bps = int(rng.integers(1, 5))
        nch = int(rng.choice([1, 2, 3, 5, 12, 33, 64, 65]))
        fs = float(rng.choice([10.0, 15.0, 50.0, 99.9, 100.0, 250.0, 360.0, 500.0, 999.9, 2000.0]))
        rad = int((10.0 * fs) / 1000.0)
        ns = int(rng.integers(max(1, rad), 2000 if nch <= 12 else 400))
        marker = float(rng.choice([1.0, -1.0, 0.0, 3.25]))
        max_peaks = int(rng.choice([0, 1, 2, 5, 50]))
        nb = int(rng.integers(1, 4))
        stateful = bool(rng.integers(0, 2))
        traces = bool(rng.integers(0, 2))
        amp = min(int(rng.choice([1 << (8 * bps - 1), 1 << max(1, 8 * bps - 5), 7])), (1 << 31) - 1)
        out.append((k, bps, nch, ns, fs, marker, max_peaks, nb, stateful, traces, amp))
    return out


@pytest.mark.gpu
def test_gpu_offline_random_sweep(api):
    """100 random shapes, widths, rates (10 Hz up; radius 0 below 100 Hz), markers, max_peaks, state on / off, against the
    restatement"""
    for k, bps, nch, ns, fs, marker, max_peaks, nb, stateful, traces, amp in _sweep_cases():
        data = np.concatenate([pc.cases._rand_native(nch, ns, bps, 9000 + 7 * k + b, amp, walk=bool(k % 2)) for b in range(nb)])
        pk = api.new_hzr(bps, nch, ns)
        r = gpu_result(pk, pc.dev(data), fs, marker, max_peaks=max_peaks, state=pk.peak_state() if stateful else None, traces=traces)
        bb = pk.block_bytes
        want = oc.detect(np.stack([pc.native_to_i32(data[b * bb : (b + 1) * bb], bps, nch, ns) for b in range(nb)]), fs, marker, stateful)
        case = (k, bps, nch, ns, fs, marker, max_peaks, nb, stateful, traces)
        assert r["count"] == want["count"], case
        pc.events_equal(r, want, max_peaks)
        if traces:
            assert pc.tdigest(r["sig"]) == pc.tdigest(want["sig"]) and pc.tdigest(r["thr"]) == pc.tdigest(want["thr"]), case
        pk.close()


@pytest.mark.gpu
def test_gpu_offline_and_detect_fw_differ(api, ocases):
    """the offline entry is not detect_fw under another name: on the ECG recording at 1 kHz the two entries give different
    peaks, each the reference's"""
    c = ocases["ecg12x34199_i32_fs1000"]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    src = pc.dev(c["data"])
    off = gpu_result(pk, src, c["fs"], traces=False)
    fw = pk.peak_detect_batch(src, variant="offline_fw", sampling_rate=c["fs"], max_peaks=pk.ns)
    import torch

    torch.cuda.synchronize()
    fw_idx = [fw[1][0, ch, : int(fw[0][0, ch])].cpu().numpy().tolist() for ch in range(pk.nch)]
    assert pc.flat(off["index"]) == c["rec"]["index"]
    assert fw_idx != off["index"][0]
    assert fw_idx == pc.detect(oc.case_i32(c), pc.OFFLINE_FW, c["fs"])["index"][0]
    pk.close()


@pytest.mark.gpu
def test_gpu_offline_relocation_collisions_sweep(api):
    """64 channels of seeded triangle waves with spike trains at 250 and 200 Hz (radius 2): peaks relocated up the ramps are
    visited again, and peaks meet, a moved peak landing on a live one not yet visited among them; against the restatement"""
    rng = np.random.default_rng(20261018)
    nch, ns = 64, 3000
    t = np.arange(ns)
    cols = []
    for _ in range(nch):
        P, S, ph = int(rng.integers(250, 1600)), int(rng.choice([1000, 10000])), int(rng.integers(0, 1600))
        a, sp, w = int(rng.choice([100000, 1000000, -1000000])), int(rng.integers(50, 90)), int(rng.integers(1, 3))
        cols.append(np.abs(((t + ph) % P) * 2 - P) * S + np.where((t % sp) < w, a, 0))
    data = pc._i32(np.stack(cols, axis=1))
    pk = api.new_hzr(4, nch, ns)
    src = pc.dev(data)
    ahead = 0
    for fs in (250.0, 200.0):
        st = {}
        want = oc.detect(pc.native_to_i32(data, 4, nch, ns)[None], fs, -1.0, stats=st)
        assert st["collisions"] > 0 and st["revisit_moves"] > 0, (fs, st)
        ahead += st["collisions_ahead"]
        r = gpu_result(pk, src, fs, -1.0)
        pc.events_equal(r, want)
        assert pc.tdigest(r["sig"]) == pc.tdigest(want["sig"]) and pc.tdigest(r["thr"]) == pc.tdigest(want["thr"])
    assert ahead > 0
    pk.close()
