"""The FIR pre-filter stage: i_filter::new_fir / init_history_values / filter_opt of the reference
(lib_rspt/lib_filter/fir_filter.cpp) driven as its test harness drives a filter, on the GPU: rspt_hip_fir_prefilter_batch_dev.

CPU: the record's inputs, the numpy restatement (tests/fir_cases.py) against the reference's answers
(tests/golden/fir_record.json, both drivings), the C ABI, and the device ISA of the kernels (no fused or matrix f64 ops).
GPU (-m gpu): bit-exact against the record and the restatement, in place and out of place."""
import os
import re

import numpy as np
import pytest

import devasm
import devframe as df
import fir_cases as fc
from cases import digest
from devframe import ERR_ARG, api  # noqa: F401


@pytest.fixture(scope="module")
def record():
    return df.golden("fir_record.json")


@pytest.fixture(scope="module")
def fcases(record):
    """the cases with the record's coefficients (exact) in place of the ones fir_cases computes"""
    out = {}
    for c, r in zip(fc.fir_cases(), record["cases"]):
        assert c["name"] == r["name"]
        out[c["name"]] = dict(c, kernel=fc.kernel_from_record(r["kernel"]), rec=r)
    return out


NAMES = [c["name"] for c in fc.fir_cases()]


# ---- CPU ----

def test_record_inputs_have_not_drifted(record):
    for c, r in zip(fc.fir_cases(), record["cases"]):
        assert (c["name"], c["bps"], c["nch"], c["ns"]) == (r["name"], r["bps"], r["nch"], r["ns"])
        assert fc.crc(c["data"]) == r["in_crc32"], c["name"]
        assert np.array_equal(np.asarray(c["kernel"]), fc.kernel_from_record(r["kernel"])), c["name"]
    assert fc.crc(fc.big_data()) == record["big"]["in_crc32"]


def test_the_record_covers_what_it_must(record):
    ks = {len(fc.kernel_from_record(r["kernel"])) for r in record["cases"]}
    assert {1, 2, 31, 101, 255, 1001, 4097, 65536} <= ks
    assert {r["bps"] for r in record["cases"]} == {1, 2, 3, 4}
    assert any(r["nch"] == 1 for r in record["cases"])
    assert any(len(fc.kernel_from_record(r["kernel"])) > r["ns"] for r in record["cases"])


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(fcases, name):
    c = fcases[name]
    y = fc.fir_prefilter(c["data"], c["bps"], c["nch"], c["ns"], c["kernel"])
    for mode in ("shared", "per_channel"):
        assert digest(y) == c["rec"][mode]["digest"] and fc.crc(y) == c["rec"][mode]["crc32"], mode


def test_restatement_matches_reference_at_full_size(record):
    b = record["big"]
    y = fc.fir_prefilter(fc.big_data(), b["bps"], b["nch"], b["ns"], fc.kernel_from_record(b["kernel"]))
    assert fc.crc(y) == b["shared"]["crc32"] == b["per_channel"]["crc32"]


def test_one_shared_filter_equals_one_filter_per_channel(record):
    """init_history_values replaces the whole window, so, unlike the IIR stage, the FIR stage has one semantics"""
    for r in record["cases"] + [record["big"]]:
        assert r["shared"] == r["per_channel"], r["name"]


def test_the_record_holds_overflow_and_nan():
    c = {x["name"]: x for x in fc.fir_cases()}
    for name in ("full_scale6x3000_i32_gain_overflow", "rand4x2000_i32_inf_nan"):
        x = c[name]
        y = fc.fir_i32(fc.native_to_i32(x["data"], x["bps"], x["nch"], x["ns"]), x["kernel"])
        assert (~np.isfinite(y) | (np.abs(y) >= 2.0 ** 31)).sum() > 100, name
    x = c["rand4x2000_i32_inf_nan"]
    assert np.isnan(fc.fir_i32(fc.native_to_i32(x["data"], x["bps"], x["nch"], x["ns"]), x["kernel"])).sum() > 100


def test_header_declares_the_entry_and_the_library_exports_it():
    df.check_entries([re.compile(r"int\s+rspt_hip_fir_prefilter_batch_dev\s*\(\s*rspt_hip_packer\s*\*\s*p\s*,\s*const\s+void\s*\*\s*d_src\s*,\s*void\s*\*\s*d_dst\s*,"
                                 r"\s*size_t\s+nblocks\s*,\s*const\s+double\s*\*\s*kernel\s*,\s*size_t\s+kernel_size\s*,\s*void\s*\*\s*stream\s*\)")], ["rspt_hip_fir_prefilter_batch_dev"])


@pytest.fixture(scope="module")
def fir_asm():
    if not os.path.exists(devasm.HIPCC):
        pytest.skip("hipcc not found")
    return {n: body for n, body in devasm.functions().items() if re.search(r"k_fir", n)}


def test_fir_kernels_round_every_product_and_sum_on_their_own(fir_asm):
    """no fused multiply-add and no f64 MFMA in any k_fir* kernel; every filter kernel (k_fir<bps, aligned>: k_fir_halo only
    copies bytes) multiplies and adds with v_mul_f64 and v_add_f64"""
    df.rounds_separately(fir_asm, r"5k_firIL", 6, fused=df.FUSED_F64)  # int8, int16 (+aligned), int24, int32 (+aligned)
    assert any("k_fir_halo" in n for n in fir_asm)
    for n, body in fir_asm.items():
        assert not [ln for ln in body if df.FUSED_F64.match(ln)], n


# ---- GPU ----

def _batch(data, n):
    import torch

    return torch.from_numpy(np.stack([np.asarray(data, dtype=np.uint8)] * n)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_fir_bit_exact(api, fcases, name):
    import torch

    c = fcases[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    src = _batch(c["data"], 3)
    out = torch.empty_like(src)
    pk.fir_prefilter_batch(src, c["kernel"], d_dst=out)  # out of place
    pk.fir_prefilter_batch(src, c["kernel"])  # in place
    torch.cuda.synchronize()
    for buf, how in ((out, "out of place"), (src, "in place")):
        for b in range(3):
            assert digest(buf[b].cpu().numpy()) == c["rec"]["shared"]["digest"], (how, b)
    pk.close()


@pytest.mark.gpu
def test_gpu_fir_full_size_block_in_place(api, record):
    import torch

    r = record["big"]
    pk = api.new_xdelta_hzr(r["bps"], r["nch"], r["ns"], 3)
    buf = _batch(fc.big_data(), 2)
    pk.fir_prefilter_batch(buf, fc.kernel_from_record(r["kernel"]))
    torch.cuda.synchronize()
    for b in range(2):
        assert fc.crc(buf[b].cpu().numpy()) == r["shared"]["crc32"], b
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [0, 1])
def test_gpu_fir_odd_block_bytes(api, misalign):
    """3 ch x int24 x an odd sample count: block_bytes is odd, so every other block starts off any 2- or 4-byte boundary;
    and an int32 batch whose base is one byte off (the byte-wise path)"""
    import torch

    for bps, nch, ns, K in ((3, 3, 1001, 37), (1, 1, 777, 5), (4, 5, 999, 64)):
        data = np.concatenate([fc.cases._rand_native(nch, ns, bps, 900 + b, 1 << (8 * bps - 2)) for b in range(3)])
        k = fc._rand_kernel(K, 901, 5)
        pk = api.new_hzr(bps, nch, ns)
        n = data.size
        raw = torch.zeros(2 * n + 64, dtype=torch.uint8, device="cuda")
        src = raw[misalign : misalign + n]
        src.copy_(torch.from_numpy(data))
        dst = raw[n + 32 + misalign : n + 32 + misalign + n]
        pk.fir_prefilter_batch(src, k, d_dst=dst)
        pk.fir_prefilter_batch(src, k)
        torch.cuda.synchronize()
        bb = bps * nch * ns
        for b in range(3):
            want = fc.fir_prefilter(data[b * bb : (b + 1) * bb], bps, nch, ns, k).tobytes()
            assert dst[b * bb : (b + 1) * bb].cpu().numpy().tobytes() == want, (bps, nch, ns, b, "out of place")
            assert src[b * bb : (b + 1) * bb].cpu().numpy().tobytes() == want, (bps, nch, ns, b, "in place")
        pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ecg12x34199_i32_bandpass101", "ds3x20000_i24_bandpass255"])
def test_gpu_fir_then_compress_matches_oracle(api, orc, fcases, name):
    """what the harness does next: xdelta_hzr on the filtered block -- the device stream equals the oracle's stream of the
    reference's filtered block"""
    import torch

    c = fcases[name]
    want_block = fc.fir_prefilter(c["data"], c["bps"], c["nch"], c["ns"], c["kernel"])
    assert digest(want_block) == c["rec"]["shared"]["digest"]
    want = orc.packer("xdelta_hzr", c["bps"], c["nch"], c["ns"], 3).compress(want_block)
    pk = api.new_xdelta_hzr(c["bps"], c["nch"], c["ns"], 3)
    buf = _batch(c["data"], 2)
    pk.fir_prefilter_batch(buf, c["kernel"])
    d_dst, d_sizes = pk.compress_batch(buf)
    torch.cuda.synchronize()
    for b in range(2):
        assert d_dst[b, : int(d_sizes[b])].cpu().numpy().tobytes() == want, b
    pk.close()


@pytest.mark.gpu
def test_gpu_fir_back_to_back_kernels_without_host_sync(api, record):
    """two calls on one stream, the first on a large batch, the second with other coefficients, the caller's arrays
    overwritten as soon as each call returns: each call filters with its own coefficients"""
    import torch

    r = record["big"]
    pk = api.new_hzr(r["bps"], r["nch"], r["ns"])
    big = _batch(fc.big_data(), 12)
    small = big[:2].clone()
    k1 = np.ascontiguousarray(fc.kernel_from_record(r["kernel"]))
    k2 = np.ascontiguousarray(fc._rand_kernel(37, 902, 6))
    k2_copy = k2.copy()
    pk.fir_prefilter_batch(big, k1)
    k1[:] = np.nan
    pk.fir_prefilter_batch(small, k2)
    k2[:] = np.nan
    torch.cuda.synchronize()
    for b in (0, 11):
        assert fc.crc(big[b].cpu().numpy()) == r["shared"]["crc32"], b
    want = fc.fir_prefilter(fc.big_data(), r["bps"], r["nch"], r["ns"], k2_copy).tobytes()
    for b in range(2):
        assert small[b].cpu().numpy().tobytes() == want, b
    pk.close()


@pytest.mark.gpu
def test_gpu_fir_halo_grows_between_back_to_back_calls_without_host_sync(api):
    """two in-place calls on one handle and one stream, no host synchronisation between them, the second with the larger halo:
    the handle replaces its halo buffer while the first call may still be in flight, and both results are exact.

    3 ch x int16 x 20000, 2 blocks.  With 3 channels a workgroup's kFirThreads = 256 lanes hold 85 rows of channels, so a chunk
    is 85 x kFirR = 85 x 16 = 1360 rows; 20000 rows allow at most 20000 // 1360 = 14 spans, each rounded up to whole chunks:
    2 x 1360 = 2720 rows, ceil(20000 / 2720) = 8 spans per block for the 9-tap and the 257-tap kernel alike (4 (K - 1) <= 1360).
    An in-place call stages the K - 1 rows in front of every span but the first: 2 x 7 pieces of 8 rows, then 2 x 7 of 256."""
    import torch

    bps, nch, ns = 2, 3, 20000
    pk = api.new_hzr(bps, nch, ns)
    data = np.concatenate([fc.cases._rand_native(nch, ns, bps, 910 + b, 1 << (8 * bps - 2)) for b in range(2)])
    k_small, k_large = fc._rand_kernel(9, 911, 4), fc._rand_kernel(257, 912, 8)
    a = torch.from_numpy(data).cuda()
    b = a.clone()
    torch.cuda.synchronize()
    pk.fir_prefilter_batch(a, k_small)
    pk.fir_prefilter_batch(b, k_large)
    torch.cuda.synchronize()
    bb = bps * nch * ns
    for buf, k in ((a, k_small), (b, k_large)):
        got = buf.cpu().numpy()
        for i in range(2):
            want = fc.fir_prefilter(data[i * bb : (i + 1) * bb], bps, nch, ns, k).tobytes()
            assert got[i * bb : (i + 1) * bb].tobytes() == want, (len(k), i)
    pk.close()


@pytest.mark.gpu
def test_gpu_fir_rejects_bad_arguments(api):
    import torch

    pk = api.new_hzr(4, 3, 100)
    buf = torch.zeros(4 * pk.block_bytes, dtype=torch.uint8, device="cuda")
    src = buf[: 2 * pk.block_bytes]
    for k, dst in ((np.zeros(0), None), (np.zeros(65537), None), (np.ones(3), buf[16 : 16 + 2 * pk.block_bytes]),
                   (np.ones(3), buf[pk.block_bytes : 3 * pk.block_bytes])):
        with pytest.raises(api.RsptHipError) as e:
            pk.fir_prefilter_batch(src, k, d_dst=dst)
        assert e.value.status == ERR_ARG
    pk.fir_prefilter_batch(src, np.ones(65536) / 65536, d_dst=buf[2 * pk.block_bytes :])  # the largest kernel, apart: accepted
    torch.cuda.synchronize()
    pk.close()


def _sweep_cases(n=200, seed=20261015):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        bps = int(rng.integers(1, 5))
        nch = int(rng.choice([1, 2, 3, 5, 12, 33, 64, 100, 257]))
        ns = int(rng.integers(1, 3000 if nch <= 12 else 600))
        K = int(rng.choice([1, 2, 3, 7, 16, 17, 31, 64, 101, 255, 300, 1000, 2500]))
        amp = int(rng.choice([1 << (8 * bps - 1), 1 << max(1, 8 * bps - 4), 100]))
        amp = min(amp, (1 << 31) - 1)
        scale = float(rng.choice([1e-3, 1.0 / K, 1.0, 3.0]))
        k = rng.standard_normal(K) * scale
        nb = int(rng.integers(1, 4))
        in_place = bool(rng.integers(0, 2))
        out.append((i, bps, nch, ns, k, amp, nb, in_place))
    return out


@pytest.mark.gpu
def test_gpu_fir_random_sweep(api):
    """about 200 random shapes, kernels and amplitudes, each launched once, against the restatement"""
    import torch

    for i, bps, nch, ns, k, amp, nb, in_place in _sweep_cases():
        data = np.concatenate([fc.cases._rand_native(nch, ns, bps, 5000 + 7 * i + b, amp) for b in range(nb)])
        pk = api.new_hzr(bps, nch, ns)
        src = torch.from_numpy(data).cuda()
        out = pk.fir_prefilter_batch(src, k, d_dst=None if in_place else torch.empty_like(src))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bb = bps * nch * ns
        for b in range(nb):
            want = fc.fir_prefilter(data[b * bb : (b + 1) * bb], bps, nch, ns, k)
            assert np.array_equal(got[b * bb : (b + 1) * bb], want), (i, bps, nch, ns, len(k), amp, nb, in_place, b)
        pk.close()
