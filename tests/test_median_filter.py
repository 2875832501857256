"""The rolling-median stage: rolling_window_median<double>(W) of the reference (lib_rspt/lib_stat/
rolling_window_median.h), one object per channel, on the GPU: rspt_hip_median_filter_batch_dev.

CPU: the record's inputs, the reference's own test expectations, the numpy restatement (tests/median_cases.py) against the
reference's answers (tests/golden/median_record.json), the integer even-window rule, and the C ABI.
GPU (-m gpu): bit-exact against the record and the restatement, in place and out of place, in both regimes."""
import re

import numpy as np
import pytest

import devframe as df
import median_cases as mc
from cases import digest
from devframe import ERR_ARG, api  # noqa: F401

SHORT_MAX = 32  # kMedShortMax in rspt_amd/csrc/median.hip: the regime switch


@pytest.fixture(scope="module")
def record():
    return df.golden("median_record.json")


@pytest.fixture(scope="module")
def mcases(record):
    out = {}
    for c, r in zip(mc.median_cases(), record["cases"]):
        assert c["name"] == r["name"]
        out[c["name"]] = dict(c, rec=r)
    return out


NAMES = [c["name"] for c in mc.median_cases()]


# ---- CPU ----

def test_record_inputs_have_not_drifted(record):
    assert len(mc.median_cases()) == len(record["cases"])
    for c, r in zip(mc.median_cases(), record["cases"]):
        assert (c["name"], c["bps"], c["nch"], c["ns"], c["W"]) == (r["name"], r["bps"], r["nch"], r["ns"], r["W"])
        assert mc.crc(c["data"]) == r["in_crc32"], c["name"]
    assert mc.crc(mc.big_data()) == record["big"]["in_crc32"]
    assert sorted(int(w) for w in record["big"]["crc32"]) == mc.BIG["windows"]


def test_the_record_covers_what_it_must(record):
    rs = record["cases"]
    ws = {r["W"] for r in rs}
    assert {1, 2, 5, 6, 7, 1500, 101, 1001} <= ws and any(w % 2 == 0 for w in ws) and any(w % 2 for w in ws)
    assert {SHORT_MAX, SHORT_MAX + 1} <= ws
    assert {r["bps"] for r in rs} == {1, 2, 3, 4}
    assert any(r["ns"] == 1 for r in rs) and any(r["nch"] == 1 for r in rs)
    for d in (-1, 0, 7):
        assert any(r["W"] == r["ns"] + d for r in rs), d


def test_reference_returns_what_its_own_test_expects(record):
    """rspt_test.cpp test_8_rolling_window_median: the shim's doubles on the 20 inputs equal the expected lists"""
    for W, want in mc.REF20_EXPECTED.items():
        assert record["ref20"][str(W)] == [float(v) for v in want], W
        x = np.asarray(mc.REF20, dtype=np.int32)[:, None]
        assert np.array_equal(mc.median_i32(x, W)[:, 0], np.trunc(np.asarray(want)).astype(np.int32)), W


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_reference(mcases, name):
    c = mcases[name]
    y = mc.median_filter(c["data"], c["bps"], c["nch"], c["ns"], c["W"])
    assert digest(y) == c["rec"]["digest"] and mc.crc(y) == c["rec"]["crc32"]


@pytest.mark.parametrize("W", mc.BIG["windows"])
def test_restatement_matches_reference_at_full_size(record, W):
    b = record["big"]
    y = mc.median_filter(mc.big_data(), b["bps"], b["nch"], b["ns"], W)
    assert mc.crc(y) == b["crc32"][str(W)]


def test_integer_even_rule_equals_the_double_rule():
    """(int32_t)(((double)a + b) / 2.0) is the integer sum halved toward zero, on extreme and odd-sum pairs"""
    v = [-(1 << 31), -(1 << 31) + 1, -3, -4, -1, 0, 1, 2, 3, (1 << 31) - 2, (1 << 31) - 1, 12345, -12345]
    a, b = np.array([(p, q) for p in v for q in v], dtype=np.int64).T
    want = np.trunc((a.astype(np.float64) + b.astype(np.float64)) / 2.0).astype(np.int64)
    assert np.array_equal(mc.half_sum(a, b).astype(np.int64), want)
    assert int(mc.half_sum(-3, -4)) == -3 and int(mc.half_sum(3, 4)) == 3


def test_a_window_of_ns_or_more_is_the_expanding_median():
    x = mc.native_to_i32(mc.cases._rand_native(3, 300, 4, 87, 1000), 4, 3, 300)
    e = mc.median_i32(x, 300)
    assert np.array_equal(mc.median_i32(x, 301), e) and np.array_equal(mc.median_i32(x, 10 ** 6), e)
    assert np.array_equal(mc.median_i32(x, 1), x)


def test_header_declares_the_entry_and_the_library_exports_it():
    df.check_entries([re.compile(r"int\s+rspt_hip_median_filter_batch_dev\s*\(\s*rspt_hip_packer\s*\*\s*p\s*,\s*const\s+void\s*\*\s*d_src\s*,\s*void\s*\*\s*d_dst\s*,"
                                 r"\s*size_t\s+nblocks\s*,\s*size_t\s+window\s*,\s*void\s*\*\s*stream\s*\)")], ["rspt_hip_median_filter_batch_dev"])


# ---- GPU ----

def _batch(data, n):
    import torch

    return torch.from_numpy(np.stack([np.asarray(data, dtype=np.uint8)] * n)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_gpu_median_bit_exact(api, mcases, name):
    import torch

    c = mcases[name]
    pk = api.new_hzr(c["bps"], c["nch"], c["ns"])
    src = _batch(c["data"], 3)
    out = torch.empty_like(src)
    pk.median_filter_batch(src, c["W"], d_dst=out)  # out of place
    pk.median_filter_batch(src, c["W"])  # in place
    torch.cuda.synchronize()
    for buf, how in ((out, "out of place"), (src, "in place")):
        for b in range(3):
            assert digest(buf[b].cpu().numpy()) == c["rec"]["digest"], (how, b)
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", mc.BIG["windows"])
def test_gpu_median_full_size_block(api, record, W):
    import torch

    r = record["big"]
    pk = api.new_xdelta_hzr(r["bps"], r["nch"], r["ns"], 3)
    src = _batch(mc.big_data(), 2)
    out = torch.empty_like(src)
    pk.median_filter_batch(src, W, d_dst=out)
    pk.median_filter_batch(src, W)
    torch.cuda.synchronize()
    for b in range(2):
        assert mc.crc(out[b].cpu().numpy()) == r["crc32"][str(W)], ("out of place", b)
        assert mc.crc(src[b].cpu().numpy()) == r["crc32"][str(W)], ("in place", b)
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [0, 1])
def test_gpu_median_odd_block_bytes(api, misalign):
    """3 ch x int24 x an odd sample count: block_bytes is odd, so every other block starts off any 2- or 4-byte boundary;
    and batches whose base is one byte off (the byte-wise path); short and generic windows"""
    import torch

    for bps, nch, ns, W in ((3, 3, 1001, 9), (3, 3, 1001, 77), (1, 1, 777, 5), (2, 5, 999, 64), (4, 5, 999, 31)):
        data = np.concatenate([mc.cases._rand_native(nch, ns, bps, 900 + b, 1 << (8 * bps - 2)) for b in range(3)])
        pk = api.new_hzr(bps, nch, ns)
        n = data.size
        raw = torch.zeros(2 * n + 64, dtype=torch.uint8, device="cuda")
        src = raw[misalign : misalign + n]
        src.copy_(torch.from_numpy(data))
        dst = raw[n + 32 + misalign : n + 32 + misalign + n]
        pk.median_filter_batch(src, W, d_dst=dst)
        pk.median_filter_batch(src, W)
        torch.cuda.synchronize()
        bb = bps * nch * ns
        for b in range(3):
            want = mc.median_filter(data[b * bb : (b + 1) * bb], bps, nch, ns, W).tobytes()
            assert dst[b * bb : (b + 1) * bb].cpu().numpy().tobytes() == want, (bps, nch, ns, W, b, "out of place")
            assert src[b * bb : (b + 1) * bb].cpu().numpy().tobytes() == want, (bps, nch, ns, W, b, "in place")
        pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("W", [4, 5, 8, 9, 16, 17, SHORT_MAX, SHORT_MAX + 1])
def test_gpu_median_at_the_regime_switch(api, W):
    """every register width of the short path at its limit and one above, and kMedShortMax against the generic path above it,
    on a wide block split into spans (in place: the halo) and heavy ties"""
    import torch

    bps, nch, ns = 4, 64, 5000
    data = np.concatenate([mc.cases._rand_native(nch, ns, bps, 910 + b, amp) for b, amp in enumerate((1 << 30, 5))])
    pk = api.new_hzr(bps, nch, ns)
    src = torch.from_numpy(data).cuda()
    out = pk.median_filter_batch(src, W, d_dst=torch.empty_like(src))
    pk.median_filter_batch(src, W)
    torch.cuda.synchronize()
    bb = bps * nch * ns
    for b in range(2):
        want = mc.median_filter(data[b * bb : (b + 1) * bb], bps, nch, ns, W)
        assert np.array_equal(out[b * bb : (b + 1) * bb].cpu().numpy(), want), (W, b, "out of place")
        assert np.array_equal(src[b * bb : (b + 1) * bb].cpu().numpy(), want), (W, b, "in place")
    pk.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ecg12x34199_i32_w101", "ds3x20000_i24_w31"])
def test_gpu_median_then_compress_matches_oracle(api, orc, mcases, name):
    """xdelta_hzr on the filtered block: the device stream equals the oracle's stream of the restated block"""
    import torch

    c = mcases[name]
    want_block = mc.median_filter(c["data"], c["bps"], c["nch"], c["ns"], c["W"])
    assert digest(want_block) == c["rec"]["digest"]
    want = orc.packer("xdelta_hzr", c["bps"], c["nch"], c["ns"], 3).compress(want_block)
    pk = api.new_xdelta_hzr(c["bps"], c["nch"], c["ns"], 3)
    buf = _batch(c["data"], 2)
    pk.median_filter_batch(buf, c["W"])
    d_dst, d_sizes = pk.compress_batch(buf)
    torch.cuda.synchronize()
    for b in range(2):
        assert d_dst[b, : int(d_sizes[b])].cpu().numpy().tobytes() == want, b
    pk.close()


@pytest.mark.gpu
def test_gpu_median_back_to_back_windows_without_host_sync(api, record):
    """calls on one stream with different windows and regimes, no synchronisation in between: each gets its own window, and the
    generic path's buffers grow between calls without disturbing the call before"""
    import torch

    r = record["big"]
    pk = api.new_hzr(r["bps"], r["nch"], r["ns"])
    big = _batch(mc.big_data(), 4)
    a, b_, c_ = big[:2].clone(), big[2:].clone(), big[:1].clone()
    small_data = mc.cases._rand_native(r["nch"], r["ns"], 4, 920, 1 << 20)
    small = torch.from_numpy(small_data).cuda()
    small_out = torch.empty_like(small)
    pk.median_filter_batch(small, 7, d_dst=small_out)  # short path first
    pk.median_filter_batch(a, 101)  # generic, in place
    pk.median_filter_batch(b_, 65536)
    pk.median_filter_batch(c_, 3)
    torch.cuda.synchronize()
    assert np.array_equal(small_out.cpu().numpy(), mc.median_filter(small_data, 4, r["nch"], r["ns"], 7))
    for blk in range(2):
        assert mc.crc(a[blk].cpu().numpy()) == r["crc32"]["101"], blk
        assert mc.crc(b_[blk].cpu().numpy()) == r["crc32"]["65536"], blk
    assert np.array_equal(c_[0].cpu().numpy(), mc.median_filter(mc.big_data(), 4, r["nch"], r["ns"], 3))
    pk.close()


@pytest.mark.gpu
def test_gpu_median_rejects_bad_arguments(api):
    import torch

    pk = api.new_hzr(4, 3, 100)
    bb = pk.block_bytes
    buf = torch.zeros(4 * bb, dtype=torch.uint8, device="cuda")
    src = buf[: 2 * bb]
    L = api.lib()
    st = torch.cuda.current_stream().cuda_stream
    for W, dst in ((0, None), (5, buf[16 : 16 + 2 * bb]), (5, buf[bb : 3 * bb]), (40, buf[8 : 8 + 2 * bb])):
        with pytest.raises(api.RsptHipError) as e:
            pk.median_filter_batch(src, W, d_dst=dst)
        assert e.value.status == ERR_ARG, (W,)
    assert L.rspt_hip_median_filter_batch_dev(pk._h, None, buf.data_ptr(), 1, 3, st) == ERR_ARG
    assert L.rspt_hip_median_filter_batch_dev(pk._h, buf.data_ptr(), None, 1, 3, st) == ERR_ARG
    assert L.rspt_hip_median_filter_batch_dev(pk._h, buf.data_ptr(), buf.data_ptr(), (1 << 31) // 3 + 1, 3, st) == ERR_ARG  # nblocks * nch >= 2^31
    pk.median_filter_batch(src, 1 << 40, d_dst=buf[2 * bb :])  # any window >= 1: apart, accepted
    torch.cuda.synchronize()
    assert np.array_equal(buf[2 * bb :].cpu().numpy(), np.zeros(2 * bb, dtype=np.uint8))
    pk.close()


@pytest.mark.gpu
def test_gpu_closing_a_handle_with_a_median_call_in_flight(api):
    """close right after a generic-path call on a full-size batch: destroy waits for the call and releases the stage's buffers --
    device memory after five such rounds is where it was"""
    import torch

    bps, nch, ns = 4, 64, 65536
    src = torch.from_numpy(np.stack([mc.cases._rand_native(nch, ns, bps, 930 + i, 1 << 20) for i in range(2)])).cuda()
    want = [mc.crc(mc.median_filter(src[i].cpu().numpy(), bps, nch, ns, 257)) for i in range(2)]

    def one_round():
        pk = api.new_hzr(bps, nch, ns)
        dst = torch.empty_like(src)
        pk.median_filter_batch(src, 257, d_dst=dst)
        pk.median_filter_batch(src.clone(), 9)  # a short-path call, in place, with its halo
        pk.close()  # no synchronisation before
        torch.cuda.synchronize()
        for i in range(2):
            assert mc.crc(dst[i].cpu().numpy()) == want[i], i
        del dst

    one_round()  # (the first launches load the code objects)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.mem_get_info()[0]
    for _ in range(5):
        one_round()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    drift = before - torch.cuda.mem_get_info()[0]
    print("device memory drift over 5 rounds: %d bytes" % drift)
    assert drift <= (16 << 20), drift  # (a leaked set of generic-path buffers is 640 MiB a round)


def _sweep_cases(n=200, seed=20261015):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        bps = int(rng.integers(1, 5))
        nch = int(rng.choice([1, 2, 3, 5, 12, 33, 64, 100, 257, 300]))
        ns = int(rng.integers(1, 3000 if nch <= 12 else 500))
        W = int(rng.choice([1, 2, 3, int(rng.integers(1, 40)), int(rng.integers(1, ns + 6)), ns, ns + 5]))
        W = max(1, W)
        amp = int(rng.choice([1 << (8 * bps - 1), 1 << max(1, 8 * bps - 4), 3]))
        amp = min(amp, (1 << 31) - 1)
        nb = int(rng.integers(1, 4))
        in_place = bool(rng.integers(0, 2))
        out.append((i, bps, nch, ns, W, amp, nb, in_place))
    return out


@pytest.mark.gpu
def test_gpu_median_random_sweep(api):
    """200 random shapes, windows (1 to ns + 5) and value ranges (full and narrow), each launched once, against the restatement"""
    import torch

    for i, bps, nch, ns, W, amp, nb, in_place in _sweep_cases():
        data = np.concatenate([mc.cases._rand_native(nch, ns, bps, 6000 + 7 * i + b, amp) for b in range(nb)])
        pk = api.new_hzr(bps, nch, ns)
        src = torch.from_numpy(data).cuda()
        out = pk.median_filter_batch(src, W, d_dst=None if in_place else torch.empty_like(src))
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bb = bps * nch * ns
        for b in range(nb):
            want = mc.median_filter(data[b * bb : (b + 1) * bb], bps, nch, ns, W)
            assert np.array_equal(got[b * bb : (b + 1) * bb], want), (i, bps, nch, ns, W, amp, nb, in_place, b)
        pk.close()
