"""A quality ladder and a per-block choice through compress and decompress (rspt_hip_compress_batch_ladder_dev,
rspt_hip_decompress_batch_ladder_dev): block b's stream, size and decoded samples are byte for byte what
rspt_hip_set_quantizer(ladder[choice[b]], nb) followed by the plain batch entry gives for that block -- the composed oracle, run on
the same device: one plain call per distinct quality, each block taken from the run of its own -- at every hadamard size class,
on the dense dct, at nb 1..4 and the sample widths; a mixed batch against the reference's own streams where
tests/golden/lossy_quantizer_record.json holds two settings of one shape and nb; choices outside the ladder; the refusals."""
import ctypes as C

import numpy as np
import pytest

import cases
import devframe as df
import lossy_quantizer_cases as lq
from devframe import ERR_ARG, ERR_UNSUPPORTED, api  # noqa: F401

pytestmark = pytest.mark.gpu

BIT63 = 1 << 63
HAD_LADDER = [0.1, 1.0, 3.0, 7.3]
DCT_LADDER = [1000.0, 128.0, 8.0, 0.37]
# (kind, bps, nch, ns, nb, amplitude): every hadamard size class at its smallest, the dense dct; nb 1..4 and int8 / 16 / 24 spread
SHAPES = [("hadamard", 4, 1, 2, 1, 3000), ("hadamard", 1, 3, 8, 2, 100), ("hadamard", 2, 5, 1024, 3, 3000), ("hadamard", 4, 2, 32768, 4, 3000),
          ("hadamard", 4, 2, 65536, 3, 3000), ("hadamard", 4, 2, 131072, 2, 3000),
          ("dct", 3, 3, 100, 2, 1 << 20), ("dct", 4, 2, 257, 3, 3000), ("dct", 2, 2, 4096, 1, 3000)]
IDS = ["%s_i%d_%dx%d_nb%d" % (k, 8 * bps, nch, ns, nb) for k, bps, nch, ns, nb, amp in SHAPES]
NBLOCKS = 5
CHOICE = [2, 0, 3, 1, 2]  # every entry, one of them twice


def _ladder(kind):
    return HAD_LADDER if kind == "hadamard" else DCT_LADDER


def _new(api, kind, bps, nch, ns, nb, flags=0):
    pk = api.SignalPacker(lq.KIND_ID[kind] | flags, bps, nch, ns, lq.DEFAULTS[kind][1])
    pk.set_quantizer(nb=nb)
    return pk


def _data(bps, nch, ns, amp, n=NBLOCKS):
    import torch

    return torch.from_numpy(np.stack([cases._rand_native(nch, ns, bps, 8800 + 13 * i + ns % 97, amp, walk=(i & 1) == 1) for i in range(n)])).cuda()


def _plain(pk, d_src, q):
    """(streams, sizes, decoded, consumed) of the plain entries at quality q, and the handle back at its own quality"""
    import torch

    q0, nb = pk.quantizer()
    pk.set_quantizer(q)
    d_dst, d_sizes = pk.compress_batch(d_src)
    d_out, d_used = pk.decompress_batch(d_dst, d_src.shape[0], d_dst.shape[1])
    torch.cuda.synchronize()
    pk.set_quantizer(q0)
    return d_dst.cpu().numpy(), d_sizes.cpu().numpy(), d_out.cpu().numpy(), d_used.cpu().numpy()


@pytest.fixture(scope="module")
def runs(api):
    """per shape, once: the handle's inputs and the composed oracle of every ladder entry"""
    memo = {}

    def get(i):
        if i not in memo:
            kind, bps, nch, ns, nb, amp = SHAPES[i]
            pk = _new(api, kind, bps, nch, ns, nb)
            d_src = _data(bps, nch, ns, amp)
            memo[i] = (pk, d_src, [_plain(pk, d_src, q) for q in _ladder(kind)])
        return memo[i]

    yield get
    for pk, _, _ in memo.values():
        pk.close()


def _ladder_roundtrip(pk, d_src, ladder, choice, d_dst=None):
    import torch

    d_choice = torch.tensor(choice, dtype=torch.int32, device="cuda")
    d_dst, d_sizes = pk.compress_batch(d_src, d_dst=d_dst, ladder=ladder, choice=d_choice)
    nblocks = d_src.shape[0]
    d_out = torch.full((nblocks, pk.block_bytes), 0x5A, dtype=torch.uint8, device="cuda")
    d_out, d_used = pk.decompress_batch(d_dst, nblocks, d_dst.shape[1], d_out=d_out, ladder=ladder, choice=d_choice)
    torch.cuda.synchronize()
    return d_dst.cpu().numpy(), d_sizes.cpu().numpy().view(np.uint64), d_out.cpu().numpy(), d_used.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_every_block_is_the_plain_entry_at_its_own_quality(runs, i):
    pk, d_src, oracle = runs(i)
    ladder = _ladder(SHAPES[i][0])
    own = pk.quantizer()
    dst, sizes, out, used = _ladder_roundtrip(pk, d_src, ladder, CHOICE)
    assert pk.quantizer() == own  # the handle's own quality is neither read nor changed
    for b, k in enumerate(CHOICE):
        o_dst, o_sizes, o_out, o_used = oracle[k]
        n = int(o_sizes[b])
        assert int(sizes[b]) == n and int(used[b]) == int(o_used[b]) == n, (IDS[i], b, k)
        assert np.array_equal(dst[b, :n], o_dst[b, :n]), (IDS[i], b, k, "stream")
        assert np.array_equal(out[b], o_out[b]), (IDS[i], b, k, "decoded")
        other = oracle[(k + 1) % len(ladder)]
        assert int(other[1][b]) != n or not np.array_equal(other[0][b, :n], o_dst[b, :n]), (IDS[i], b, "two entries write one stream")


@pytest.mark.parametrize("i", [2, 4, 7], ids=[IDS[2], IDS[4], IDS[7]])
def test_one_choice_for_all_is_the_plain_call(runs, i):
    pk, d_src, oracle = runs(i)
    ladder = _ladder(SHAPES[i][0])
    for k in (1, 3):
        dst, sizes, out, used = _ladder_roundtrip(pk, d_src, ladder, [k] * NBLOCKS)
        o_dst, o_sizes, o_out, o_used = oracle[k]
        assert np.array_equal(sizes.view(np.int64), o_sizes) and np.array_equal(used.view(np.int64), o_used)
        for b in range(NBLOCKS):
            assert np.array_equal(dst[b, : int(sizes[b])], o_dst[b, : int(sizes[b])]) and np.array_equal(out[b], o_out[b]), (IDS[i], k, b)


@pytest.mark.parametrize("i", [1, 3, 4, 5], ids=[IDS[1], IDS[3], IDS[4], IDS[5]])
def test_quality_one_is_the_all_integer_kernels(api, runs, i):
    """a ladder entry of 1.0 divides in fp64 by n = 2^k: the streams of a fresh handle's integer kernels (k_fwht, k_fwht64k,
    k_fwht_cross), which rspt_hip_set_quantizer(1.0) selects -- oracle[1] of HAD_LADDER is that run"""
    assert HAD_LADDER[1] == 1.0
    pk, d_src, oracle = runs(i)
    dst, sizes, out, used = _ladder_roundtrip(pk, d_src, [1.0], [0] * NBLOCKS)
    o_dst, o_sizes, o_out, _ = oracle[1]
    for b in range(NBLOCKS):
        n = int(o_sizes[b])
        assert int(sizes[b]) == n and np.array_equal(dst[b, :n], o_dst[b, :n]) and np.array_equal(out[b], o_out[b]), (IDS[i], b)


@pytest.mark.parametrize("i", [2, 4, 5, 6], ids=[IDS[2], IDS[4], IDS[5], IDS[6]])
def test_a_choice_outside_the_ladder_flags_its_block_alone(runs, i):
    import torch

    pk, d_src, oracle = runs(i)
    ladder = _ladder(SHAPES[i][0])
    choice = [2, len(ladder), 3, -1, 1]  # (-1: 0xFFFFFFFF to the device)
    stride = (pk.max_compressed_size + 255) // 256 * 256
    d_dst = torch.full((NBLOCKS, stride), 0xC3, dtype=torch.uint8, device="cuda")
    dst, sizes, out, used = _ladder_roundtrip(pk, d_src, ladder, choice, d_dst=d_dst)
    for b, k in enumerate(choice):
        if 0 <= k < len(ladder):
            o_dst, o_sizes, o_out, o_used = oracle[k]
            n = int(o_sizes[b])
            assert int(sizes[b]) == n == int(used[b]) and np.array_equal(dst[b, :n], o_dst[b, :n]) and np.array_equal(out[b], o_out[b]), (IDS[i], b)
        else:
            assert int(sizes[b]) == BIT63 and int(used[b]) & BIT63, (IDS[i], b, hex(int(sizes[b])), hex(int(used[b])))
            assert (dst[b] == 0xC3).all() and (out[b] == 0x5A).all(), (IDS[i], b, "nothing is written")


@pytest.mark.parametrize("i", [2, 4, 5, 7], ids=[IDS[2], IDS[4], IDS[5], IDS[7]])
def test_decoding_with_another_choice_gives_other_samples(runs, i):
    """the table is read on the way back too"""
    import torch

    pk, d_src, oracle = runs(i)
    ladder = _ladder(SHAPES[i][0])
    d_choice = torch.tensor(CHOICE, dtype=torch.int32, device="cuda")
    d_dst, _ = pk.compress_batch(d_src, ladder=ladder, choice=d_choice)
    wrong = torch.tensor([(k + 1) % len(ladder) for k in CHOICE], dtype=torch.int32, device="cuda")
    d_out, d_used = pk.decompress_batch(d_dst, NBLOCKS, d_dst.shape[1], ladder=ladder, choice=wrong)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    for b, k in enumerate(CHOICE):
        assert not np.array_equal(out[b], oracle[k][2][b]), (IDS[i], b)
        assert int(d_used[b]) == int(oracle[k][1][b])  # (the stream itself is read the same)


def test_a_mixed_batch_is_the_reference_s_own_streams(api):
    """had_3x8 at quality 2 and 0.1, both at nb 2: the record's streams of the reference rebuilt with each, in one call"""
    import torch

    rec = {e["name"]: e for e in df.golden("lossy_quantizer_record.json")["cases"]}
    C_ = {c["name"]: c for c in lq.all_cases()}
    a, b = C_["had_3x8_q2_nb2"], C_["had_3x8_q0p1_nb2"]
    order = [(a, 0, 0), (b, 0, 1), (b, 1, 1), (a, 1, 0)]  # (case, its block, ladder index)
    data = [lq.block_data(c, j) for c, j, k in order]
    want = [rec[c["name"]]["blocks"][j] for c, j, k in order]
    for d, w in zip(data, want):
        assert lq.crc(d) == w["in_crc32"] and "stream" in w
    pk = _new(api, "hadamard", 4, 3, 8, 2)
    d_src = torch.from_numpy(np.stack(data)).cuda()
    dst, sizes, out, used = _ladder_roundtrip(pk, d_src, [a["q"], b["q"]], [k for c, j, k in order])
    for i, w in enumerate(want):
        assert dst[i, : int(sizes[i])].tobytes() == lq.unpack(w["stream"]), i
        assert int(used[i]) == w["size"] and lq.crc(out[i]) == w["dec_crc32"], i
    pk.close()


def test_refusals(api):
    import torch

    L = api.lib()
    d_choice = torch.zeros(2, dtype=torch.int32, device="cuda")

    def both(pk, ladder, choice=d_choice):
        """the status of the two entries for this ladder; nothing may be launched, so the buffers stay as they were"""
        lad = np.ascontiguousarray(ladder, dtype=np.float64)
        d_src = torch.zeros((2, pk.block_bytes), dtype=torch.uint8, device="cuda")
        d_dst = torch.full((2, 4096), 0x77, dtype=torch.uint8, device="cuda")
        d_sizes = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        lp = lad.ctypes.data_as(C.POINTER(C.c_double)) if lad.size else None
        rc = (L.rspt_hip_compress_batch_ladder_dev(pk._h, d_src.data_ptr(), 2, lp, lad.size, choice.data_ptr(), d_dst.data_ptr(), 4096, d_sizes.data_ptr(), None),
              L.rspt_hip_decompress_batch_ladder_dev(pk._h, d_dst.data_ptr(), 4096, 2, lp, lad.size, choice.data_ptr(), d_src.data_ptr(), d_sizes.data_ptr(), None))
        torch.cuda.synchronize()
        assert (d_dst == 0x77).all() and (d_sizes == -1).all() and (d_src == 0).all()
        return rc

    had = _new(api, "hadamard", 4, 3, 8, 3)
    assert both(had, []) == (ERR_ARG, ERR_ARG)
    assert both(had, [1.0] * 9) == (ERR_ARG, ERR_ARG)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-320):  # (1e-320: n / q is not finite) -- what rspt_hip_set_quantizer refuses
        with pytest.raises(api.RsptHipError):
            had.set_quantizer(bad)
        assert both(had, [1.0, bad]) == (ERR_ARG, ERR_ARG), bad
    had.close()
    natural = api.new_dct(4, 1, 16384)  # beyond the dense table: the FFT kernels
    forced = api.SignalPacker(api.KIND_DCT | api.DCT_FORCE_FFT, 4, 2, 64, 2)
    for pk in (natural, forced, api.new_hzr(4, 3, 8), api.new_xdelta_hzr(4, 3, 8, 2), api.new_bytes(64)):
        assert both(pk, [128.0]) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED), pk.kind
        pk.close()
    dense = api.new_dct(4, 3, 100)
    assert both(dense, [128.0, 0.0]) == (ERR_ARG, ERR_ARG)
    dense.close()
