"""Planar int32 in and out of the packers (rspt_hip_compress_planar_batch_dev, rspt_hip_decompress_planar_batch_dev,
rspt_hip_decompress_packed_planar_dev).

Without a GPU: a NULL handle is refused by all three entries before a device is looked for, and the model identity the GPU
tests compare against holds on the CPU oracle for every case.
On the GPU: every expected stream is the CPU oracle's stream of convert_cases.i32_to_native(P); equality with the native entry
on the GPU is a second assertion on top.  The one exception is the dct at ns = 2^k > 8192 (the fp64 FFT route, where the oracle
is a tolerance yardstick): there the planar stream equals the native entry's stream byte for byte.  Every comparison is
equality.
"""

import numpy as np
import pytest

import convert_cases as cc
import planar_cases as pc
from devframe import ERR_ARG

NB_CTOR = {"xdelta_hzr": 3, "hzr": 4, "dct": 2, "hadamard": 3}


# ---- without a GPU ------------------------------------------------------------------------------------------------------------
def test_null_handle_is_refused_without_a_device():
    from rspt_amd import api

    L = api.lib()
    buf = np.zeros(64, dtype=np.uint8)
    q = buf.ctypes.data
    assert L.rspt_hip_compress_planar_batch_dev(None, q, 1, q, 64, q, None) == ERR_ARG
    assert L.rspt_hip_decompress_planar_batch_dev(None, q, 64, 1, q, q, None) == ERR_ARG
    assert L.rspt_hip_decompress_packed_planar_dev(None, q, 64, 1, q, q, None) == ERR_ARG


def test_python_binding_has_the_planar_methods():
    from rspt_amd import api

    for name in ("compress_planar_batch", "decompress_planar_batch", "decompress_packed_planar"):
        assert callable(getattr(api.SignalPacker, name))


@pytest.mark.parametrize("nch,ns", pc.LOSSLESS_SHAPES)
def test_model_identity_on_the_oracle(orc, nch, ns):
    """What the GPU tests compare against: the oracle's stream of i32_to_native(P) decodes, through native_to_i32, to
    sign_extend(P, bps) for the lossless kinds; the byte order of the native block cancels out of the planar view."""
    for kind in pc.LOSSLESS:
        for bps in (1, 2, 3, 4):
            P = pc.noise(1, nch, ns, pc.seed_of(kind, bps, nch, ns)) if nch * ns <= 4096 else pc.walk(1, nch, ns, bps, pc.seed_of(kind, bps, nch, ns))
            streams, nbs = pc.oracle_streams(orc, kind, bps, nch, ns, NB_CTOR[kind], P)
            got = pc.oracle_decode(orc, kind, bps, nch, ns, [nb or 4 for nb in nbs], streams)
            assert np.array_equal(got, cc.sign_extend(P, bps)), (kind, bps)
            if nch * ns <= 4096:
                for be in (False, True):
                    assert np.array_equal(cc.native_to_i32(cc.i32_to_native(P[0], bps, be), bps, nch, ns, be), cc.sign_extend(P[0], bps))


def test_escalation_batch_needs_one_one_three_four_bytes(orc):
    nch, ns = 3, 5000
    _, nbs = pc.oracle_streams(orc, "xdelta_hzr", 4, nch, ns, 1, pc.escalation_batch(nch, ns))
    assert nbs == [1, 1, 3, 4]


# ---- GPU ------------------------------------------------------------------------------------------------------------------------
def _t(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _streams(d_dst, d_sizes):
    """the streams of a compress call as bytes (a flagged one: None), after a synchronisation"""
    import torch

    torch.cuda.synchronize()
    sizes = d_sizes.cpu().numpy().astype(np.uint64)
    dst = d_dst.cpu().numpy()
    return [None if int(s) >> 63 else dst[i, : int(s)].tobytes() for i, s in enumerate(sizes)], [int(s) for s in sizes]


def _rows(streams, stride=None):
    """streams -> a uint8 device tensor [n, stride], zero padded"""
    stride = stride or (max(len(s) for s in streams) + 271) // 256 * 256
    buf = np.zeros((len(streams), stride), dtype=np.uint8)
    for i, s in enumerate(streams):
        buf[i, : len(s)] = np.frombuffer(s, dtype=np.uint8)
    return _t(buf), stride


def _check_lossless(api, orc, kind, bps, nch, ns, nblocks, P):
    """compress_planar(P): streams, sizes and nb against the oracle and against the native entry; P unchanged; decompress_planar
    of those streams: sign_extend(P), consumed = sizes, against the native entry too"""
    import torch

    want, nbs = pc.oracle_streams(orc, kind, bps, nch, ns, NB_CTOR[kind], P)
    pk = api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind])
    d_P = _t(P)
    d_dst, d_sizes = pk.compress_planar_batch(d_P)
    got, sizes = _streams(d_dst, d_sizes)
    assert got == want, (kind, bps, nch, ns, nblocks, [len(s or b"") for s in got], [len(s) for s in want])
    assert sizes == [len(s) for s in want]
    if kind == "xdelta_hzr":
        assert pk.nb == nbs[-1]
    assert torch.equal(d_P, _t(P))
    # the native entry on a second handle
    pn = api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind])
    n_dst, n_sizes = pn.compress_batch(pn.from_planar_i32(d_P))
    assert _streams(n_dst, n_sizes)[0] == want
    # back: planar decode on the handle that compressed (its nb state is the streams')
    assert kind != "xdelta_hzr" or len(set(nbs)) == 1
    guard = torch.full((nblocks * nch * ns + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out = guard[4: 4 + nblocks * nch * ns]
    d_out, d_used = pk.decompress_planar_batch(d_dst, nblocks, d_dst.shape[1], d_out=out)
    n_out, n_used = pn.decompress_batch(n_dst, nblocks, n_dst.shape[1])
    n_planar = pn.to_planar_i32(n_out)
    torch.cuda.synchronize()
    assert torch.equal(d_used, d_sizes) and torch.equal(n_used, d_used)
    assert np.array_equal(d_out.cpu().numpy().reshape(nblocks, nch, ns), cc.sign_extend(P, bps))
    assert torch.equal(d_out.reshape(nblocks, nch, ns), n_planar)
    assert bool((guard[:4] == 0x5A5A5A5A).all()) and bool((guard[4 + nblocks * nch * ns:] == 0x5A5A5A5A).all())
    pk.close()
    pn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nch,ns", pc.LOSSLESS_SHAPES)
def test_lossless_packers_from_and_to_planar(orc, nch, ns):
    from rspt_amd import api

    for kind in pc.LOSSLESS:
        for bps in (1, 2, 3, 4):
            for nblocks in pc.BATCHES:
                _check_lossless(api, orc, kind, bps, nch, ns, nblocks, pc.walk(nblocks, nch, ns, bps, pc.seed_of(kind, bps, nch, ns, nblocks)))


def _check_lossy(api, orc, kind, bps, nch, ns, flags=0, oracle_is_exact=True):
    import torch

    nblocks = 2
    P = pc.walk(nblocks, nch, ns, bps, pc.seed_of(kind, bps, nch, ns))
    pk = api.SignalPacker(api.KINDS[kind] | flags, bps, nch, ns, NB_CTOR[kind])
    pn = api.SignalPacker(api.KINDS[kind] | flags, bps, nch, ns, NB_CTOR[kind])
    d_P = _t(P)
    d_dst, d_sizes = pk.compress_planar_batch(d_P)
    got, sizes = _streams(d_dst, d_sizes)
    assert torch.equal(d_P, _t(P)), "compress_planar wrote the caller's matrix"
    n_dst, n_sizes = pn.compress_batch(pn.from_planar_i32(d_P))
    native, _ = _streams(n_dst, n_sizes)
    assert got == native, (kind, bps, nch, ns)
    if oracle_is_exact:
        want, _ = pc.oracle_streams(orc, kind, bps, nch, ns, NB_CTOR[kind], P)
        assert got == want, (kind, bps, nch, ns)
    d_out, d_used = pk.decompress_planar_batch(d_dst, nblocks, d_dst.shape[1])
    n_out, n_used = pn.decompress_batch(n_dst, nblocks, n_dst.shape[1])
    n_planar = pn.to_planar_i32(n_out)
    torch.cuda.synchronize()
    assert torch.equal(d_used, d_sizes) and torch.equal(n_used, d_used)
    assert torch.equal(d_out, n_planar)
    if oracle_is_exact:
        assert np.array_equal(d_out.cpu().numpy(), pc.oracle_decode(orc, kind, bps, nch, ns, NB_CTOR[kind], got))
    pk.close()
    pn.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nch,ns", pc.HADAMARD_SHAPES)
def test_hadamard_from_and_to_planar(orc, nch, ns):
    from rspt_amd import api

    for bps in (2, 3, 4):
        _check_lossy(api, orc, "hadamard", bps, nch, ns)


@pytest.mark.gpu
@pytest.mark.parametrize("nch,ns", pc.DCT_SHAPES)
def test_dct_from_and_to_planar(orc, nch, ns):
    from rspt_amd import api

    fft = ns > 8192  # the fp64 FFT route: the native entry's stream is the yardstick (module docstring)
    for bps in (2, 3, 4):
        _check_lossy(api, orc, "dct", bps, nch, ns, oracle_is_exact=not fft)


@pytest.mark.gpu
def test_dct_forced_fft_route_from_planar(orc):
    """the FFT route at a small ns through the test hook: the ingest kernel's channel sums feed the means"""
    from rspt_amd import api

    for bps in (2, 4):
        _check_lossy(api, orc, "dct", bps, 3, 256, flags=api.DCT_FORCE_FFT, oracle_is_exact=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,nch,ns", [("hadamard", 3, 16), ("dct", 3, 17)])
def test_transform_packers_cut_values_outside_the_sample_width(orc, kind, nch, ns):
    """full-range int32 into a transform packer with bps 2 and 3: the ingest kernel cuts to the sample width, so the streams are
    the oracle's of i32_to_native(P), the same as those of sign_extend(P), and P stays as it was"""
    import torch

    from rspt_amd import api

    for bps in (2, 3):
        P = pc.noise(2, nch, ns, 311 + bps)
        want, _ = pc.oracle_streams(orc, kind, bps, nch, ns, NB_CTOR[kind], P)
        pk, pk2 = api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind]), api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind])
        d_P = _t(P)
        assert _streams(*pk.compress_planar_batch(d_P))[0] == want, (kind, bps)
        assert _streams(*pk2.compress_planar_batch(_t(cc.sign_extend(P, bps))))[0] == want, (kind, bps)
        assert torch.equal(d_P, _t(P))
        pk.close()
        pk2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", pc.LOSSLESS)
def test_values_outside_the_sample_width(orc, kind):
    """full-range int32 with bps 1, 2, 3: the streams are those of sign_extend(P), the decoded values are sign-extended"""
    import torch

    from rspt_amd import api

    for bps in (1, 2, 3):
        for nch, ns in ((3, 17), (5, 4099)):
            P = pc.noise(2, nch, ns, 77 + bps)
            want, nbs = pc.oracle_streams(orc, kind, bps, nch, ns, NB_CTOR[kind], P)
            pk = api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind])
            d_dst, d_sizes = pk.compress_planar_batch(_t(P))
            got, _ = _streams(d_dst, d_sizes)
            assert got == want
            pk2 = api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind])
            d2, s2 = pk2.compress_planar_batch(_t(cc.sign_extend(P, bps)))
            assert _streams(d2, s2)[0] == want
            assert len(set(nbs)) == 1
            d_out, d_used = pk.decompress_planar_batch(d_dst, 2, d_dst.shape[1])
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), cc.sign_extend(P, bps))
            pk.close()
            pk2.close()


@pytest.mark.gpu
def test_alignment_and_a_foreign_stream(orc):
    """d_planar at +4, +8 and +12 bytes from a 16-byte boundary on both entries, on a stream that is not the current one"""
    import torch

    from rspt_amd import api

    s = torch.cuda.Stream()
    for kind, bps, nch, ns in (("xdelta_hzr", 4, 3, 30000), ("hzr", 3, 5, 4099), ("hadamard", 4, 3, 1024), ("dct", 2, 3, 17), ("xdelta_hzr", 2, 4, 16384)):
        P = pc.walk(2, nch, ns, bps, 500 + ns)
        n = P.size
        want, _ = pc.oracle_streams(orc, kind, bps, nch, ns, NB_CTOR[kind], P)
        for off in (1, 2, 3):
            pk = api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind])
            src = torch.zeros(n + 4, dtype=torch.int32, device="cuda")
            assert src.data_ptr() % 16 == 0
            src[off: off + n] = _t(P).reshape(-1)
            dst = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            d_dst, d_sizes = pk.compress_planar_batch(src[off: off + n], stream=s.cuda_stream)
            d_out, d_used = pk.decompress_planar_batch(d_dst, 2, d_dst.shape[1], d_out=dst[off: off + n], stream=s.cuda_stream)
            got, _ = _streams(d_dst, d_sizes)
            assert got == want, (kind, off)
            ref = pk.to_planar_i32(pk.decompress_batch(d_dst, 2, d_dst.shape[1])[0])
            torch.cuda.synchronize()
            assert torch.equal(d_used, d_sizes) and torch.equal(d_out.reshape(-1), ref.reshape(-1)), (kind, off)
            if kind in pc.LOSSLESS:
                assert np.array_equal(d_out.cpu().numpy().reshape(P.shape), cc.sign_extend(P, bps))
            assert bool((dst[:off] == 0x5A5A5A5A).all()) and bool((dst[off + n:] == 0x5A5A5A5A).all())
            pk.close()


@pytest.mark.gpu
def test_escalation_inside_a_batch(orc):
    """xdelta created with nb = 1; blocks 2 and 3 need three and four bytes: streams, sizes and the nb state are the oracle's
    sequence, also over a second call on the same handle"""
    from rspt_amd import api

    nch, ns = 3, 5000
    P = pc.escalation_batch(nch, ns)
    po = orc.packer("xdelta_hzr", 4, nch, ns, 1)
    pk = api.new_xdelta_hzr(4, nch, ns, 1)
    want, nbs = pc.oracle_streams(orc, "xdelta_hzr", 4, nch, ns, 1, P, po)
    assert nbs == [1, 1, 3, 4]
    got, sizes = _streams(*pk.compress_planar_batch(_t(P)))
    assert got == want and sizes == [len(s) for s in want] and pk.nb == 4
    want2, _ = pc.oracle_streams(orc, "xdelta_hzr", 4, nch, ns, 1, P[:2], po)
    got2, _ = _streams(*pk.compress_planar_batch(_t(P[:2])))
    assert got2 == want2 and pk.nb == 4
    # and from nb = 1 to 3 only, then a native call on the same handle
    pk3, po3 = api.new_xdelta_hzr(4, nch, ns, 1), orc.packer("xdelta_hzr", 4, nch, ns, 1)
    want3, nbs3 = pc.oracle_streams(orc, "xdelta_hzr", 4, nch, ns, 1, P[:3], po3)
    got3, _ = _streams(*pk3.compress_planar_batch(_t(P[:3])))
    assert got3 == want3 and nbs3 == [1, 1, 3]
    want4, _ = pc.oracle_streams(orc, "xdelta_hzr", 4, nch, ns, 1, P[3:], po3)
    got4, _ = _streams(*pk3.compress_batch(pk3.from_planar_i32(_t(P[3:]))))
    assert got4 == want4 and pk3.nb == 4
    for h in (pk, pk3, po, po3):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", pc.LOSSLESS)
def test_clean_block_invariant_across_the_entries(orc, kind):
    """one (4, 65536) int32 handle; planar dense, native quiet, planar quiet, native dense, planar quiet, planar dense, then a
    decompress between two compresses (it marks every plane dirty): every stream is the oracle's"""
    import torch

    from rspt_amd import api

    nch, ns = 4, 65536
    pk = api.SignalPacker(kind, 4, nch, ns, NB_CTOR[kind])
    po = orc.packer(kind, 4, nch, ns, NB_CTOR[kind])
    dense, quiet = pc.noise(1, nch, ns, 31), pc.quiet(1, nch, ns, 32)
    last = None
    for i, (planar, P) in enumerate([(True, dense), (False, quiet), (True, quiet), (False, dense), (True, quiet), (True, dense), (True, quiet)]):
        if i == 6:  # a decode of the dense streams lands in the planes; the quiet block behind it must not inherit them
            d_out, d_used = pk.decompress_planar_batch(last[0], 1, last[0].shape[1])
            torch.cuda.synchronize()
            assert np.array_equal(d_out.cpu().numpy(), dense) and torch.equal(d_used, last[1])
        want, _ = pc.oracle_streams(orc, kind, 4, nch, ns, NB_CTOR[kind], P, po)
        last = pk.compress_planar_batch(_t(P)) if planar else pk.compress_batch(pk.from_planar_i32(_t(P)))
        got, _ = _streams(*last)
        assert got == want, (kind, i)
    pk.close()
    po.close()


@pytest.mark.gpu
def test_byte_order_has_no_effect(orc):
    import torch

    from rspt_amd import api

    for kind, bps, nch, ns in (("xdelta_hzr", 3, 5, 4099), ("hzr", 2, 12, 64), ("hadamard", 4, 3, 16), ("dct", 3, 3, 17)):
        P = pc.walk(2, nch, ns, bps, 900 + bps)
        le, be = api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind]), api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind])
        be.set_byte_order(True)
        want, _ = pc.oracle_streams(orc, kind, bps, nch, ns, NB_CTOR[kind], P)
        a = le.compress_planar_batch(_t(P))
        b = be.compress_planar_batch(_t(P))
        assert _streams(*a)[0] == want and _streams(*b)[0] == want, kind
        oa, _ = le.decompress_planar_batch(a[0], 2, a[0].shape[1])
        ob, _ = be.decompress_planar_batch(b[0], 2, b[0].shape[1])
        torch.cuda.synchronize()
        assert torch.equal(oa, ob), kind
        le.close()
        be.close()


@pytest.mark.gpu
def test_container_with_mixed_nb(orc):
    """compress_planar_batch -> pack_batch -> decompress_packed_planar: every stream decoded with the nb of its index entry"""
    import torch

    from rspt_amd import api

    nch, ns = 3, 5000
    P = pc.escalation_batch(nch, ns)
    pk = api.new_xdelta_hzr(4, nch, ns, 1)
    d_dst, d_sizes = pk.compress_planar_batch(_t(P))
    packed, total = pk.pack_batch(d_dst, d_sizes)
    torch.cuda.synchronize()
    other = api.new_xdelta_hzr(4, nch, ns, 2)
    guard = torch.full((P.size + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out, used = other.decompress_packed_planar(packed[: int(total.item())], d_out=guard[4: 4 + P.size])
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().reshape(P.shape), P) and torch.equal(used, d_sizes)
    assert bool((guard[:4] == 0x5A5A5A5A).all()) and bool((guard[4 + P.size:] == 0x5A5A5A5A).all())
    assert other.nb == 2  # (the handle's nb state is neither used nor changed)
    pk.close()
    other.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", pc.LOSSLESS)
def test_damaged_input_is_flagged_as_by_the_native_entry(orc, kind):
    """a truncated stream and one with a broken length field, built on the CPU from a sound one: bit 63 and d_consumed are the
    native entry's, the sound neighbour decodes, the words around d_planar stay untouched; with and without verification"""
    import torch

    from rspt_amd import api

    bps, nch, ns = 4, 3, 30000
    P = pc.walk(1, nch, ns, bps, 41)
    (sound,), _ = pc.oracle_streams(orc, kind, bps, nch, ns, NB_CTOR[kind], P)
    cut = bytearray(sound)
    cut[len(cut) // 2:] = bytes(len(cut) - len(cut) // 2)  # framing and payload gone behind the middle
    broken = bytearray(sound)
    broken[1:5] = (0xFFFFFFF0).to_bytes(4, "little")  # the first plane's length word
    rows, stride = _rows([sound, bytes(cut), bytes(broken), sound])
    for verify in (False, True):
        pk = api.SignalPacker(kind, bps, nch, ns, NB_CTOR[kind])
        pk.set_verify(verify)
        n = 4 * nch * ns
        guard = torch.full((n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        d_out, d_used = pk.decompress_planar_batch(rows, 4, stride, d_out=guard[4: 4 + n])
        _, n_used = pk.decompress_batch(rows, 4, stride)
        torch.cuda.synchronize()
        used = d_used.cpu().numpy().astype(np.uint64)
        assert torch.equal(d_used, n_used)
        assert [int(u) >> 63 for u in used] == [0, 1, 1, 0] and int(used[0]) == int(used[3]) == len(sound)
        out = d_out.cpu().numpy().reshape(4, nch, ns)
        assert np.array_equal(out[0], P[0]) and np.array_equal(out[3], P[0])
        assert bool((guard[:4] == 0x5A5A5A5A).all()) and bool((guard[4 + n:] == 0x5A5A5A5A).all())
        pk.close()


@pytest.mark.gpu
def test_a_short_dst_stride_flags_the_block_and_spares_its_neighbours(orc):
    import torch

    from rspt_amd import api

    nch, ns = 4, 16384
    P = np.concatenate([pc.quiet(1, nch, ns, 1), pc.noise(1, nch, ns, 2), pc.quiet(1, nch, ns, 3)])
    want, _ = pc.oracle_streams(orc, "hzr", 4, nch, ns, 4, P)
    stride = (max(len(want[0]), len(want[2])) + 64 + 15) // 16 * 16
    assert stride < len(want[1])
    pk = api.new_hzr(4, nch, ns)
    d_dst = torch.full((3, stride), 0xA5, dtype=torch.uint8, device="cuda")
    _, d_sizes = pk.compress_planar_batch(_t(P), d_dst=d_dst, dst_stride=stride)
    got, sizes = _streams(d_dst, d_sizes)
    assert got[0] == want[0] and got[2] == want[2] and got[1] is None
    assert sizes[1] >> 63 and bool((d_dst[1] == 0xA5).all())
    # the native entry says the same of the same blocks
    pn = api.new_hzr(4, nch, ns)
    n_dst = torch.full((3, stride), 0xA5, dtype=torch.uint8, device="cuda")
    _, n_sizes = pn.compress_batch(pn.from_planar_i32(_t(P)), d_dst=n_dst, dst_stride=stride)
    torch.cuda.synchronize()
    assert torch.equal(n_sizes, d_sizes)
    pk.close()
    pn.close()


@pytest.mark.gpu
def test_refusals_write_nothing():
    import torch

    from rspt_amd import api

    L = api.lib()
    bps, nch, ns, nb = 3, 12, 65, 2
    pk = api.new_hzr(bps, nch, ns)
    raw = api.new_bytes(4096)
    planar = torch.full((nb * nch * ns + 4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    stride = (pk.max_compressed_size + 255) // 256 * 256
    dst = torch.full((nb * stride,), 0x5A, dtype=torch.uint8, device="cuda")
    sizes = torch.full((nb,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    h, p, d, s = pk._h, planar.data_ptr(), dst.data_ptr(), sizes.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    comp, dec, decp = L.rspt_hip_compress_planar_batch_dev, L.rspt_hip_decompress_planar_batch_dev, L.rspt_hip_decompress_packed_planar_dev

    def refused():
        return [
            (comp, (h, None, nb, d, stride, s, st)), (comp, (h, p, nb, None, stride, s, st)), (comp, (h, p, nb, d, stride, None, st)),
            (comp, (h, p, 0, d, stride, s, st)), (comp, (h, p + 1, nb, d, stride, s, st)), (comp, (h, p + 2, nb, d, stride, s, st)),
            (comp, (h, p, 65536, d, stride, s, st)), (comp, (raw._h, p, 1, d, stride, s, st)),
            (dec, (h, None, stride, nb, p, s, st)), (dec, (h, d, stride, nb, None, s, st)), (dec, (h, d, stride, nb, p, None, st)),
            (dec, (h, d, stride, 0, p, s, st)), (dec, (h, d, stride, nb, p + 3, s, st)), (dec, (h, d, stride, 65536, p, s, st)),
            (dec, (raw._h, d, stride, 1, p, s, st)),
            (decp, (h, None, nb * stride, nb, p, s, st)), (decp, (h, d, nb * stride, nb, None, s, st)), (decp, (h, d, nb * stride, nb, p, None, st)),
            (decp, (h, d, nb * stride, 0, p, s, st)), (decp, (h, d, nb * stride, nb, p + 2, s, st)), (decp, (h, d + 8, nb * stride, nb, p, s, st)),
            (decp, (h, d, nb * stride, 65536, p, s, st)), (decp, (raw._h, d, nb * stride, 1, p, s, st)),
        ]

    for f, a in refused():
        assert f(*a) == ERR_ARG, a[1:5]
    pk.feed_begin(1, 2)  # an open feed owns the workspace
    assert comp(h, p, nb, d, stride, s, st) == ERR_ARG and dec(h, d, stride, nb, p, s, st) == ERR_ARG
    assert decp(h, d, nb * stride, nb, p, s, st) == ERR_ARG
    pk.feed_end()
    torch.cuda.synchronize()
    assert bool((planar == 0x5A5A5A5A).all()) and bool((dst == 0x5A).all()) and bool((sizes == 0x5A5A5A5A).all())
    # and a valid call still works on the same handle
    P = pc.walk(nb, nch, ns, bps, 5)
    d_dst, d_sizes = pk.compress_planar_batch(_t(P))
    d_out, d_used = pk.decompress_planar_batch(d_dst, nb, d_dst.shape[1])
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), P) and torch.equal(d_used, d_sizes)
    pk.close()
    raw.close()
