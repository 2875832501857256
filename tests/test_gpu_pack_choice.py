"""The per-block choice of a ladder compress in the container index (rspt_hip_pack_batch_choice_dev,
rspt_hip_decompress_packed_ladder_dev, rspt_hip_decompress_packed_planar_ladder_dev): bits 60..62 of each stream's length word.
1030 streams -- past the 1024-entry round of the index kernel -- of hadamard 3 x 8 at a ladder of eight, two of them refused at
compress time; the container against rspt_hip_pack_batch_dev's; the two decoders against the ladder decoders given the choices
by hand; a shorter ladder at decode time; the decoders that know no choice; a truncated container; and the dense dct."""
import ctypes as C

import numpy as np
import pytest

import cases
import lossy_quantizer_cases as lq
from devframe import ERR_ARG, ERR_CORRUPT, ERR_UNSUPPORTED, api  # noqa: F401

pytestmark = pytest.mark.gpu

BIT63 = 1 << 63
CHOICE_MASK = np.uint64(7 << 60)
HAD8 = [1.0 / 16, 1.0 / 8, 1.0 / 4, 1.0 / 2, 1.0, 2.0, 4.0, 64.0]
DCT4 = [1000.0, 128.0, 8.0, 0.37]


def _new(api, kind, bps, nch, ns, nb):
    pk = api.SignalPacker(lq.KIND_ID[kind], bps, nch, ns, lq.DEFAULTS[kind][1])
    pk.set_quantizer(nb=nb)
    return pk


def _index(cont, nblocks):
    """(offsets, length words) of a container's bytes"""
    idx = np.frombuffer(cont[32 : 32 + 16 * nblocks].tobytes(), dtype=np.uint64).reshape(nblocks, 2)
    return idx[:, 0].copy(), idx[:, 1].copy()


def _without_choice(cont, nblocks):
    c = cont.copy()
    words = c[32 : 32 + 16 * nblocks].view(np.uint64).reshape(nblocks, 2)
    words[:, 1] &= ~CHOICE_MASK
    return c


def _setup(api, kind, bps, nch, ns, nb, ladder, choice, amp=3000):
    """compress with the ladder, then every container the test wants, before anything else touches the handle"""
    import torch

    nblocks = len(choice)
    pk = _new(api, kind, bps, nch, ns, nb)
    rng = np.random.default_rng(1234 + ns)
    if bps == 4:
        x = rng.integers(-amp, amp, size=(nblocks, ns, nch)).astype(np.int32)
        d_src = torch.from_numpy(x.view(np.uint8).reshape(nblocks, -1)).cuda()
    else:
        d_src = torch.from_numpy(np.stack([cases._rand_native(nch, ns, bps, 7100 + i, amp, walk=False) for i in range(nblocks)])).cuda()
    d_choice = torch.tensor(choice, dtype=torch.int32, device="cuda")
    stride = (pk.max_compressed_size + 255) // 256 * 256
    d_dst, d_sizes = pk.compress_batch(d_src, d_dst=torch.full((nblocks, stride), 0xC3, dtype=torch.uint8, device="cuda"), ladder=ladder, choice=d_choice)
    K = len(ladder)
    conts = {}
    for tag, kw in (("plain", {}), ("choice", dict(choice=d_choice, nladder=K)), ("zeros", dict(choice=torch.zeros_like(d_choice), nladder=K)),
                    ("short", dict(choice=d_choice, nladder=3))):
        d_packed, d_total = pk.pack_batch(d_dst, d_sizes, **kw)
        torch.cuda.synchronize()
        conts[tag] = d_packed[: int(d_total.item())].clone()  # (each container ends where its allocation ends)
    return pk, d_src, d_choice, d_dst, d_sizes, stride, conts


def _decoded(pk, fn, *a, planar=False, **kw):
    """(out bytes, consumed) of a decoder writing into a buffer of 0x5A"""
    import torch

    nblocks = kw.pop("nblocks")
    d_out = (torch.full((nblocks, pk.nch, pk.ns), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if planar
             else torch.full((nblocks, pk.block_bytes), 0x5A, dtype=torch.uint8, device="cuda"))
    out, used = fn(*a, d_out=d_out, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint8).reshape(nblocks, -1), used.cpu().numpy().view(np.uint64)


def test_1030_streams_of_a_ladder_of_eight(api):
    import torch

    nblocks, K = 1030, 8
    choice = [b % K for b in range(nblocks)]
    refused = [5, 1027]  # outside the ladder at compress time: flagged in d_sizes
    choice[5], choice[1027] = K, -1
    pk, d_src, d_choice, d_dst, d_sizes, stride, conts = _setup(api, "hadamard", 4, 3, 8, 3, HAD8, choice)
    sizes = d_sizes.cpu().numpy().view(np.uint64)
    assert [b for b in range(nblocks) if int(sizes[b]) >> 63] == refused and all(int(sizes[b]) == BIT63 for b in refused)
    plain, cont, zeros, short = [conts[t].cpu().numpy() for t in ("plain", "choice", "zeros", "short")]

    # the container against pack_batch's: identical but for bits 60..62, which are the choices; all-zero choices: the same bytes
    assert cont.size == plain.size and np.array_equal(_without_choice(cont, nblocks), plain)
    assert not np.array_equal(cont, plain) and np.array_equal(_without_choice(plain, nblocks), plain)
    assert np.array_equal(zeros, plain)
    offs, words = _index(cont, nblocks)
    for b in range(nblocks):
        w = int(words[b])
        if b in refused:
            assert w >> 63 == 1 and (w >> 60) & 7 == 0 and w & ((1 << 56) - 1) == 0, (b, hex(w))
        else:
            assert w >> 63 == 0 and (w >> 60) & 7 == choice[b] and w & ((1 << 56) - 1) == int(sizes[b]) and (w >> 56) & 0xF == 3, (b, hex(w))
    assert int(cont[24:32].view(np.uint64)[0]) >> 32 == len(refused)

    # a choice outside the (shorter) ladder on a block that was written: an empty flagged entry, never an alias
    _, swords = _index(short, nblocks)
    late = [b for b in range(nblocks) if b in refused or choice[b] >= 3]
    for b in range(nblocks):
        w = int(swords[b])
        if b in late:
            assert w >> 63 == 1 and (w >> 60) & 7 == 0 and w & ((1 << 56) - 1) == 0, (b, hex(w))
        else:
            assert w == int(words[b]), (b, hex(w))
    assert int(short[24:32].view(np.uint64)[0]) >> 32 == len(late) and short.size < cont.size

    # the two decoders against the ladder decoders given the choices by hand
    want, wused = _decoded(pk, pk.decompress_batch, d_dst, nblocks, stride, nblocks=nblocks, ladder=HAD8, choice=d_choice)
    got, used = _decoded(pk, pk.decompress_packed, conts["choice"], nblocks=nblocks, ladder=HAD8)
    wantp, wusedp = _decoded(pk, pk.decompress_planar_batch, d_dst, nblocks, stride, nblocks=nblocks, planar=True, ladder=HAD8, choice=d_choice)
    gotp, usedp = _decoded(pk, pk.decompress_packed_planar, conts["choice"], nblocks=nblocks, planar=True, ladder=HAD8)
    assert np.array_equal(got, want) and np.array_equal(gotp, wantp)
    for b in range(nblocks):
        if b in refused:  # flagged and untouched
            assert int(used[b]) >> 63 and int(usedp[b]) >> 63 and (got[b] == 0x5A).all() and (gotp[b] == 0x5A).all(), b
        else:
            assert int(used[b]) == int(wused[b]) == int(sizes[b]) == int(usedp[b]) == int(wusedp[b]), b
    assert len({got[b].tobytes() for b in range(nblocks)}) > nblocks // 2  # (the blocks differ: a decoder cannot have mixed them up unseen)

    # the same container with a ladder of three: exactly the blocks whose stored choice is >= 3 are flagged, and not written
    got3, used3 = _decoded(pk, pk.decompress_packed, conts["choice"], nblocks=nblocks, ladder=HAD8[:3])
    for b in range(nblocks):
        if b in late:
            assert int(used3[b]) >> 63 and (got3[b] == 0x5A).all(), b
        else:
            assert int(used3[b]) == int(sizes[b]) and np.array_equal(got3[b], want[b]), b

    # the decoders that know no choice ignore bits 60..62
    for planar in (False, True):
        fn = pk.decompress_packed_planar if planar else pk.decompress_packed
        a, au = _decoded(pk, fn, conts["plain"], nblocks=nblocks, planar=planar)
        b_, bu = _decoded(pk, fn, conts["choice"], nblocks=nblocks, planar=planar)
        assert np.array_equal(a, b_) and np.array_equal(au, bu), planar

    # a truncated container: inside the index -- refused on the host before the device reads the index, nothing written; inside
    # the payload -- the streams decompress_packed flags
    L = api.lib()
    lad = np.ascontiguousarray(HAD8, dtype=np.float64)
    lp = lad.ctypes.data_as(C.POINTER(C.c_double))
    total = cont.size
    for entry, planar in ((L.rspt_hip_decompress_packed_ladder_dev, False), (L.rspt_hip_decompress_packed_planar_ladder_dev, True)):
        cut = 32 + 16 * nblocks - 8
        piece = conts["choice"][:cut].clone()
        d_out = torch.full((nblocks, pk.block_bytes), 0x5A, dtype=torch.uint8, device="cuda")
        d_used = torch.full((nblocks,), -1, dtype=torch.int64, device="cuda")
        assert entry(pk._h, piece.data_ptr(), cut, nblocks, lp, lad.size, d_out.data_ptr(), d_used.data_ptr(), None) == ERR_CORRUPT
        torch.cuda.synchronize()
        assert (d_out == 0x5A).all() and (d_used == -1).all()
        assert entry(pk._h, conts["choice"].data_ptr(), total, nblocks, None, 8, d_out.data_ptr(), d_used.data_ptr(), None) == ERR_ARG
        assert entry(pk._h, conts["choice"].data_ptr(), total, nblocks, lp, 9, d_out.data_ptr(), d_used.data_ptr(), None) == ERR_ARG
        assert entry(pk._h, conts["choice"].data_ptr() + 8, total - 8, nblocks, lp, 8, d_out.data_ptr(), d_used.data_ptr(), None) == ERR_ARG
        torch.cuda.synchronize()
        assert (d_out == 0x5A).all() and (d_used == -1).all()
    cut = (32 + 16 * nblocks + (total - 32 - 16 * nblocks) // 2) & ~15
    piece = conts["choice"][:cut].clone()
    _, pu = _decoded(pk, pk.decompress_packed, piece, nblocks=nblocks)
    for planar in (False, True):
        fn = pk.decompress_packed_planar if planar else pk.decompress_packed
        t, tu = _decoded(pk, fn, piece, nblocks=nblocks, planar=planar, ladder=HAD8)
        assert [int(x) >> 63 for x in tu] == [int(x) >> 63 for x in pu] and any(int(x) >> 63 for x in tu)
        for b in range(nblocks):  # (what a stream flagged for its container leaves in its block is as unspecified as decompress_packed's)
            if not int(tu[b]) >> 63:
                assert np.array_equal(t[b], (wantp if planar else want)[b]), (planar, b)
    assert L.rspt_hip_last_hip_error(pk._h) == 0
    pk.close()


def test_the_dense_dct(api):
    nblocks = 4
    choice = [0, 3, 1, 2]
    pk, d_src, d_choice, d_dst, d_sizes, stride, conts = _setup(api, "dct", 4, 3, 100, 2, DCT4, choice)
    sizes = d_sizes.cpu().numpy().view(np.uint64)
    plain, cont = conts["plain"].cpu().numpy(), conts["choice"].cpu().numpy()
    assert np.array_equal(_without_choice(cont, nblocks), plain) and np.array_equal(conts["zeros"].cpu().numpy(), plain)
    _, words = _index(cont, nblocks)
    assert [(int(w) >> 60) & 7 for w in words] == choice and not any(int(w) >> 63 for w in words)
    want, wused = _decoded(pk, pk.decompress_batch, d_dst, nblocks, stride, nblocks=nblocks, ladder=DCT4, choice=d_choice)
    got, used = _decoded(pk, pk.decompress_packed, conts["choice"], nblocks=nblocks, ladder=DCT4)
    wantp, wusedp = _decoded(pk, pk.decompress_planar_batch, d_dst, nblocks, stride, nblocks=nblocks, planar=True, ladder=DCT4, choice=d_choice)
    gotp, usedp = _decoded(pk, pk.decompress_packed_planar, conts["choice"], nblocks=nblocks, planar=True, ladder=DCT4)
    assert np.array_equal(got, want) and np.array_equal(gotp, wantp)
    assert np.array_equal(used, wused) and np.array_equal(usedp, wusedp) and np.array_equal(used, sizes)
    assert np.array_equal(gotp.view(np.int32).reshape(nblocks, 3, 100).transpose(0, 2, 1).reshape(nblocks, -1), got.view(np.int32))
    pk.close()


def test_refusals(api):
    import torch

    L = api.lib()

    def status(pk, nladder, nblocks=2, choice_off=0):
        stride = 4096
        d_src = torch.zeros((nblocks, pk.block_bytes), dtype=torch.uint8, device="cuda")
        d_dst, d_sizes = pk.compress_batch(d_src, dst_stride=stride, d_dst=torch.zeros((nblocks, stride), dtype=torch.uint8, device="cuda"))
        d_choice = torch.zeros(nblocks + 1, dtype=torch.int32, device="cuda")
        d_packed = torch.full((pk.pack_bound(nblocks),), 0x77, dtype=torch.uint8, device="cuda")
        d_total = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        rc = L.rspt_hip_pack_batch_choice_dev(pk._h, d_dst.data_ptr(), stride, d_sizes.data_ptr(), nblocks, d_choice.data_ptr() + choice_off, nladder,
                                              d_packed.data_ptr(), d_total.data_ptr(), None)
        torch.cuda.synchronize()
        if rc:
            assert (d_packed == 0x77).all() and int(d_total.item()) == -1
        return rc

    had = api.new_hadamard(4, 3, 8)
    assert status(had, 1) == 0 and status(had, 8) == 0
    assert status(had, 0) == ERR_ARG and status(had, 9) == ERR_ARG and status(had, 2, choice_off=2) == ERR_ARG
    had.close()
    for pk in (api.SignalPacker(api.KIND_DCT | api.DCT_FORCE_FFT, 4, 2, 64, 2), api.new_hzr(4, 3, 8), api.new_xdelta_hzr(4, 3, 8, 2), api.new_bytes(64)):
        assert status(pk, 2) == ERR_UNSUPPORTED, pk.kind
        pk.close()
