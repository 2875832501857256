"""The quality ladder on the planar int32 matrix (rspt_hip_compress_planar_batch_ladder_dev,
rspt_hip_decompress_planar_batch_ladder_dev), held to the two identities of include/rspt_hip.h with the native ladder entries --
which tests/test_gpu_ladder.py holds to the composed oracle -- on the same device:

    compress_planar_ladder(P, ladder, choice)    == compress_batch_ladder(i32_to_native(P), ladder, choice)
    decompress_planar_ladder(S, ladder, choice)  == native_to_i32(decompress_batch_ladder(S, ladder, choice))

with two choices outside the ladder among four blocks (exactly bit 63, nothing written: not one byte of their rows, next to a
served block inside one workgroup of the emit kernel), from a base 4 bytes past a 16-byte boundary, with garbage above the sample
width, and the handle's own quantiser and plain planar streams untouched; then the refusals."""
import ctypes as C

import numpy as np
import pytest

import cases
import devframe as df
import lossy_quantizer_cases as lq
import target_planar_cases as tp
from devframe import ERR_ARG, ERR_UNSUPPORTED, api  # noqa: F401

pytestmark = pytest.mark.gpu

BIT63 = 1 << 63
HAD_LADDER = [0.1, 1.0, 3.0, 7.3]
DCT_LADDER = [1000.0, 128.0, 8.0, 0.37]
# (kind, bps, nch, ns, nb, amplitude)
SHAPES = [("hadamard", 4, 3, 8, 3, 3000), ("hadamard", 2, 5, 1024, 2, 3000), ("dct", 4, 3, 100, 2, 3000), ("dct", 3, 2, 257, 3, 1 << 20)]
IDS = ["%s_i%d_%dx%d_nb%d" % (k, 8 * bps, nch, ns, nb) for k, bps, nch, ns, nb, amp in SHAPES]
NBLOCKS = 4
# (tag, bytes past a 16-byte boundary, garbage above the sample width)
VARIANTS = [("base0", 0, False), ("base4", 4, False), ("garbage", 0, True), ("garbage_base4", 4, True)]
RUNS = [(i, v) for i in range(len(SHAPES)) for v in VARIANTS if not v[2] or SHAPES[i][1] < 4]


def _ladder(kind):
    return HAD_LADDER if kind == "hadamard" else DCT_LADDER


def _new(api, kind, bps, nch, ns, nb, flags=0):
    pk = api.SignalPacker(lq.KIND_ID[kind] | flags, bps, nch, ns, lq.DEFAULTS[kind][1])
    pk.set_quantizer(nb=nb)
    return pk


def _matrix(bps, nch, ns, amp, garbage):
    P = np.stack([lq.native_to_i32(cases._rand_native(nch, ns, bps, 6600 + 11 * i + ns % 89, amp, walk=(i & 1) == 1), bps, nch, ns)
                  for i in range(NBLOCKS)]).astype(np.int32)
    if garbage:
        hi = np.random.default_rng(4242 + ns).integers(0, 1 << (32 - 8 * bps), size=P.shape, dtype=np.uint64).astype(np.uint32)
        G = ((P.view(np.uint32) & np.uint32((1 << (8 * bps)) - 1)) | (hi << np.uint32(8 * bps))).view(np.int32)
        assert np.array_equal(tp.cut(G, bps), P) and (G != P).mean() > 0.9
        return P, G
    return P, P


@pytest.mark.parametrize("i,variant", RUNS, ids=["%s-%s" % (IDS[i], v[0]) for i, v in RUNS])
def test_both_identities_with_two_blocks_refused(api, i, variant):
    import torch

    kind, bps, nch, ns, nb, amp = SHAPES[i]
    tag, off, garbage = variant
    ladder = _ladder(kind)
    K = len(ladder)
    choice = [0, K, K - 1, -1]  # (-1: 0xFFFFFFFF to the device)
    served = [b for b, k in enumerate(choice) if 0 <= k < K]
    d_choice = torch.tensor(choice, dtype=torch.int32, device="cuda")
    clean, P = _matrix(bps, nch, ns, amp, garbage)
    pk = _new(api, kind, bps, nch, ns, nb)
    own = pk.quantizer()
    sraw, src = df.guarded_matrix(P, off)
    stride = (pk.max_compressed_size + 255) // 256 * 256
    plain_before, plain_sizes = [t.cpu().numpy() for t in pk.compress_planar_batch(src)]

    # oracle (a): the native ladder entries on i32_to_native(P)
    d_native = pk.from_planar_i32(torch.from_numpy(clean).cuda())
    o_dst, o_sizes = pk.compress_batch(d_native, d_dst=torch.full((NBLOCKS, stride), 0xC3, dtype=torch.uint8, device="cuda"), ladder=ladder, choice=d_choice)
    o_out, o_used = pk.decompress_batch(o_dst, NBLOCKS, stride, d_out=torch.full((NBLOCKS, pk.block_bytes), 0x77, dtype=torch.uint8, device="cuda"),
                                        ladder=ladder, choice=d_choice)
    o_planar = pk.to_planar_i32(o_out)
    torch.cuda.synchronize()
    o_dst, o_sizes, o_used, o_planar = o_dst.cpu().numpy(), o_sizes.cpu().numpy().view(np.uint64), o_used.cpu().numpy().view(np.uint64), o_planar.cpu().numpy()
    assert all(int(o_sizes[b]) == BIT63 for b in (1, 3)) and all(0 < int(o_sizes[b]) < BIT63 for b in served)

    # compress identity: streams, sizes, exact bit 63, nothing written for a refused block
    d_dst, d_sizes = pk.compress_planar_batch(src, d_dst=torch.full((NBLOCKS, stride), 0xC3, dtype=torch.uint8, device="cuda"), ladder=ladder, choice=d_choice)
    torch.cuda.synchronize()
    dst, sizes = d_dst.cpu().numpy(), d_sizes.cpu().numpy().view(np.uint64)
    assert np.array_equal(sizes, o_sizes), (IDS[i], tag, [hex(int(x)) for x in sizes])
    for b in range(NBLOCKS):
        if b in served:
            n = int(o_sizes[b])
            assert np.array_equal(dst[b, :n], o_dst[b, :n]), (IDS[i], tag, b, "stream")
        else:
            assert int(sizes[b]) == BIT63 and (dst[b] == 0xC3).all(), (IDS[i], tag, b, "nothing is written")
    assert np.array_equal(src.cpu().numpy(), P) and df.guards_untouched(sraw, off, P.size * 4), (IDS[i], tag, "d_planar is only read")

    # decompress identity, into a matrix of 0x77 between guards
    draw, out = df.guarded_matrix(P, off, fill=0x77)
    d_out, d_used = pk.decompress_planar_batch(d_dst, NBLOCKS, stride, d_out=out, ladder=ladder, choice=d_choice)
    torch.cuda.synchronize()
    assert d_out is out
    got, used = out.cpu().numpy(), d_used.cpu().numpy().view(np.uint64)
    assert np.array_equal(used, o_used), (IDS[i], tag, [hex(int(x)) for x in used])
    for b in range(NBLOCKS):
        if b in served:
            assert np.array_equal(got[b], o_planar[b]), (IDS[i], tag, b, "decoded")
            assert int(used[b]) == int(sizes[b])
        else:
            assert int(used[b]) & BIT63, (IDS[i], tag, b)
            assert (got[b].view(np.uint8) == 0x77).all(), (IDS[i], tag, b, "a refused block's rows are written")
    assert df.guards_untouched(draw, off, P.size * 4), (IDS[i], tag, "destination guards")

    # the handle's quantiser and its plain planar streams are what they were
    assert pk.quantizer() == own
    plain_after, sizes_after = [t.cpu().numpy() for t in pk.compress_planar_batch(src)]
    assert np.array_equal(sizes_after, plain_sizes)
    for b in range(NBLOCKS):
        assert np.array_equal(plain_after[b, : int(plain_sizes[b])], plain_before[b, : int(plain_sizes[b])]), (IDS[i], tag, b)
    assert api.lib().rspt_hip_last_hip_error(pk._h) == 0
    pk.close()


def test_refusals(api):
    import torch

    L = api.lib()
    d_choice = torch.zeros(4, dtype=torch.int32, device="cuda")

    def both(pk, ladder, planar_off=0, choice_off=0):
        """the status of the two entries; nothing may be launched, so every buffer stays as it was"""
        lad = np.ascontiguousarray(ladder, dtype=np.float64)
        lp = lad.ctypes.data_as(C.POINTER(C.c_double)) if lad.size else None
        n = pk.nch * pk.ns
        d_planar = torch.full((2 * n + 4,), 0x55555555, dtype=torch.int32, device="cuda")
        d_dst = torch.full((2, 4096), 0x77, dtype=torch.uint8, device="cuda")
        d_sizes = torch.full((2,), -1, dtype=torch.int64, device="cuda")
        pp, cp = d_planar.data_ptr() + planar_off, d_choice.data_ptr() + choice_off
        rc = (L.rspt_hip_compress_planar_batch_ladder_dev(pk._h, pp, 2, lp, lad.size, cp, d_dst.data_ptr(), 4096, d_sizes.data_ptr(), None),
              L.rspt_hip_decompress_planar_batch_ladder_dev(pk._h, d_dst.data_ptr(), 4096, 2, lp, lad.size, cp, pp, d_sizes.data_ptr(), None))
        torch.cuda.synchronize()
        assert (d_dst == 0x77).all() and (d_sizes == -1).all() and (d_planar == 0x55555555).all() and (d_choice == 0).all()
        return rc

    had = _new(api, "hadamard", 4, 3, 8, 3)
    assert both(had, []) == (ERR_ARG, ERR_ARG)
    assert both(had, [1.0] * 9) == (ERR_ARG, ERR_ARG)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-320):  # what rspt_hip_set_quantizer refuses
        assert both(had, [1.0, bad]) == (ERR_ARG, ERR_ARG), bad
    for off in (1, 2, 3):
        assert both(had, [1.0], planar_off=off) == (ERR_ARG, ERR_ARG), off  # a matrix off its 4-byte alignment
    assert both(had, [1.0], choice_off=2) == (ERR_ARG, ERR_ARG)
    had.close()
    natural = api.new_dct(4, 1, 16384)  # beyond the dense table: the FFT kernels
    forced = api.SignalPacker(api.KIND_DCT | api.DCT_FORCE_FFT, 4, 2, 64, 2)
    for pk in (natural, forced, api.new_hzr(4, 3, 8), api.new_xdelta_hzr(4, 3, 8, 2), api.new_bytes(64)):
        assert both(pk, [128.0]) == (ERR_UNSUPPORTED, ERR_UNSUPPORTED), pk.kind
        pk.close()
    dense = api.new_dct(4, 3, 100)
    assert both(dense, [128.0, 0.0]) == (ERR_ARG, ERR_ARG)
    dense.close()
