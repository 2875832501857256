"""tests/total_planar_cases.py held to what it promises, without a GPU: the garbage above the sample width is there in every row and
cuts back to the clean matrix, the clean matrix is the native batch, and the shapes take the routes and give the probe launches the
GPU tests lean on -- the route as tests/test_gpu_total.py states it."""
import numpy as np

import budget_cases as bc
import lossy_quantizer_cases as lq
import test_gpu_total as tg
import total_planar_cases as tp


def test_the_shapes():
    assert tp.SHAPES == [("hadamard", 4, 1, 2, 1), ("hadamard", 1, 3, 8, 2), ("hadamard", 2, 5, 1024, 3), ("hadamard", 3, 2, 4096, 3),
                         ("hadamard", 4, 9, 8192, 3), ("hadamard", 4, 2, 16384, 3), ("hadamard", 2, 2, 16384, 3), ("dct", 3, 3, 100, 2)]
    assert len(set(tp.SHAPES)) == len(tp.SHAPES) and tp.OFFSETS == (0, 4) and tp.NBLOCKS == 5


def test_which_shapes_are_fused_and_the_probe_launches_they_give():
    assert (tp.FUSED_MAX_NS, tp.FUSED_MAX_N, tp.MAX_SLOTS) == (tg.FUSED_MAX_NS, tg.FUSED_MAX_N, tg.MAX_SLOTS)
    for s in tp.SHAPES:
        K = len(bc.ladder_of(s[0]))
        assert tp.FUSED[s] == tg.fused(s) == tg.fused(s, tp.NBLOCKS, K) == tp.fused(s) == tp.fused(s, tp.NBLOCKS, K), s
    for args in ((tg.TINY, 8192, 8), (tg.TINY, 8192, 7), (tg.TINY, 13107, 5), (("hadamard", 4, 512, 8192, 3), 1, 1), (("hadamard", 4, 511, 8192, 3), 1, 1)):
        assert tp.fused(*args) == tg.fused(*args), args
    assert [tp.FUSED[s] for s in tp.SHAPES] == [True] * 5 + [False] * 3
    assert {tp.probe_threads(s) for s in tp.SHAPES if tp.FUSED[s]} == {64, 128, 512, 1024}
    assert all(tp.probe_threads(s) * 8 >= s[3] for s in tp.SHAPES if tp.FUSED[s])
    # every cut runs through the fused probe, and the general route sees a shape with an orig of its own and one without
    assert {s[1] for s in tp.SHAPES if tp.FUSED[s]} == {1, 2, 3, 4}
    assert {s[1] < 4 for s in tp.SHAPES if s[0] == "hadamard" and not tp.FUSED[s]} == {True, False}


def test_the_garbage_is_in_every_row_and_cuts_back_to_the_clean_matrix():
    narrow = [s for s in tp.SHAPES if s[1] < 4]
    assert len(narrow) == 5 and all(tp.variants(s) == [("clean", False), ("garbage", True)] for s in narrow)
    assert all(tp.variants(s) == [("clean", False)] for s in tp.SHAPES if s[1] == 4)
    for s in narrow:
        kind, bps, nch, ns, nb = s
        clean, dirty = tp.matrix(s), tp.matrix(s, garbage=True)
        assert clean.shape == dirty.shape == (tp.NBLOCKS, nch, ns) and clean.dtype == dirty.dtype == np.int32
        assert (clean != dirty).any(axis=2).all(), s  # at least one element of every row
        assert np.array_equal(tp.cut(dirty, bps), clean), s
        assert np.array_equal(tp.cut(clean, bps), clean), s
        # most of the garbage is no sign extension: a matrix that only repeated the sign would test nothing
        assert (clean != dirty).mean() > 0.9, s


def test_the_clean_matrix_is_the_native_batch():
    for s in tp.SHAPES:
        P, natives = tp.matrix(s), bc.batch_native(s, tp.NBLOCKS)
        assert P.shape == (tp.NBLOCKS, s[2], s[3])
        assert np.array_equal(P, tp.to_matrix(natives, s))
        for i in range(tp.NBLOCKS):
            assert np.array_equal(lq.i32_to_native(P[i], s[1]), natives[i]), (s, i)
        for tag, garbage in tp.variants(s):
            assert not tp.matrix(s, garbage).flags.writeable
