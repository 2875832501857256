"""tests/budget_planar_cases.py held to what it promises, without a GPU: the garbage above the sample width is there in every row
and cuts back to the clean matrix, the clean matrix is the native batch, the shapes that take the batched route and the probe
launches they give are the ones the GPU tests lean on, and the rule cases' matrices are their restated blocks."""
import numpy as np

import budget_cases as bc
import budget_planar_cases as bp
import lossy_quantizer_cases as lq


def test_the_shapes_are_budget_cases_and_two_narrow_batched_ones():
    assert bp.SHAPES[: len(bc.SHAPES)] == list(bc.SHAPES)
    assert bp.EXTRA_SHAPES == [("hadamard", 3, 2, 4096, 3), ("hadamard", 2, 3, 2048, 2)]
    assert len(set(bp.SHAPES)) == len(bp.SHAPES) and bp.OFFSETS == (0, 4)
    assert {s[1] for s in bp.SHAPES if s[1] < 4 and bc.batched(s)} == {1, 2, 3}  # every cut runs through the probe


def test_which_shapes_are_batched_and_the_probe_launches_they_give():
    assert [bc.batched(s) for s in bp.SHAPES] == [True] * 5 + [False] * 3 + [False] * 3 + [True] * 2
    assert all(bc.batched(s, bp.NBLOCKS, len(bc.ladder_of(s[0]))) == bc.batched(s) for s in bp.SHAPES)
    assert {bp.probe_threads(s) for s in bp.SHAPES if bc.batched(s)} == {64, 128, 256, 512, 1024}
    assert [bp.probe_threads(s) for s in bp.EXTRA_SHAPES] == [512, 256]
    assert all(bp.probe_threads(s) * 8 >= s[3] for s in bp.SHAPES if bc.batched(s))


def test_the_garbage_is_in_every_row_and_cuts_back_to_the_clean_matrix():
    narrow = [s for s in bp.SHAPES if s[1] < 4]
    assert len(narrow) >= 5 and all(bp.variants(s) == [("clean", False), ("garbage", True)] for s in narrow)
    assert all(bp.variants(s) == [("clean", False)] for s in bp.SHAPES if s[1] == 4)
    for s in narrow:
        kind, bps, nch, ns, nb = s
        clean, dirty = bp.matrix(s), bp.matrix(s, garbage=True)
        assert clean.shape == dirty.shape == (bp.NBLOCKS, nch, ns) and clean.dtype == dirty.dtype == np.int32
        assert (clean != dirty).any(axis=2).all(), s  # at least one element of every row
        assert np.array_equal(bp.cut(dirty, bps), clean), s
        assert np.array_equal(bp.cut(clean, bps), clean), s
        # most of the garbage is no sign extension: a matrix that only repeated the sign would test nothing
        assert (clean != dirty).mean() > 0.9, s


def test_the_clean_matrix_is_the_native_batch():
    for s in bp.SHAPES:
        P, natives = bp.matrix(s), bc.batch_native(s, bp.NBLOCKS)
        assert P.shape == (bp.NBLOCKS, s[2], s[3])
        for i in range(bp.NBLOCKS):
            assert np.array_equal(lq.i32_to_native(P[i], s[1]), natives[i]), (s, i)
        for tag, garbage in bp.variants(s):
            assert not bp.matrix(s, garbage).flags.writeable


def test_the_rule_matrices_are_the_restated_blocks():
    for c in bc.rule_cases():
        natives = bc.restated(c)[0]
        P = bp.rule_matrix(c)
        kind, bps, nch, ns, nb = c["shape"]
        assert P.shape == (c["nblocks"], nch, ns) and P.dtype == np.int32 and not P.flags.writeable
        for i in range(c["nblocks"]):
            assert np.array_equal(lq.i32_to_native(P[i], bps), natives[i]), (c["name"], i)
