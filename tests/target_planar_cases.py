"""The matrices of the planar ladder, target and container-choice tests (rspt_hip_compress_planar_batch_ladder_dev,
rspt_hip_compress_target_planar_batch_dev and their kin): for every case of tests/target_cases.py the planar int32 matrix of its
native blocks, P = native_to_i32(block_native(c, i)); for the cases below four bytes a sample a second variant whose bytes above
the sample width hold seeded garbage, which the planar entries must cut away; and the base offsets every matrix is run from --
a 16-byte boundary and 4 bytes past one, the alignment the entries promise to need.

The oracles of those tests never involve the code under test: (a) the native entries on i32_to_native(P), which
tests/test_gpu_ladder.py and tests/test_gpu_target.py hold to the composed oracle and the numpy restatement, and (b) the
restatement's choices, target_cases.restated.  tests/test_target_planar_cases.py holds this file to what it promises, on the CPU."""
import functools

import numpy as np

import lossy_quantizer_cases as lq
import target_cases as tc

NARROW = ("had_i16_5x1024_nb2", "had_i8_3x8_nb1_none", "dct_i24_2x257_nb3")  # the cases of bps < 4
OFFSETS = (0, 4)  # bytes past a 16-byte boundary


def case(name):
    return next(c for c in tc.all_cases() if c["name"] == name)


def cut(P, bps):
    """every value's low bps bytes, sign-extended: what convert_i32_to_native keeps and convert_native_to_i32 reads back"""
    sh = np.uint32(32 - 8 * bps)
    return ((np.ascontiguousarray(P).view(np.uint32) << sh).view(np.int32) >> sh).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _matrix(name, garbage):
    c = case(name)
    P = np.stack([lq.native_to_i32(tc.block_native(c, i), c["bps"], c["nch"], c["ns"]) for i in range(c["nblocks"])]).astype(np.int32)
    if garbage:
        assert c["bps"] < 4, name
        bits, top = 8 * c["bps"], 32 - 8 * c["bps"]
        u = P.view(np.uint32)
        own = u >> np.uint32(bits)  # the sign extension
        hi = np.random.default_rng(77000 + c["seed"]).integers(0, 1 << top, size=u.shape, dtype=np.uint64).astype(np.uint32)
        hi[..., 0] = own[..., 0] ^ np.uint32(1)  # (at least one element of every row differs whatever the draw)
        P = ((u & np.uint32((1 << bits) - 1)) | (hi << np.uint32(bits))).view(np.int32)
    P.setflags(write=False)
    return P


def matrix(c, garbage=False):
    """int32 [nblocks][nch][ns] of case c, read-only and computed once per process"""
    return _matrix(c["name"], bool(garbage))


def variants(c):
    """[(tag, garbage)]: the clean matrix, and for a narrow case the one with garbage above the sample width"""
    return [("clean", False)] + ([("garbage", True)] if c["name"] in NARROW else [])
