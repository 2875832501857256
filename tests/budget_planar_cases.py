"""The matrices of the planar byte-budget tests (rspt_hip_compress_budget_planar_batch_dev): for every shape of
tests/budget_cases.py, and for two narrow batched shapes more, the planar int32 matrix of its native batch,
P = native_to_i32(budget_cases.batch_native(shape, 5)); for the shapes below four bytes a sample a second variant whose bytes above
the sample width hold seeded garbage, which the planar entry must cut away; the base offsets every matrix is run from -- a 16-byte
boundary and 4 bytes past one, the alignment the entry promises to need; and the matrices of budget_cases.rule_cases().

The two shapes more: 24-bit samples (the cut of one byte) on rows of 4096 points, and 16-bit ones on rows of 2048 -- probe launches
of 512 and of 256 threads, where budget_cases' own batched shapes give 64, 128 and 1024 (nt = max(64, min(1024, ns / 8))).

The oracles of those tests never involve the code under test: (a) the native entry on i32_to_native(P), which
tests/test_gpu_budget.py holds to the composed oracle, and (b) the restated choices, budget_cases.restated.
tests/test_budget_planar_cases.py holds this file to what it promises, on the CPU."""
import functools

import numpy as np

import budget_cases as bc
import lossy_quantizer_cases as lq
from target_planar_cases import cut  # noqa: F401  (every value's low bps bytes, sign-extended)

EXTRA_SHAPES = [("hadamard", 3, 2, 4096, 3), ("hadamard", 2, 3, 2048, 2)]
SHAPES = list(bc.SHAPES) + EXTRA_SHAPES
NBLOCKS = 5
OFFSETS = (0, 4)  # bytes past a 16-byte boundary


def probe_threads(shape):
    """the workgroup size of the batched route's probe for this shape (host_rate.hip: probe_launch)"""
    return max(64, min(1024, shape[3] // 8))


def to_matrix(natives, shape):
    """native blocks [nblocks][block_bytes] -> int32 [nblocks][nch][ns]"""
    kind, bps, nch, ns, nb = shape
    return np.stack([lq.native_to_i32(n, bps, nch, ns) for n in natives]).astype(np.int32)


def with_garbage(P, bps, seed):
    """P with seeded garbage above the sample width, at least one element of every row changed (target_planar_cases._matrix)"""
    assert bps < 4
    bits, top = 8 * bps, 32 - 8 * bps
    u = np.ascontiguousarray(P).view(np.uint32)
    own = u >> np.uint32(bits)  # the sign extension
    hi = np.random.default_rng(seed).integers(0, 1 << top, size=u.shape, dtype=np.uint64).astype(np.uint32)
    hi[..., 0] = own[..., 0] ^ np.uint32(1)  # (at least one element of every row differs whatever the draw)
    return ((u & np.uint32((1 << bits) - 1)) | (hi << np.uint32(bits))).view(np.int32)


@functools.lru_cache(maxsize=None)
def _matrix(shape, garbage):
    P = to_matrix(bc.batch_native(shape, NBLOCKS), shape)
    if garbage:
        P = with_garbage(P, shape[1], 88000 + SHAPES.index(shape))
    P.setflags(write=False)
    return P


def matrix(shape, garbage=False):
    """int32 [NBLOCKS][nch][ns] of a shape, read-only and computed once per process"""
    return _matrix(tuple(shape), bool(garbage))


def variants(shape):
    """[(tag, garbage)]: the clean matrix, and for a shape of bps < 4 the one with garbage above the sample width"""
    return [("clean", False)] + ([("garbage", True)] if shape[1] < 4 else [])


@functools.lru_cache(maxsize=None)
def _rule_matrix(name):
    c = next(c for c in bc.rule_cases() if c["name"] == name)
    P = to_matrix(bc.restated(c)[0], c["shape"])
    P.setflags(write=False)
    return P


def rule_matrix(c):
    """int32 [nblocks][nch][ns] of a rule case: the blocks of budget_cases.restated(c)[0]"""
    return _rule_matrix(c["name"])
