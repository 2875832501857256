"""The matrices of the planar byte-total tests (rspt_hip_compress_total_planar_batch_dev): for each shape below the planar int32
matrix of its native batch, P = native_to_i32(budget_cases.batch_native(shape, 5)); for the shapes below four bytes a sample a second
variant whose bytes above the sample width hold seeded garbage, which the planar entry must cut away -- for the sizes and for the
original its figures are taken against; and the base offsets every matrix is run from -- a 16-byte boundary and 4 bytes past one,
the alignment the entry promises to need.

The shapes are the smallest that tell the code paths apart: every sample width through the fused probe's cut, its launches of 64,
128, 512 and 1024 threads (nt = max(64, min(1024, ns / 8))), and on the general route a shape of bps 4 (no orig in the work area),
one of bps < 4 (orig by k_planar_ingest) and the dense dct.

The oracles of those tests never involve the code under test: (a) the native entry on i32_to_native(P), which
tests/test_gpu_total.py holds to the composed oracle, and (b) total_cases.choose_total_np on the composed oracle's tables.
tests/test_total_planar_cases.py holds this file to what it promises, on the CPU."""
import functools

import budget_cases as bc
from budget_planar_cases import to_matrix, with_garbage  # noqa: F401
from target_planar_cases import cut  # noqa: F401  (every value's low bps bytes, sign-extended)

# (kind, bps, nch, ns, nb) -> why it is here
WHY = {
    ("hadamard", 4, 1, 2, 1): "smallest fused row",
    ("hadamard", 1, 3, 8, 2): "smallest fused row, 8-bit samples",
    ("hadamard", 2, 5, 1024, 3): "16-bit samples, 128-thread probe",
    ("hadamard", 3, 2, 4096, 3): "24-bit cut, 512 threads",
    ("hadamard", 4, 9, 8192, 3): "longest fused row, ragged last hzr block, 1024 threads",
    ("hadamard", 4, 2, 16384, 3): "general route only, bps 4, no orig",
    ("hadamard", 2, 2, 16384, 3): "general only, bps < 4, orig by ingest",
    ("dct", 3, 3, 100, 2): "dense dct, general",
}
SHAPES = list(WHY)
FUSED = dict(zip(SHAPES, [True] * 5 + [False] * 3))  # the route the host picks for 5 blocks of the shape and its ladder
NBLOCKS = 5
OFFSETS = (0, 4)  # bytes past a 16-byte boundary
FUSED_MAX_NS, FUSED_MAX_N, MAX_SLOTS = 8192, 1 << 22, 65535


def fused(shape, nblocks=1, nladder=1):
    """the fused route runs this call (host_total.hip: total_fused_ok)"""
    return shape[0] == "hadamard" and shape[3] <= FUSED_MAX_NS and shape[2] * shape[3] < FUSED_MAX_N and nblocks * nladder <= MAX_SLOTS


def probe_threads(shape):
    """the workgroup size of the fused route's probe for this shape (host_total.hip)"""
    return max(64, min(1024, shape[3] // 8))


@functools.lru_cache(maxsize=None)
def _matrix(shape, garbage):
    P = to_matrix(bc.batch_native(shape, NBLOCKS), shape)
    if garbage:
        P = with_garbage(P, shape[1], 99000 + SHAPES.index(shape))
    P.setflags(write=False)
    return P


def matrix(shape, garbage=False):
    """int32 [NBLOCKS][nch][ns] of a shape, read-only and computed once per process"""
    return _matrix(tuple(shape), bool(garbage))


def variants(shape):
    """[(tag, garbage)]: the clean matrix, and for a shape of bps < 4 the one with garbage above the sample width"""
    return [("clean", False)] + ([("garbage", True)] if shape[1] < 4 else [])
