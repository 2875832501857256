"""Planar int32 in and out of the packers (rspt_hip_compress_planar_batch_dev / rspt_hip_decompress_planar_batch_dev; DESIGN.md
4i): the shapes, the inputs and the CPU side of every expectation of tests/test_planar_packers.py.

The contract is two identities: compress_planar(P) == compress(i32_to_native(P)) and decompress_planar(S) ==
native_to_i32(decompress(S)).  So every expected stream is the CPU oracle's stream of convert_cases.i32_to_native(P) -- the numpy
model the converters' record pins to the reference -- and every expected value the model's view of the oracle's decode.
"""
import numpy as np

import cases
import convert_cases as cc

LOSSLESS = ("xdelta_hzr", "hzr")

# (nch, ns): what each shape exercises in k_planar_stream and the decode routes
LOSSLESS_SHAPES = [
    (1, 1), (1, 2),                       # the halo at flat index 0 and 1
    (3, 17),                              # N < 64, ragged
    (12, 64),                             # a small, regular shape
    (5, 4099),                            # N % 16 != 0; partial last segment
    (3, 30000),                           # N = 90000 > one hzr block; channel boundaries inside segments
    (4, 16384),                           # exactly one hzr block per plane, fully aligned
    (4, 65536),                           # four hzr blocks per plane
    (4, 256), (12, 512), (64, 256),       # the native entry's row-scan decode shapes (CG = 16 / 64)
    (1100, 64),                           # a `wide` handle
    (8193, 16),                           # Tn_native == 0
]
HADAMARD_SHAPES = [(3, 16), (12, 1024), (2, 65536), (1, 131072)]  # k_fwht, k_fwht64k, the two-pass route
DCT_SHAPES = [(3, 17), (12, 64), (2, 4096), (1, 16384)]          # dense table (ragged, regular, large); the FFT route
BATCHES = (1, 3)  # (the second block of an odd N starts off a 16-byte boundary)


def seed_of(kind, bps, nch, ns, nblocks=1):
    return 9000 + 131 * ("dct", "hadamard", "hzr", "xdelta_hzr").index(kind) + 17 * bps + 7 * nch + 3 * ns + nblocks


def walk(nblocks, nch, ns, bps, seed):
    """[nblocks][nch][ns] int32: slow random walks along every channel inside +-2000 (one-byte samples: as far as they go), cut to
    the sample width -- compressible, an xdelta packer stays at the nb it was created with, and small enough for the transforms'
    int32 arithmetic"""
    step = cases.hash_i32(nblocks * nch * ns, seed, 40 if bps > 1 else 3).astype(np.int64).reshape(nblocks, nch, ns)
    x = np.cumsum(step, axis=2) % 4001 - 2000 if bps > 1 else np.cumsum(step, axis=2)
    return cc.sign_extend(x.astype(np.int32), bps)


def noise(nblocks, nch, ns, seed):
    """full-range int32: noise in every byte, values far outside the narrower sample widths"""
    return cases.hash_i32(nblocks * nch * ns, seed, (1 << 31) - 1).astype(np.int32).reshape(nblocks, nch, ns)


def quiet(nblocks, nch, ns, seed):
    """zeros with a small value every 977 elements: almost every 128-byte line of every plane stays zero"""
    x = np.zeros(nblocks * nch * ns, dtype=np.int32)
    x[seed % 977::977] = 5
    return x.reshape(nblocks, nch, ns)


def escalation_batch(nch, ns):
    """four blocks for an xdelta packer created with nb = 1: two ramps (one byte), one that needs three bytes, one that needs four"""
    n = nch * ns
    ramp = np.arange(n, dtype=np.int64)
    b2, b3 = ramp.copy(), ramp.copy()
    b2[n // 2] += 100000
    b3[n // 3] += 1 << 30
    return np.stack([ramp, ramp + 1, b2, b3]).astype(np.int32).reshape(4, nch, ns)


def oracle_streams(orc, kind, bps, nch, ns, nb, P, po=None):
    """the oracle's streams of the blocks of P in order on ONE packer instance (the nb escalation carries on), and its nb after
    each block.  po: an instance to go on with."""
    own = po is None
    po = po or orc.packer(kind, bps, nch, ns, nb)
    streams, nbs = [], []
    for blk in P:
        streams.append(po.compress(cc.i32_to_native(blk, bps, False)))
        nbs.append(orc.packer_nb(po) if kind == "xdelta_hzr" else None)
    if own:
        po.close()
    return streams, nbs


def oracle_decode(orc, kind, bps, nch, ns, nbs, streams):
    """the model's planar view of the oracle's decode of each stream; nbs[i]: the plane count of stream i (the reference keeps it
    out of the stream: an xdelta stream is decoded by an instance in that state), one number where it is the same for all"""
    one = None if isinstance(nbs, (list, tuple)) else orc.packer(kind, bps, nch, ns, nbs)
    out = []
    for i, s in enumerate(streams):
        po = one or orc.packer(kind, bps, nch, ns, nbs[i])
        dec, used, rc = po.decompress(s)
        assert rc == 0 and used == len(s)
        out.append(cc.native_to_i32(np.frombuffer(dec, dtype=np.uint8), bps, nch, ns, False))
        if one is None:
            po.close()
    if one is not None:
        one.close()
    return np.stack(out)
