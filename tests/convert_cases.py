"""The native <-> int32 converter stages and the wide packers: test inputs, a numpy model of the reference's
two functions, and the entries of tests/golden/convert_record.json.

convert_native_to_i32 (utils.cpp:123-191) reads every sample of the interleaved block sign-extended from bps bytes into a
[nch][ns] int32 matrix; convert_i32_to_native (utils.cpp:51-121) writes the low bps bytes of every value back.  With
reverse_byte_order a sample's bytes are most significant first.  One-byte samples have no byte order: the reference's
reversed one-byte STORE writes at native + 1 (utils.cpp:115), one byte past the buffer, and is left out everywhere.

The record is made by tests/golden/make_convert_record.py from the compiled reference; record_cases(backend) is the one
function that makes its entries, so that a test can make them again from oracle/_ref and compare.
"""
import numpy as np

import cases
from casetools import record_text

FNV_OFFSET, FNV_PRIME = 0x811C9DC5, 0x01000193


def fnv1a(buf):
    """32-bit FNV-1a of a buffer, as golden.json has it (plain Python: small buffers only -- see hash_of)"""
    h = FNV_OFFSET
    for b in bytes(buf):
        h = ((h ^ b) * FNV_PRIME) & 0xFFFFFFFF
    return h


def native_to_i32(native, bps, nch, ns, be=False):
    """model of convert_native_to_i32: native bytes -> [nch][ns] int32"""
    a = np.ascontiguousarray(native, dtype=np.uint8).reshape(ns, nch, bps)
    if be and bps > 1:
        a = a[:, :, ::-1]
    u = np.zeros((ns, nch), dtype=np.uint32)
    for k in range(bps):
        u |= a[:, :, k].astype(np.uint32) << np.uint32(8 * k)
    sh = np.uint32(32 - 8 * bps)
    return np.ascontiguousarray(((u << sh).view(np.int32) >> np.int32(32 - 8 * bps)).T)


def i32_to_native(planar, bps, be=False):
    """model of convert_i32_to_native: [nch][ns] int32 -> native bytes (flat uint8)"""
    u = np.ascontiguousarray(np.asarray(planar, dtype=np.int32).T).view(np.uint32)
    b = np.stack([((u >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.uint8) for k in range(bps)], axis=-1)
    if be and bps > 1:
        b = b[:, :, ::-1]
    return np.ascontiguousarray(b).reshape(-1)


def sign_extend(planar, bps):
    sh = np.int32(32 - 8 * bps)
    return (np.asarray(planar, dtype=np.int32) << sh) >> sh


# ---- converter cases of the record --------------------------------------------------------------------------------------
SMALL_SHAPES = [(1, 1), (1, 9), (3, 17), (12, 64), (5, 63), (64, 65), (70, 3)]  # nch, ns
LARGE_SHAPES = [(1000, 257, 2), (8193, 65, 3), (20000, 17, 1), (65535, 5, 4)]  # nch, ns, bps: hashes only


def native_input(nch, ns, bps, seed):
    """every byte value: negative samples at every width"""
    return cases.hash_bytes(nch * ns * bps, seed)


def planar_input(nch, ns, seed):
    """full-range int32: the high bytes must be dropped"""
    return cases.hash_i32(nch * ns, seed, (1 << 31) - 1).astype(np.int32).reshape(nch, ns)


def converter_cases():
    """name, dir ('n2i' | 'i2n'), bps, nch, ns, be, store ('full' | 'hash')"""
    C = []
    for nch, ns in SMALL_SHAPES:
        for bps in (1, 2, 3, 4):
            for be in (0, 1):
                store = "full" if nch * ns <= 64 else "hash"
                C.append(dict(name="n2i_%dx%d_i%d_%s" % (nch, ns, 8 * bps, "be" if be else "le"), dir="n2i", bps=bps, nch=nch, ns=ns, be=be, store=store))
                if not (bps == 1 and be):  # (the reference's one-byte reversed store is out of bounds)
                    C.append(dict(name="i2n_%dx%d_i%d_%s" % (nch, ns, 8 * bps, "be" if be else "le"), dir="i2n", bps=bps, nch=nch, ns=ns, be=be, store=store))
    for nch, ns, bps in LARGE_SHAPES:
        for be in (0, 1):
            C.append(dict(name="n2i_%dx%d_i%d_%s" % (nch, ns, 8 * bps, "be" if be else "le"), dir="n2i", bps=bps, nch=nch, ns=ns, be=be, store="hash"))
            if not (bps == 1 and be):
                C.append(dict(name="i2n_%dx%d_i%d_%s" % (nch, ns, 8 * bps, "be" if be else "le"), dir="i2n", bps=bps, nch=nch, ns=ns, be=be, store="hash"))
    return C


def case_input(c):
    seed = 5000 + 7 * c["nch"] + 3 * c["ns"] + c["bps"]
    return native_input(c["nch"], c["ns"], c["bps"], seed) if c["dir"] == "n2i" else planar_input(c["nch"], c["ns"], seed)


def model_output(c, x):
    """the numpy model's answer as flat bytes"""
    if c["dir"] == "n2i":
        return native_to_i32(x, c["bps"], c["nch"], c["ns"], bool(c["be"])).view(np.uint8).reshape(-1)
    return i32_to_native(x, c["bps"], bool(c["be"]))


# ---- wide packer cases of the record ------------------------------------------------------------------------------------
WIDE_PACKER_CASES = [
    dict(name="wide_xdelta_hzr_8193x16_i32", kind="xdelta_hzr", bps=4, nch=8193, ns=16, nb=3),
    dict(name="wide_hzr_8193x16_i16", kind="hzr", bps=2, nch=8193, ns=16, nb=4),
    dict(name="wide_dct_8193x16_i24", kind="dct", bps=3, nch=8193, ns=16, nb=2),
    dict(name="wide_hadamard_8193x16_i32", kind="hadamard", bps=4, nch=8193, ns=16, nb=3),
    dict(name="wide_xdelta_hzr_65535x8_i32", kind="xdelta_hzr", bps=4, nch=65535, ns=8, nb=3),
]


def wide_block(bps, nch, ns, seed):
    """a block of slow random walks, kept inside the sample width (and small enough for the transforms' int32 arithmetic)"""
    amp = 40 if bps > 1 else 3
    return cases._rand_native(nch, ns, bps, seed, amp, walk=True)


def wide_packer_input(c):
    return wide_block(c["bps"], c["nch"], c["ns"], 6000 + c["nch"] % 97 + c["bps"])


def record_cases(backend, hash_of):
    """the record's entries.  backend: native_to_i32(native, ns, nch, bps, reverse) -> [nch][ns] int32,
    i32_to_native(planar, bps, reverse) -> bytes, pack(kind, bps, nch, ns, nb, data) -> bytes, all of the compiled reference;
    hash_of(bytes) -> 32-bit FNV-1a"""
    out = []
    for c in converter_cases():
        x = case_input(c)
        if c["dir"] == "n2i":
            y = np.ascontiguousarray(backend.native_to_i32(x, c["ns"], c["nch"], c["bps"], bool(c["be"]))).view(np.uint8).reshape(-1)
        else:
            y = np.frombuffer(backend.i32_to_native(x, c["bps"], bool(c["be"])), dtype=np.uint8)
        e = dict(c)
        e.update(size=int(y.size), fnv1a=int(hash_of(y)))
        if c["store"] == "full":
            e["hex"] = y.tobytes().hex()
        out.append(e)
    for c in WIDE_PACKER_CASES:
        s = backend.pack(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"], wide_packer_input(c))
        e = dict(c)
        e.update(dir="pack", size=len(s), fnv1a=int(hash_of(s)))
        out.append(e)
    return out


def dump_record(entries):
    """the record file's text (one case per line)"""
    return record_text({"generator": "tests/golden/make_convert_record.py (the reference's convert_native_to_i32 / convert_i32_to_native and packers + "
                                     "tests/golden/convert_shim.cpp, g++ -O2 -std=gnu++11)",
                        "fnv1a": "32-bit FNV-1a of the output bytes (int32 matrices as little-endian bytes, [nch][ns])", "cases": entries})
