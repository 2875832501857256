"""tests/target_planar_cases.py held to what it promises, without a GPU: the garbage above the sample width is there in every row
and cuts back to the clean matrix; the restated choices the planar tests lean on (target_cases.restated) still cover what they
are there for; and the new entries are declared, exported and bound with the signatures of their native twins.

(The issue speaks of eight new prototypes; it names seven functions, which are the seven checked here.)"""
import re

import numpy as np

import devframe as df
import target_cases as tc
import target_planar_cases as tp


def test_the_narrow_cases_are_the_cases_below_four_bytes():
    assert sorted(tp.NARROW) == sorted(c["name"] for c in tc.all_cases() if c["bps"] < 4)
    assert {c["bps"] for c in tc.all_cases() if c["name"] in tp.NARROW} == {1, 2, 3}


def test_the_garbage_is_in_every_row_and_cuts_back_to_the_clean_matrix():
    for name in tp.NARROW:
        c = tp.case(name)
        clean, dirty = tp.matrix(c), tp.matrix(c, garbage=True)
        assert clean.shape == dirty.shape == (c["nblocks"], c["nch"], c["ns"]) and clean.dtype == dirty.dtype == np.int32
        assert (clean != dirty).any(axis=2).all(), name  # at least one element of every row
        assert np.array_equal(tp.cut(dirty, c["bps"]), clean), name
        assert np.array_equal(tp.cut(clean, c["bps"]), clean), name
        assert not np.array_equal(dirty, clean)
        # most of the garbage is no sign extension: a matrix that only repeated the sign would test nothing
        assert (clean != dirty).mean() > 0.9, name


def test_the_clean_matrix_is_the_native_block():
    import lossy_quantizer_cases as lq

    for c in tc.all_cases():
        if c["nch"] * c["ns"] > 1 << 16:
            continue
        P = tp.matrix(c)
        for i in range(c["nblocks"]):
            assert np.array_equal(lq.i32_to_native(P[i], c["bps"]), tc.block_native(c, i)), (c["name"], i)


def test_the_restated_choices_cover_what_the_planar_tests_lean_on():
    R = [(c, tc.restated(c)) for c in tc.all_cases()]
    assert len({k for c, blocks in R for figs, (k, p) in blocks}) >= 3
    assert [c["name"] for c, blocks in R for figs, (k, p) in blocks
            if k == len(figs) - 1 and not any(tc.meets(pp, m, path, c["target"]) for pp, m, path in figs)], "none meets it"
    assert [c["name"] for c, blocks in R for figs, pick in blocks for pp, m, path in figs if path == 1], "no candidate on path 1"


PLANAR_OF = {
    "rspt_hip_compress_planar_batch_ladder_dev": "rspt_hip_compress_batch_ladder_dev",
    "rspt_hip_decompress_planar_batch_ladder_dev": "rspt_hip_decompress_batch_ladder_dev",
    "rspt_hip_compress_target_planar_work_bytes": "rspt_hip_compress_target_work_bytes",
    "rspt_hip_compress_target_planar_batch_dev": "rspt_hip_compress_target_batch_dev",
    "rspt_hip_decompress_packed_planar_ladder_dev": "rspt_hip_decompress_packed_ladder_dev",
}
DECLARATIONS = [
    re.compile(r"int rspt_hip_compress_planar_batch_ladder_dev\(rspt_hip_packer\* p, const int32_t\* d_planar, size_t nblocks, const double\* ladder, "
               r"size_t nladder, const uint32_t\* d_choice, void\* d_dst, size_t dst_stride, uint64_t\* d_sizes, void\* stream\);"),
    re.compile(r"int rspt_hip_decompress_planar_batch_ladder_dev\(rspt_hip_packer\* p, const void\* d_src, size_t src_stride, size_t nblocks, "
               r"const double\* ladder, size_t nladder, const uint32_t\* d_choice, int32_t\* d_planar, uint64_t\* d_consumed, void\* stream\);"),
    "int rspt_hip_compress_target_planar_work_bytes(rspt_hip_packer* p, size_t nblocks, size_t nladder, size_t* bytes);",
    re.compile(r"int rspt_hip_compress_target_planar_batch_dev\(rspt_hip_packer\* p, const int32_t\* d_planar, size_t nblocks, const double\* ladder, "
               r"size_t nladder, double target_prdn, void\* d_dst, size_t dst_stride, uint64_t\* d_sizes, uint32_t\* d_choice, double\* d_prdn, "
               r"void\* d_work, void\* stream\);"),
    re.compile(r"int rspt_hip_pack_batch_choice_dev\(rspt_hip_packer\* p, const void\* d_dst, size_t dst_stride, const uint64_t\* d_sizes, size_t nblocks, "
               r"const uint32_t\* d_choice, size_t nladder, void\* d_packed, uint64_t\* d_total, void\* stream\);"),
    re.compile(r"int rspt_hip_decompress_packed_ladder_dev\(rspt_hip_packer\* p, const void\* d_packed, size_t packed_len, size_t nblocks, "
               r"const double\* ladder, size_t nladder, void\* d_dst, uint64_t\* d_consumed, void\* stream\);"),
    re.compile(r"int rspt_hip_decompress_packed_planar_ladder_dev\(rspt_hip_packer\* p, const void\* d_packed, size_t packed_len, size_t nblocks, "
               r"const double\* ladder, size_t nladder, int32_t\* d_planar, uint64_t\* d_consumed, void\* stream\);"),
]


def test_the_new_entries_are_declared_exported_and_bound():
    import ctypes as C

    from rspt_amd import api

    df.check_entries(DECLARATIONS, list(PLANAR_OF), native_of=PLANAR_OF,
                     methods=("compress_to_prdn_planar", "target_planar_work_bytes", "compress_planar_batch", "decompress_planar_batch", "pack_batch",
                              "decompress_packed", "decompress_packed_planar"))
    df.check_entries([], ["rspt_hip_pack_batch_choice_dev", "rspt_hip_decompress_packed_ladder_dev"])
    p, z, dp = C.c_void_p, C.c_size_t, C.POINTER(C.c_double)
    # the two without a native twin: pack_batch's row with (d_choice, nladder) behind nblocks, decompress_packed's with the ladder
    restype, a = api.C_ABI["rspt_hip_pack_batch_dev"]
    assert api.C_ABI["rspt_hip_pack_batch_choice_dev"] == (restype, a[:5] + [p, z] + a[5:])
    restype, a = api.C_ABI["rspt_hip_decompress_packed_dev"]
    assert api.C_ABI["rspt_hip_decompress_packed_ladder_dev"] == (restype, a[:4] + [dp, z] + a[4:])
