"""The adjustable quantiser of the lossy packers without a GPU: the record of the reference rebuilt with other constants
(tests/golden/lossy_quantizer_record.json) against its generator's inputs, against the existing golden entries at the default
constants, and against the numpy restatement of both quantisers (tests/lossy_quantizer_cases.py); and the new entry points'
signatures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import devframe as df
import lossy_quantizer_cases as lq
from devframe import ROOT


@pytest.fixture(scope="module")
def record():
    r = df.golden("lossy_quantizer_record.json")
    return {e["name"]: e for e in r["cases"]}, {e["name"]: e for e in r["defaults"]}


def test_the_record_holds_every_case_and_its_inputs(record):
    rec, _ = record
    want = lq.all_cases()
    assert sorted(rec) == sorted(c["name"] for c in want)
    for c in want:
        e = rec[c["name"]]
        assert [e[k] for k in ("kind", "bps", "nch", "ns", "nb")] == [c[k] for k in ("kind", "bps", "nch", "ns", "nb")]
        assert float.fromhex(e["q_hex"]) == c["q"] and len(e["blocks"]) == c["nblocks"]
        if c["nch"] * c["ns"] <= 1 << 17:  # (the inputs of the long rows are checked where they are used, on the GPU)
            for i, b in enumerate(e["blocks"]):
                assert lq.crc(lq.block_data(c, i)) == b["in_crc32"], (c["name"], i)
    # every plane count, on both packers, with and without cutting; quality below and above the reference's on both
    for kind in ("dct", "hadamard"):
        assert {c["nb"] for c in want if c["kind"] == kind} == {1, 2, 3, 4}
        q0 = lq.DEFAULTS[kind][0]
        assert any(c["q"] < q0 for c in want if c["kind"] == kind) and any(c["q"] > q0 for c in want if c["kind"] == kind)


def test_the_patched_build_reproduces_the_golden_entries_at_the_default_constants(record, golden):
    _, defaults = record
    assert sorted(defaults) == sorted(lq.default_cases())
    for name, d in defaults.items():
        g = golden["packers"][name]
        assert (d["size"], d["crc32"], d["decoded_crc32"]) == (g["size"], g["crc32"], g["decoded_crc32"]), name


def _small(c):
    return c["full"] and c["fft"] is None and c["ns"] <= 1024


def test_the_restatement_is_the_reference_on_the_small_cases(record, orc):
    """Both directions of both quantisers: the values the restatement stores (cut to nb bytes where the stream cuts them) against
    the record's streams, and its decode of those values against the record's decoded blocks."""
    rec, _ = record
    n = 0
    for c in lq.all_cases():
        if not _small(c):
            continue
        for i, b in enumerate(rec[c["name"]]["blocks"]):
            data = lq.block_data(c, i)
            stream = lq.unpack(b["stream"])
            got, means, used = lq.stream_values(orc, stream, c["kind"], c["nch"], c["ns"], c["nb"])
            assert used == len(stream)
            want, m32 = lq.restated_stored(c, data)
            stored = lq.cut_to_nb(lq.xdelta_forward(got.reshape(-1)) if c["kind"] == "dct" else got.reshape(-1), c["nb"])
            assert (stored == want).all(), (c["name"], i)
            assert (means == ((m32.astype(np.int64) << 8).astype(np.int32) >> 8)).all(), (c["name"], i)  # the header keeps 24 bits
            assert lq.restated_decode(c, got, means).tobytes() == lq.unpack(b["decoded"]), (c["name"], i)
            n += 1
    assert n >= 50  # (every case of at most 256 bytes, and the four of lossy_quantizer_cases.FULL_TOO)


@pytest.mark.parametrize("name", [c["name"] for c in lq.hadamard_restated_cases()])
def test_the_restatement_is_the_oracle_on_the_long_rows(orc, name):
    """The cases that are held to the restatement alone (2^19, 2^20, 2^21 points): at the reference's own constants the
    restatement stores what the oracle's packer stores, whose stream tests/test_oracle_golden.py holds to the real reference at
    these very inputs -- so the numpy transform and the means are right at these row lengths."""
    c = {c["name"]: c for c in lq.hadamard_restated_cases()}[name]
    q0, nb0 = lq.DEFAULTS["hadamard"]
    data = lq.block_data(c, 0)
    pk = orc.packer("hadamard", c["bps"], c["nch"], c["ns"], nb0)
    stream = pk.compress(data)
    got, means, used = lq.stream_values(orc, stream, "hadamard", c["nch"], c["ns"], nb0)
    assert used == len(stream)
    want, m32 = lq.restated_stored(dict(c, q=q0, nb=nb0), data)
    assert (got.reshape(-1) == want).all() and (means == ((m32.astype(np.int64) << 8).astype(np.int32) >> 8)).all()
    dec, used, rc = pk.decompress(stream)
    assert rc == 0 and lq.restated_decode(dict(c, q=q0, nb=nb0), got, means).tobytes() == dec
    pk.close()
    # and at the case's own setting the restatement keeps something: the quantised transform is not all zero
    stored, _ = lq.restated_stored(c, data)
    assert (stored != 0).mean() > 0.001


def test_an_out_of_range_quotient_is_in_the_record(record, orc):
    """the case that exists for the x86 truncation value really produces it: at quality 2n the quotient is twice the wrapped
    transform, and what leaves int32 is stored as 0x80000000 (nb = 4 keeps it whole)"""
    rec, _ = record
    c = {c["name"]: c for c in lq.all_cases()}["had_2x64_full_scale_q2n_nb4"]
    hit = 0
    for b in rec[c["name"]]["blocks"]:
        got, _, _ = lq.stream_values(orc, lq.unpack(b["stream"]), "hadamard", c["nch"], c["ns"], c["nb"])
        hit += int((got == -(1 << 31)).sum())
    assert hit > 0


def test_the_fft_cases_stay_inside_the_gates_on_the_cpu(record):
    """a numpy fp64 FFT DCT against the record (measured by the generator): |diff| <= 1 and a share of differing coefficients
    inside the gate of tests/test_gpu_dct_fft.py, so that the GPU test of these cases tests the kernels and not the inputs"""
    rec, _ = record
    fft = [c for c in lq.all_cases() if c["fft"]]
    assert {c["fft"] for c in fft} == {"forced", "natural"}
    for c in fft:
        e = rec[c["name"]]
        assert e["fft_maxdiff"] <= lq.FFT_MAX_DIFF and max(e["fft_share"]) <= lq.FFT_MAX_SHARE / 2, (c["name"], e["fft_share"], e["fft_maxdiff"])


def test_the_quantizer_entry_points_have_the_stated_signatures():
    from rspt_amd import api

    L = api.lib()
    assert api.C_ABI["rspt_hip_set_quantizer"] == (C.c_int, [C.c_void_p, C.c_double, C.c_uint])
    restype, argtypes = api.C_ABI["rspt_hip_get_quantizer"]
    assert restype is C.c_int and len(argtypes) == 3 and argtypes[0] is C.c_void_p and argtypes[1] is C.POINTER(C.c_double)
    assert api.CXX_SHIM["rspt_cxx_set_quantizer"] == (C.c_int, [C.c_void_p, C.c_double, C.c_uint])
    for name in ("rspt_hip_set_quantizer", "rspt_hip_get_quantizer", "rspt_cxx_set_quantizer"):
        assert hasattr(L, name), name
    head = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "rspt_hip.h")).read(), flags=re.S)
    head = " ".join(head.split())
    assert "int rspt_hip_set_quantizer(rspt_hip_packer* p, double quality, unsigned nb);" in head
    assert "int rspt_hip_get_quantizer(const rspt_hip_packer* p, double* quality, unsigned* nb);" in head
    cxx = " ".join(re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "signal_packer.h")).read(), flags=re.S).split())
    assert 'extern "C" int rspt_cxx_set_quantizer(i_signal_packer* instance, double quality, unsigned nb);' in cxx
    exported = df.exported()
    for name in ("rspt_hip_set_quantizer", "rspt_hip_get_quantizer", "rspt_cxx_set_quantizer"):
        assert re.search(r"\bT %s\b" % name, exported), name  # C linkage: the plain name


def test_a_null_handle_is_refused():
    from rspt_amd import api

    L = api.lib()
    q, nb = C.c_double(), C.c_uint()
    assert L.rspt_hip_set_quantizer(None, 1.0, 3) == -1
    assert L.rspt_hip_get_quantizer(None, C.byref(q), C.cast(C.byref(nb), C.c_void_p)) == -1
    assert L.rspt_cxx_set_quantizer(None, 1.0, 3) == -1
