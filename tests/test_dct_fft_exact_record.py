"""The exact-value rule for the dct's FFT kernels without a GPU: the inputs keep out of the comparator's band (the record of
tests/golden/make_dct_fft_exact_record.py), the fp64 restatement that every other dct test leans on (oracle.dct_big_*) passes
the rule itself, and the comparator rejects a single coefficient moved by one count."""

import numpy as np
import pytest

import dct_fft_cases as dc
import devframe as df

SMALL = [c["name"] for c in dc.all_cases() if c["k"] <= 16]


@pytest.fixture(scope="module")
def record():
    r = df.golden("dct_fft_exact_record.json")
    assert r["cap"] == dc.CAP
    return {e["name"]: e for e in r["cases"]}


def test_the_sweep_takes_every_decomposition():
    ks = {c["k"] for c in dc.sweep_cases() if c["src"] == "noise" and c["bps"] == 4}
    assert ks == set(range(4, 23))
    by = dc.by_name()
    for k in range(4, 23):
        c = by["noise_k%02d" % k]
        assert c["forced"] == (k <= 13) and c["inverse"] and (c["nch"], c["nblocks"]) == ((3, 2) if k <= 16 else (2, 1) if k <= 19 else (1, 1))
    assert {c["k"] for c in dc.sweep_cases() if c["src"] == "full"} == {5, 7, 12, 17, 19, 21}
    assert {c["k"] for c in dc.sweep_cases() if c["bps"] == 3} == {9, 17}
    assert {c["k"] for c in dc.sweep_cases() if c["planar"]} == {5, 17, 21}
    # each block is different, each channel has its own mean, some negative
    c = by["noise_k16"]
    a, b = dc.block_i32(c, 0), dc.block_i32(c, 1)
    assert not (a == b).all()
    m = a.mean(axis=1)  # (the noise's own mean is about 150 here)
    assert len(set(np.rint(m / 10))) == c["nch"] and (m < -300).any() and (m > 300).any()


def test_every_case_keeps_out_of_the_band(record):
    want = dc.all_cases()
    assert sorted(record) == sorted(c["name"] for c in want)
    for c in want:
        e = record[c["name"]]
        assert [e[k] for k in ("src", "bps", "nch", "ns", "nblocks", "q", "nb")] == [c[k] for k in ("src", "bps", "nch", "ns", "nblocks", "q", "nb")]
        assert e["fwd_share"] <= dc.CAP and len(e["fwd_digest"]) == c["nblocks"], c["name"]
        # the band leaves three orders of magnitude over a correct fp64 FFT's error
        assert e["fwd_err_eps"] * 1000 <= dc.BAND / dc.EPS, c["name"]
        assert ("inv_share" in e) == c["inverse"]
        if c["inverse"]:
            assert e["inv_share"] <= dc.CAP and e["inv_err_eps"] * 1000 <= dc.BAND / dc.EPS, c["name"]
        elif c["src"] == "full":  # a leg is left out only where the inputs would be what is tested
            assert e["inverse_share_not_run"] > dc.CAP, c["name"]


@pytest.mark.parametrize("name", SMALL)
def test_the_restatement_passes_the_rule_and_the_record_is_reproduced(record, orc, name):
    """oracle.dct_big_compress / dct_big_decompress, the checker of tests/test_gpu_dct_fft.py, held to check_exact (the
    reference's own quantiser: the noise and ECG-like cases; a full-scale case through its untruncated coefficient array)"""
    c, e = dc.by_name()[name], record[name]
    for i in range(c["nblocks"]):
        x = dc.block_i32(c, i)
        v, means = dc.exact_forward(x, c["ns"], c["q"])
        assert dc.digest(v) == e["fwd_digest"][i], (name, i)
        if c["q"] != 128.0:
            continue
        stream, coeffs = orc.dct_big_compress(dc.block_native(c, x), c["bps"], c["nch"], c["ns"])
        share = dc.check_exact(coeffs, v, "%s block %d forward" % (name, i))
        assert share <= e["fwd_share"]
        if c["nb"] != 2:
            continue  # (the stream of dct_big_compress keeps two planes)
        assert stream[1:1 + 3 * c["nch"]] == dc.header_bytes(means)
        got, header = dc.stream_coeffs(orc, stream, c)
        assert (got == coeffs).all() and header == dc.header_bytes(means)
        if c["inverse"]:
            m24 = dc.means24_of(means)
            w = dc.exact_inverse(coeffs, m24, c["ns"], c["q"])
            assert (coeffs == np.trunc(v)).all()  # (nothing in the band: the inverse is the record's)
            assert dc.digest(w) == e["inv_digest"][i], (name, i)
            dec, used = orc.dct_big_decompress(stream, c["bps"], c["nch"], c["ns"])
            assert used == len(stream)
            dec = dc.lq.native_to_i32(np.frombuffer(dec, dtype=np.uint8), c["bps"], c["nch"], c["ns"])
            dc.check_exact(dc.decoded_minus_mean(dec, m24), w, "%s block %d inverse" % (name, i))


def test_one_count_on_one_coefficient_is_rejected():
    c = dc.by_name()["noise_k10"]
    x = dc.block_i32(c, 0)
    v, _ = dc.exact_forward(x, c["ns"])
    good = np.trunc(v).astype(np.int64).astype(np.int32)
    stats = {}
    assert dc.check_exact(good, v, "unchanged", stats) == 0.0 and stats == {"values": v.size, "band": 0, "flips": 0}
    for row, i, step in ((0, 0, 1), (1, c["ns"] // 2, -1), (2, c["ns"] - 1, 1), (1, 7, 1)):
        bad = good.copy()
        bad[row, i] += step
        with pytest.raises(AssertionError, match=r"1 of %d values outside the rule \(first: \[%d, %d\]" % (v.size, row, i)):
            dc.check_exact(bad, v, "moved")
    # a value that truncates to 0 admits nothing but 0, on either side
    i = int(np.argmin(np.abs(v[0])))
    assert abs(v[0, i]) < 1
    for step in (1, -1):
        bad = good.copy()
        bad[0, i] = step
        with pytest.raises(AssertionError):
            dc.check_exact(bad, v, "zero")


def test_the_band_is_where_it_is_said_to_be():
    LD = dc.LD
    d = LD(1000) * LD(dc.BAND)  # 3.6e-9
    v = np.array([[LD(1000), LD(3) + d / 2, LD(7) - d / 2, LD(-2) + d / 2, LD(0.2), d / 2, LD(5) + 2 * d, LD(-1) - d / 2]], dtype=LD)
    assert dc.band_of(v).tolist() == [[True, True, True, True, False, False, False, True]]
    good = [1000, 3, 6, -1, 0, 0, 5, -1]
    stats = {}
    assert dc.check_exact(np.array([good]), v, "exact", stats) == 5 / 8 and stats["flips"] == 0
    assert dc.check_exact(np.array([[1000, 2, 7, -2, 0, 0, 5, -2]]), v, "the other side of each boundary", stats) == 5 / 8 and stats["flips"] == 4
    for i, g in ((1, 5), (2, 4), (4, 1), (4, -1), (5, 1), (6, 6), (6, 4), (7, -3), (0, 1002)):
        bad = list(good)
        bad[i] = g
        with pytest.raises(AssertionError):
            dc.check_exact(np.array([bad]), v, "element %d" % i)
