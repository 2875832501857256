"""Every hadamard row length 2^1 .. 2^16 without a GPU: the numpy restatement of the quantiser, of a stream's size and of the
PRDN figures against what the reference wrote and decoded at each length (tests/golden/hadamard_rows_record.json), and the case
list of tests/hadamard_rows_cases.py against the conditions it exists for.  tests/test_gpu_hadamard_rows.py then holds the device
to the same record."""
import numpy as np
import pytest

import budget_cases as bc
import devframe as df
import hadamard_rows_cases as hr
import lossy_quantizer_cases as lq
import target_cases as tc


@pytest.fixture(scope="module")
def rec():
    return {e["k"]: e for e in df.golden("hadamard_rows_record.json")["cases"]}


IDS = [hr.case_id(k) for k in hr.KS]


def test_the_record_holds_every_case_entry_and_block(rec):
    assert sorted(rec) == hr.KS
    for k in hr.KS:
        rows = hr.record_blocks(rec, k)  # (the shape and the ladder are the case's)
        assert len(rows) == len(hr.LADDER) and all(len(row) == hr.NBLOCKS for row in rows), k
        kind, bps, nch, ns, nb = hr.shapes()[k]
        for row in rows:
            for b, w in enumerate(row):
                assert lq.crc(hr.natives(k)[b]) == w["in_crc32"], (k, b)
                assert ("stream" in w) == ("decoded" in w) == (bps * nch * ns <= lq.FULL_LIMIT), (k, b)
                if "stream" in w:
                    s = lq.unpack(w["stream"])
                    assert (len(s), lq.crc(s)) == (w["size"], w["crc32"]) and lq.crc(lq.unpack(w["decoded"])) == w["dec_crc32"], (k, b)


@pytest.mark.parametrize("k", hr.KS, ids=IDS)
def test_the_restatement_is_the_reference_at_every_row_length(rec, orc, k):
    """the restated stored values decode to the reference's decoded block, the restated size is the reference's stream size, and
    where the record keeps a stream its values are the restated ones"""
    kind, bps, nch, ns, nb = hr.shapes()[k]
    for e, q in enumerate(hr.LADDER):
        c = hr.case_of(k, q)
        for b, w in enumerate(hr.record_blocks(rec, k)[e]):
            native = hr.natives(k)[b]
            want, m32 = lq.restated_stored(c, native)
            back = lq.restated_decode(c, want.reshape(nch, ns), tc.mean24(m32))
            assert lq.crc(back) == w["dec_crc32"], (k, q, b, "decoded")
            assert bc.restated_size(kind, bps, nch, ns, nb, native, q) == w["size"], (k, q, b, "size")
            if "stream" in w:
                got, means, used = lq.stream_values(orc, lq.unpack(w["stream"]), kind, nch, ns, nb)
                assert used == w["size"] and (got.reshape(-1) == want).all() and (means == tc.mean24(m32)).all(), (k, q, b, "stream")
                assert back.tobytes() == lq.unpack(w["decoded"]), (k, q, b)


@pytest.mark.parametrize("k", hr.FUSED, ids=[hr.case_id(k) for k in hr.FUSED])
def test_the_prdn_restatement_runs_where_the_probes_run(k):
    """every figure of the table comes out, a target can sit on one per ladder entry, and the rule's special cells are there: the
    constant block's NaN at mse == 0, which every target takes at the first entry"""
    figs = hr.restated_figures(k)
    assert len(figs) == len(hr.LADDER) and all(len(row) == hr.NBLOCKS for row in figs)
    assert {e for e, b in hr.finite_cells(figs)} == set(range(len(hr.LADDER))), (k, figs)
    const = bc.CONTENTS.index("const")
    assert all(row[const][0] != row[const][0] and row[const][1] == 0.0 and row[const][2] == 0 for row in figs), (k, [row[const] for row in figs])
    targets = hr.derive_targets(figs)
    assert len(targets) == 2 * len(hr.LADDER) + 2
    for t in targets:
        assert tc.choose([row[const] for row in figs], t)[0] == 0
    # the targets move the choice: over the list a block takes more than one entry
    assert any(len({tc.choose([row[b] for row in figs], t)[0] for t in targets}) > 1 for b in range(hr.NBLOCKS)), (k, targets)


def test_the_case_list_is_what_it_exists_for(rec):
    S = hr.shapes()
    assert sorted(S) == list(range(1, 17)) and all(S[k][0] == "hadamard" and S[k][3] == 1 << k for k in S)
    for r in range(3):
        mine = [S[k] for k in S if k % 3 == r]
        assert {s[4] for s in mine} == {1, 2, 3, 4} and {s[1] for s in mine} == {1, 2, 3, 4}, r
    assert all(S[k][2] == (1 if k == hr.NCH1_K else 3 if k <= 10 else 2) for k in S) and 1 <= hr.NCH1_K <= 16
    assert hr.FUSED == list(range(1, 14)) and (1 << hr.FUSED_MAX_K) == bc.BATCHED_MAX_NS == tc.FUSED_MAX_NS
    assert all(bc.batched(S[k], hr.NBLOCKS, len(hr.LADDER)) == (k in hr.FUSED) for k in S)
    assert len(hr.LADDER) == 4 and sorted(hr.CHOICE) == [0, 1, 2, 2, 3]  # the ladder call: every entry, one of them twice
    assert hr.NBLOCKS == len(bc.CONTENTS)  # random, walk, constant, full scale


def test_the_probe_launch_shapes_are_stated_once():
    """nt of host_rate.hip (probe_launch, the one launch of every fused probe) as tests/hadamard_rows_cases.py restates it, at the k
    the list expects: the five workgroup sizes -- 1, 2, 4, 8 and 16 waves of partial sums -- all occur, idle lanes below 512
    points included"""
    got = {k: hr.probe_threads(1 << k) for k in hr.FUSED}
    assert got == hr.PROBE_THREADS
    assert set(got.values()) == {64, 128, 256, 512, 1024}
    assert [k for k in hr.FUSED if got[k] == 256] == [11] and [k for k in hr.FUSED if got[k] == 512] == [12]
    assert all(got[k] * hr.TP_PER >= 1 << k for k in hr.FUSED)  # a thread holds TP_PER samples at the most
    assert [k for k in hr.FUSED if got[k] * hr.TP_PER > 1 << k] == list(range(1, 9))  # lanes that hold no octet
    for name, count in (("host_rate.hip", 1), ("host_target.hip", 0), ("host_budget.hip", 0), ("host_total.hip", 0)):  # probe_launch alone
        text = open("%s/rspt_amd/csrc/%s" % (df.ROOT, name)).read()
        assert text.count("nt = std::max(64u, std::min(1024u, g.ns / kTpPer));") == count and text.count("kTpPer") == count, name
    assert "constexpr uint32_t kTpPer = %d;" % hr.TP_PER in open("%s/rspt_amd/csrc/target.hip" % df.ROOT).read()


@pytest.mark.parametrize("k", hr.KS, ids=IDS)
def test_a_wrong_choice_or_a_missing_cut_would_show(rec, k):
    """per case: a block whose four ladder entries write four different streams; a block whose stored values at quality 3 are not
    all zero; and, below four planes (four keep a value whole), an entry whose values leave nb bytes, so that the cut is made"""
    kind, bps, nch, ns, nb = hr.shapes()[k]
    rows = hr.record_blocks(rec, k)
    assert any(len({(row[b]["size"], row[b]["crc32"]) for row in rows}) == len(hr.LADDER) for b in range(hr.NBLOCKS)), k
    assert hr.LADDER[2] == 3.0
    whole = [[lq.hadamard_forward(lq.native_to_i32(n, bps, nch, ns), q)[0].reshape(-1) for n in hr.natives(k)] for q in hr.LADDER]
    assert any((lq.cut_to_nb(y, nb) != 0).any() for y in whole[2]), k
    if nb < 4:
        assert any((lq.cut_to_nb(y, nb) != y).any() for row in whole for y in row), k
