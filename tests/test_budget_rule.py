"""Compress to a byte budget on the CPU: the restated stream size of tests/budget_cases.py against the reference's own streams, and
its cases against the conditions they exist for.  tests/test_gpu_budget.py then holds the device to the same rule."""
import numpy as np

import budget_cases as bc
import devframe as df
import lossy_quantizer_cases as lq

MODE_COPY, MODE_HUFF, MODE_FILL = 0, 1, 2  # libhzr's block modes (hzr_encode.c), as the oracle's hzr_block_stats names them


def _R():
    return {c["name"]: (c, bc.restated(c)) for c in bc.rule_cases()}


def _modes(c, native, q):
    """the libhzr mode of every plane of a block (shapes of one hzr block per plane)"""
    assert c["shape"][2] * c["shape"][3] <= 65536
    return [bc.oracle().hzr_block_stats(p)[1] for p in bc.planes_of(*c["shape"], native, q)]


def test_the_restated_size_is_the_size_of_the_reference_s_stream():
    """every case of the record that the restatement covers: hadamard at every row length, the dct on the dense table"""
    rec = {e["name"]: e for e in df.golden("lossy_quantizer_record.json")["cases"]}
    seen = set()
    for c in lq.all_cases():
        if c["fft"] is not None:
            continue
        for i, blk in enumerate(rec[c["name"]]["blocks"]):
            native = lq.block_data(c, i)
            assert lq.crc(native) == blk["in_crc32"], c["name"]
            got = bc.restated_size(c["kind"], c["bps"], c["nch"], c["ns"], c["nb"], native, c["q"])
            assert got == blk["size"], (c["name"], i, got, blk["size"])
        seen.add((c["kind"], c["ns"] > 65536))
    assert seen == {("hadamard", False), ("hadamard", True), ("dct", False)}


def test_choose_states_the_rule():
    assert bc.choose([10, 20, 30], 20) == 1 and bc.choose([10, 20, 30], 19) == 0 and bc.choose([10, 20, 30], bc.U64_MAX) == 2
    assert bc.choose([30, 10, 40, 20], 20) == 3  # the highest fitting index, past one that does not fit
    assert bc.choose([10, 20, 20, 40], 20) == 2  # equal sizes: the later index
    assert bc.choose([30, 10, 10, 20], 9) == 1 and bc.choose([30, 10, 10, 20], 0) == 1  # nothing fits: the smallest, its lowest index
    assert bc.choose([7], 0) == 0 and bc.choose([7], 7) == 0


def test_every_ladder_index_is_chosen_and_one_block_fits_nothing():
    c, (natives, table, budgets, choices) = _R()["every_index"]
    assert set(choices) == set(range(len(c["ladder"]))), choices
    missed = [b for b in range(c["nblocks"]) if table[choices[b], b] > budgets[b]]
    assert missed and all(budgets[b] < table[:, b].min() and choices[b] == int(np.argmin(table[:, b])) for b in missed)
    assert all(table[choices[b], b] <= budgets[b] for b in range(c["nblocks"]) if b not in missed)


def test_budgets_sit_exactly_at_a_size_and_one_byte_below():
    c, (natives, table, budgets, choices) = _R()["every_index"]
    at = [b for b in range(c["nblocks"]) if budgets[b] == table[choices[b], b]]
    below = [(b, k) for b in range(c["nblocks"]) for k in range(len(c["ladder"])) if budgets[b] == table[k, b] - 1]
    assert len(at) >= len(c["ladder"]), at
    fitting = [(b, k) for b, k in below if table[:, b].min() <= budgets[b]]
    assert fitting and all(choices[b] != k for b, k in fitting), below  # (one byte short of entry k: where anything fits, k is not taken)
    assert any(choices[b] == k - 1 for b, k in below if k > 0)


def test_the_highest_fitting_index_skips_one_that_does_not_fit():
    c, (natives, table, budgets, choices) = _R()["unsorted"]
    assert any(np.any(np.diff(table[:, b]) < 0) for b in range(c["nblocks"])), "the sizes are sorted in ladder order"
    skips = [b for b in range(c["nblocks"]) if any(table[j, b] > budgets[b] for j in range(choices[b])) and table[choices[b], b] <= budgets[b]]
    assert skips, (table, budgets, choices)


def test_of_a_repeated_quality_the_later_index_wins():
    c, (natives, table, budgets, choices) = _R()["repeated"]
    assert c["ladder"][1] == c["ladder"][2] and np.array_equal(table[1], table[2])
    assert any(choices[b] == 2 and budgets[b] == table[1, b] for b in range(c["nblocks"])), (budgets, choices)
    assert 1 not in choices


def test_constant_planes_are_fill_blocks_of_one_size_at_every_entry():
    c, (natives, table, budgets, choices) = _R()["constant"]
    for q in c["ladder"]:
        assert set(_modes(c, natives[0], q)) == {MODE_FILL}
    assert len(set(table.reshape(-1).tolist())) == 1
    K = len(c["ladder"])
    assert K - 1 in choices and 0 in choices  # all fit: the finest; none fits: the lowest index among equals
    assert all(choices[b] == (K - 1 if budgets[b] >= table[0, b] else 0) for b in range(c["nblocks"]))


def test_a_fine_candidate_is_stored_uncompressed():
    c, (natives, table, budgets, choices) = _R()["stored"]
    coarse, fine = _modes(c, natives[0], c["ladder"][0]), _modes(c, natives[0], c["ladder"][-1])
    assert any(a == MODE_HUFF and b == MODE_COPY for a, b in zip(coarse, fine)), (coarse, fine)
    assert len(c["ladder"]) - 1 in choices


def test_the_dct_cases_choose_differently_inside_one_batch():
    c, (natives, table, budgets, choices) = _R()["dct"]
    assert len(set(choices)) >= 3 and np.all(np.diff(table[:, 0]) > 0)


def test_derived_budgets_fit_every_batch_shape():
    for K, B in ((4, 5), (8, 1), (8, 9), (1, 3)):
        t = np.arange(1, K * B + 1, dtype=np.int64).reshape(K, B) * 100
        b = bc.derive_budgets(t)
        assert len(b) == B and all(v >= 0 for v in b)
        assert [bc.choose(t[:, j], b[j]) for j in range(min(K, B))] == list(range(min(K, B)))
    assert bc.scalar_budget(np.array([[5, 1], [9, 7]])) == 7
