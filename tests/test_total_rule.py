"""Compress a batch to one byte total on the CPU: the three statements of the rule in tests/total_cases.py against each other on
every case and every total placed on its table, and the cases against the conditions they exist for.  tests/test_gpu_total.py then
holds the device to the same rule."""
import math

import numpy as np

import target_cases as tc
import total_cases as tt

INF = tt.INF


def _R():
    return {c["name"]: (c, tt.restated(c)) for c in tt.rule_cases()}


def _arrays(figs):
    return [np.array([[f[i] for f in row] for row in figs]) for i in range(3)]


def test_choose_total_states_the_rule_on_a_table_made_by_hand():
    nan = float("nan")
    sizes = [[10, 10], [20, 30], [40, 50]]
    figs = [[(9.0, 1.0, 0), (8.0, 1.0, 0)], [(5.0, 1.0, 0), (5.0, 1.0, 0)], [(1.0, 1.0, 0), (2.0, 1.0, 0)]]
    assert tt.choose_total(sizes, figs, tt.U64_MAX) == (2.0, [2, 2], 90)  # the lowest admissible level: 1.0 leaves block 1 without a pick
    assert tt.choose_total(sizes, figs, 90) == (2.0, [2, 2], 90) and tt.choose_total(sizes, figs, 89) == (5.0, [1, 1], 50)  # <= is inclusive
    assert tt.choose_total(sizes, figs, 50) == (5.0, [1, 1], 50)  # one level moves both picks
    assert tt.choose_total(sizes, figs, 49) == (8.0, [1, 0], 30) and tt.choose_total(sizes, figs, 29) == (9.0, [0, 0], 20)
    assert tt.choose_total(sizes, figs, 19) == (INF, [0, 0], 20) and tt.choose_total(sizes, figs, 0) == (INF, [0, 0], 20)  # a miss
    # equal sizes: the lowest index; a dominated entry (larger and worse) is never picked; mse == 0 is the figure +0.0
    sizes = [[7, 9, 5], [7, 8, 5], [9, 3, 5]]
    figs = [[(3.0, 1.0, 0), (4.0, 1.0, 0), (nan, 0.0, 0)], [(2.0, 1.0, 0), (6.0, 1.0, 0), (nan, 1.0, 0)], [(2.5, 1.0, 0), (1.0, 1.0, 1), (7.0, 1.0, 1)]]
    assert tt.choose_total(sizes, figs, 100) == (4.0, [0, 0, 0], 21)
    assert tt.choose_total(sizes, figs, 20) == (6.0, [0, 1, 0], 20) and tt.choose_total(sizes, figs, 19) == (INF, [0, 1, 0], 20)
    # no rated block: +0.0 whatever the total, every block its smallest stream, the lowest index among equals
    figs = [[(nan, 1.0, 0), (1.0, 1.0, 1), (1.0, 0.0, 1)]] * 3
    assert tt.choose_total(sizes, figs, 0) == (0.0, [0, 2, 0], 15) and tt.choose_total(sizes, figs, 100) == (0.0, [0, 2, 0], 15)
    assert math.copysign(1.0, tt.choose_total(sizes, figs, 0)[0]) == 1.0


def test_the_three_statements_agree_on_every_case_and_every_total():
    for name, (c, (sizes, figs)) in _R().items():
        prdn, mse, path = _arrays(figs)
        totals = tt.derive_totals(sizes, figs)
        assert len(totals) >= 4 and totals[0] == 0 and totals[-1] == tt.U64_MAX
        for total in totals:
            want = tt.choose_total(sizes, figs, total)
            for other in (tt.choose_total_bisect(sizes, figs, total), tt.choose_total_np(sizes, prdn, mse, path, total)):
                assert tt.same_level(other[0], want[0]) and list(other[1]) == want[1] and other[2] == want[2], (name, total, want, other)


def test_totals_on_the_table_give_their_level_and_the_next_one():
    """cost(L) gives the lowest level of that cost -- L itself where the cost drops at L -- and cost(L) - 1 the next level of a
    smaller cost; below cost(+inf) is a miss; 2^64 - 1 gives the lowest admissible level"""
    for name, (c, (sizes, figs)) in _R().items():
        adm = [(L, tt.cost_at(sizes, figs, L)) for L in tt.levels_of(figs) if tt.cost_at(sizes, figs, L) is not None]
        assert adm[-1][0] == INF
        if not any(tt.rated(f) for row in figs for f in row):
            continue
        drops = 0
        for i, (L, cost) in enumerate(adm):
            first = next(M for M, cM in adm if cM <= cost)
            assert tt.choose_total(sizes, figs, cost)[::2] == (first, cost), (name, L)
            drops += first == L
            below = [(M, cM) for M, cM in adm if cM < cost]
            got = tt.choose_total(sizes, figs, cost - 1)
            assert got[::2] == (below[0] if below else (INF, adm[-1][1])), (name, L)
        assert drops >= (1 if name == "unrated" else 2), name  # (all sizes of "unrated" are equal: one cost)
        miss = tt.choose_total(sizes, figs, adm[-1][1] - 1)
        assert miss[0] == INF and miss[2] > adm[-1][1] - 1 and tt.choose_total(sizes, figs, 0)[0] == INF
        assert tt.choose_total(sizes, figs, tt.U64_MAX)[::2] == adm[0], name


def test_sizes_ascend_and_figures_descend_and_the_target_rule_agrees():
    c, (sizes, figs) = _R()["sorted"]
    s, f = np.array(sizes), np.array([[tt.figure(x) for x in row] for row in figs])
    assert np.all(np.diff(s, axis=0) > 0) and np.all(np.diff(f, axis=0) < 0)
    assert len(set(f.reshape(-1).tolist())) == f.size == 24 and f.max() > 16.7 and f.min() < 0.028
    assert any(f[k].max() > 10 * f[k].min() for k in range(4))  # blocks of one batch a decade apart at one entry
    seen = set()
    for total in tt.derive_totals(sizes, figs):
        level, choice, cost = tt.choose_total(sizes, figs, total)
        seen.add(level)
        for b in range(c["nblocks"]):
            col = [figs[k][b] for k in range(4)]
            if any(tc.meets(*x, level) for x in col):
                assert tc.choose(col, level)[0] == choice[b], (total, b)
    assert len(seen) >= 10 and INF in seen


def test_neither_table_is_sorted_in_ladder_order():
    c, (sizes, figs) = _R()["unsorted"]
    s, f = np.array(sizes), np.array([[tt.figure(x) for x in row] for row in figs])
    for b in range(c["nblocks"]):
        assert np.any(np.diff(s[:, b]) < 0) and np.any(np.diff(s[:, b]) > 0) and np.any(np.diff(f[:, b]) < 0) and np.any(np.diff(f[:, b]) > 0)
    picked = {k for total in tt.derive_totals(sizes, figs) for k in tt.choose_total(sizes, figs, total)[1]}
    assert picked == {0, 1, 2, 3}


def test_constant_blocks_have_the_figure_zero_and_take_entry_0():
    c, (sizes, figs) = _R()["constant"]
    for b in (0, 2):
        assert all(figs[k][b][1] == 0.0 and math.isnan(figs[k][b][0]) and figs[k][b][2] == 0 and sizes[k][b] == 42 for k in range(4))
        assert all(tt.rated(figs[k][b]) and tt.bits(tt.figure(figs[k][b])) == 0 for k in range(4))
    for total in tt.derive_totals(sizes, figs):
        choice = tt.choose_total(sizes, figs, total)[1]
        assert choice[0] == 0 and choice[2] == 0


def test_blocks_of_path_1_are_unrated_and_equal_sizes_take_the_lowest_index_that_meets_the_level():
    c, (sizes, figs) = _R()["unrated"]
    assert all(figs[k][b][2] == 1 for k in range(3) for b in (0, 2)) and all(figs[k][1][2] == 0 for k in range(3))
    assert all(sizes[k][b] == 150 for k in range(3) for b in range(3))
    f = [tt.figure(figs[k][1]) for k in range(3)]
    assert f[0] < f[2] < f[1] and 73 < f[0] < 74 and 111 < f[1] < 112
    for total in (0, 449, 450, tt.U64_MAX):
        level, choice, cost = tt.choose_total(sizes, figs, total)
        assert choice == [0, 0, 0] and cost == 450 and level == (f[0] if total >= 450 else INF)
    assert math.isnan(tt.figure(figs[0][0])) and tt.reported(figs[0][0]) == INF


def test_a_path_1_entry_beside_rated_ones_and_a_dominated_entry_are_never_picked():
    c, (sizes, figs) = _R()["dct"]
    for b in (0, 1):
        assert figs[0][b][2] == 1 and all(figs[k][b][2] == 0 for k in (1, 2, 3))
        assert sizes[3][b] > sizes[2][b] and tt.figure(figs[3][b]) > tt.figure(figs[2][b])  # entry 3: larger and worse than entry 2
        assert sizes[0][b] == min(sizes[k][b] for k in range(4))  # (the smallest stream of all, and not to be had)
    assert all(figs[k][2][1] == 0.0 for k in range(4))
    picked = [tt.choose_total(sizes, figs, total)[1] for total in tt.derive_totals(sizes, figs)]
    assert {ch[b] for ch in picked for b in (0, 1)} == {1, 2} and {ch[2] for ch in picked} == {0}


def test_equal_figures_in_two_blocks_move_two_picks_at_one_level():
    c, (sizes, figs) = _R()["twins"]
    assert [row[2] for row in figs] == [row[0] for row in figs] and [row[2] for row in sizes] == [row[0] for row in sizes]
    levels = [L for L in tt.levels_of(figs) if tt.cost_at(sizes, figs, L) is not None]
    moved = 0
    for lo, hi in zip(levels, levels[1:]):
        a, b = tt._picks(sizes, figs, lo)[0], tt._picks(sizes, figs, hi)[0]
        diff = [i for i in range(c["nblocks"]) if a[i] != b[i]]
        assert (0 in diff) == (2 in diff)
        moved += diff == [0, 2]
    assert moved >= 2
