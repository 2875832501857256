"""What the device tests of compress-a-batch-to-one-byte-total share (tests/test_gpu_total.py): the comparison of everything one
rspt_hip_compress_total_batch_dev returns (lossy_dev.rate_call) with the composed oracle's tables put through the rule of
tests/total_cases.py.

torch is imported inside the functions, as in tests/devframe.py."""
import numpy as np

import lossy_dev as ld
import total_cases as tt


def tables_of(oracle):
    """lossy_dev.composed(..., prdn=True) -> (sizes, prdn, mse, path), each [K][B]"""
    sizes = np.stack([o["sizes"] for o in oracle])
    assert sizes.min() > 0 and not (sizes.view(np.uint64) >> np.uint64(63)).any()
    return sizes, np.stack([o["prdn"] for o in oracle]), np.stack([o["mse"] for o in oracle]), np.stack([o["path"] for o in oracle])


def figure_bits(prdn, mse, path):
    """the table of figures as the device reports it, as bit patterns"""
    is_rated = (path == 0) & ((mse == 0.0) | ~np.isnan(prdn))
    fig = np.where(mse == 0.0, 0.0, prdn)
    return np.where(is_rated, fig, np.float64(tt.from_bits(tt.NAN_BITS))).view(np.uint64), is_rated


def as_lists(sizes, prdn, mse, path):
    K, B = sizes.shape
    return ([[int(sizes[k, b]) for b in range(B)] for k in range(K)],
            [[(float(prdn[k, b]), float(mse[k, b]), int(path[k, b])) for b in range(B)] for k in range(K)])


def some_totals(oracle, n=8):
    """6 to n + 2 totals placed on the oracle's own tables (total_cases.some_totals, its numpy form for more than 64 blocks)"""
    t = tables_of(oracle)
    return tt.some_totals(*as_lists(*t), n=n) if t[0].shape[1] <= 64 else tt.some_totals_np(*t, n=n)


def held_to_the_oracle(pk, d_src, ladder, oracle, total, tag, second="brute"):
    """one total call, checked in full against the rule on the oracle's tables: the vectorised statement, and beside it a second
    one -- "brute": choose_total; "bisect": choose_total_bisect, for batches too large for every level in turn; None: none.
    -> (level, choice, cost) as the rule gives them"""
    sizes, prdn, mse, path = tables_of(oracle)
    K, B = sizes.shape
    level, choice, cost = tt.choose_total_np(sizes, prdn, mse, path, total)
    if second:
        want = (tt.choose_total if second == "brute" else tt.choose_total_bisect)(*as_lists(sizes, prdn, mse, path), total)
        assert tt.same_level(want[0], level) and want[1] == choice.tolist() and want[2] == cost, (tag, "the two statements of the rule")
    got = ld.rate_call(pk, "total", d_src, total, ladder, tag)
    fbits, is_rated = figure_bits(prdn, mse, path)
    assert np.array_equal(got["cand"], sizes), (tag, "the table of candidate sizes")
    assert np.array_equal(got["figs"].view(np.uint64), fbits), (tag, "the table of figures")
    assert got["level"] == tt.bits(level), (tag, tt.from_bits(got["level"]), level)
    assert np.array_equal(got["choice"], choice), (tag, np.flatnonzero(got["choice"] != choice)[:8].tolist())
    assert got["total"] == cost, (tag, got["total"], cost)
    rows = np.arange(B)
    want_prdn = np.where(path[choice, rows] != 0, np.float64(tt.INF), fbits[choice, rows].view(np.float64))
    assert np.array_equal(got["prdn"].view(np.uint64), want_prdn.view(np.uint64)), (tag, "d_prdn")
    n = sizes[choice, rows]
    assert np.array_equal(got["sizes"], n), (tag, "d_sizes")
    cols = np.arange(got["dst"].shape[1])[None, :]
    for k in np.unique(choice):
        r = rows[choice == k]
        assert ((got["dst"][r] == oracle[k]["dst"][r]) | (cols >= n[r, None])).all(), (tag, k, "streams")
        assert np.array_equal(got["out"][r], oracle[k]["out"][r]), (tag, k, "decoded")
    return level, choice, cost
