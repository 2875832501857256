"""The cases of compress-to-a-PRDN-target (tests/target_cases.py), held on the CPU to the conditions they exist for: the numpy
restatement of the rule must take the first entry, a middle one and -- nothing having met the target -- the last one; choose
differently inside one batch; pass over a candidate because its figure needs the sequential path; take one through mse == 0;
and sit on no rounding edge.  tests/test_gpu_target.py then holds the device to the same choices."""
import math

import target_cases as tc


def _all():
    return [(c, tc.restated(c)) for c in tc.all_cases()]


def test_the_choices_cover_first_middle_and_nothing_met():
    R = _all()
    picks = {(k, len(c["ladder"])) for c, blocks in R for figs, (k, p) in blocks}
    assert len({k for k, n in picks}) >= 3, sorted(picks)
    assert any(k == 0 for k, n in picks), "the first entry is never chosen"
    assert any(0 < k < n - 1 for k, n in picks), "no middle entry is chosen"
    none_met = [c["name"] for c, blocks in R for figs, (k, p) in blocks
                if k == len(figs) - 1 and not any(tc.meets(pp, m, path, c["target"]) for pp, m, path in figs)]
    assert none_met, "no block falls through to the last entry"


def test_a_batch_chooses_differently_for_its_blocks():
    assert any(len({k for figs, (k, p) in blocks}) > 1 for c, blocks in _all())


def test_a_candidate_is_passed_over_for_its_path_alone():
    """full-scale samples at nb = 1: the figure would meet the target, but its error sum is not exact"""
    hits = [(c["name"], b, k) for c, blocks in _all() for b, (figs, pick) in enumerate(blocks) for k, (p, m, path) in enumerate(figs)
            if path == 1 and tc.meets(p, m, 0, c["target"])]
    assert hits
    c = next(c for c in tc.all_cases() if c["name"] == hits[0][0])
    figs, (k, p) = tc.restated(c)[hits[0][1]]
    assert k != hits[0][2] or p == math.inf  # (chosen only as the last entry nothing met, and then without a figure)


def test_a_candidate_is_taken_through_mse_zero():
    """a constant block: ref == 0 and the PRDN is a NaN, which never compares below a target"""
    assert any(figs[k][1] == 0.0 and figs[k][0] != figs[k][0] for c, blocks in _all() for figs, (k, p) in blocks)


def test_no_candidate_sits_on_the_edge_of_its_target():
    for c, blocks in _all():
        for b, (figs, pick) in enumerate(blocks):
            for k, (p, m, path) in enumerate(figs):
                if p == p and not math.isinf(p):
                    assert abs(p - c["target"]) > tc.EDGE * c["target"], (c["name"], b, k, p)


def test_every_case_orders_a_valid_ladder():
    for c in tc.all_cases():
        assert 1 <= len(c["ladder"]) <= 8 and all(math.isfinite(q) and q > 0 for q in c["ladder"]), c["name"]
        assert math.isfinite(c["target"]) and c["target"] > 0, c["name"]
