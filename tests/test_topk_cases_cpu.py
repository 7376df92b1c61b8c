"""CPU: the case table of ii2_topk_ranges (tests/topk_cases.py) is worth running - for every case some k cuts inside a score class
(a real tie at the cut), some k takes a class whole, some k asks for more docs than are eligible, and the tombstone run differs from
the plain one wherever the case names removed ids.  A case taken over from tests/atleast_cases.py must do so wherever its scores
allow it (some hold no two docs of one score); the cases written for the ranking must, all of them."""
import numpy as np
import pytest

from tests import atleast_cases as ac
from tests import topk_cases as tc


def _kinds(t, tomb=False):
    """which of {tie, whole, beyond} the case's (min_match, k) runs show"""
    seen = set()
    for m in t.min_matches:
        _, _, hist = tc.reference(t.case, 0, m, tomb)
        total = int(hist.sum())
        for k in t.ks:
            _, c, above, n_cut = tc.cut(hist, k)
            if total and int(hist[c]) > n_cut:
                seen.add("tie")
            if total and k <= total and int(hist[c]) == n_cut:
                seen.add("whole")
            if k > total:
                seen.add("beyond")
    return seen


def _possible(t):
    out = {"beyond"}
    for m in t.min_matches:
        _, _, hist = tc.reference(t.case, 0, m)
        if hist.any():
            out.add("whole")
        if (hist >= 2).any():
            out.add("tie")
    return out


@pytest.mark.parametrize("t", tc.CASES, ids=lambda t: t.name)
def test_every_case_cuts_ties_and_runs_out(t):
    want = {"tie", "whole", "beyond"} if t.strict else _possible(t)
    assert _kinds(t) >= want, (t.name, _kinds(t), want)
    assert 0 not in t.ks and t.ks == sorted(set(t.ks)) and 1 <= len(t.ks) <= 11


@pytest.mark.parametrize("t", tc.CASES, ids=lambda t: t.name)
def test_the_tombstone_run_differs(t):
    if not len(t.case.removed):
        assert t.name == "high_ids" or not t.strict
        return
    differs = False
    for m in t.min_matches:
        for k in t.ks:
            a, b = tc.reference(t.case, k, m), tc.reference(t.case, k, m, tomb=True)
            differs = differs or not (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]))
    assert differs, t.name


def test_the_table_holds_every_atleast_case_that_fits():
    names = {t.name for t in tc.CASES}
    for c in ac.CASES:
        assert (c.name in names) == (c.n_counted <= 255), c.name
        if c.name in names:
            assert tc.BY_NAME[c.name].min_matches == sorted({1, c.m})
    for name in ("tie_in_word", "tie_across_seams", "dense_classes", "every_score_255", "excluded_and_removed_top", "high_ids", "empty_groups"):
        assert tc.BY_NAME[name].strict


def test_reference_on_hand_made_answers():
    t = tc.BY_NAME["every_score_255"]
    ids, scores, hist = tc.reference(t.case, 57)
    assert ids[:55].tolist() == list(range(255, 200, -1)) and ids[55:].tolist() == [200, 1000] and scores[55:].tolist() == [200, 200]
    assert tc.cut(hist, 57) == (255, 200, 55, 2) and int(hist[200]) == 11 and int(hist.sum()) == 265
    t = tc.BY_NAME["dense_classes"]
    _, _, hist = tc.reference(t.case, 0)
    assert [int(hist[s]) for s in (3, 2, 1)] == [200, 1400, 2800]
    ids, scores, _ = tc.reference(t.case, 201)
    assert ids[199:].tolist() == [5970, 6] and scores[199:].tolist() == [3, 2]
    t = tc.BY_NAME["tie_in_word"]
    ids, scores, _ = tc.reference(t.case, 4)
    assert ids.tolist() == [5, 17, 0, 1] and scores.tolist() == [3, 3, 2, 2]
    t = tc.BY_NAME["excluded_and_removed_top"]
    assert tc.reference(t.case, 2)[0].tolist() == [20, 30] and tc.reference(t.case, 2, tomb=True)[0].tolist() == [30, 31]
    t = tc.BY_NAME["empty_groups"]
    assert tc.reference(t.case, 5, 4)[0].size == 0 and t.case.n_counted == 3
    assert tc.cut(np.zeros(256, np.uint64), 5) == (0, 0, 0, 0) and tc.cut(hist, 0) == (0, 0, 0, 0)
