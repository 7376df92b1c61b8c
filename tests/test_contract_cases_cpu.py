"""The contract tables are sound (tests/contract_cases.py; no GPU): every layout of removed ids does on every distinct path case
what it says it aims at - where the bitmap ends, what its last word holds, which summary bits lie about which survivors - every
reference is a non-trivial part of the result, and the only case no layout runs on is the one with a single result id."""
import numpy as np
import pytest

from tests import contract_cases as cc
from tests import path_cases as pc

RUN = [c for c in cc.PATH_CASES if c.name not in cc.DEGENERATE]


@pytest.fixture(scope="module")
def sets():
    cache = {}

    def get(case):
        if case.name not in cache:
            lists = case.lists()
            cache[case.name] = (lists,) + cc.sets_of(case, lists)
        return cache[case.name]
    return get


def test_the_distinct_cases():
    names = [c.name for c in cc.PATH_CASES]
    assert len(set(names)) == len(names)
    assert set(cc.TOMB_ONLY) <= set(names) and set(cc.DEGENERATE) <= set(names)
    twins = {c.name[:-len("_tomb")] for c in pc.CASES if c.name.endswith("_tomb")}
    assert twins <= set(names) and not any(n.endswith("_tomb") for n in names)
    assert len(names) == len(pc.CASES) - len(twins)
    # nothing of the path table is lost: every path id a case of pc.CASES expects is expected by a distinct case
    paths = lambda cases: {k for c in cases for k in c.expect}
    assert paths(cc.PATH_CASES) == paths(pc.CASES)


def test_the_skipped_pairs_are_the_one_degenerate_case(sets):
    """a (case, layout) pair is left out only when the case has fewer than two result ids"""
    skipped = set()
    for case in cc.PATH_CASES:
        _, R, E = sets(case)
        for layout in cc.LAYOUTS:
            if cc.removed_for(layout, R, E) is None:
                assert R.size < 2, (case.name, layout)
                skipped.add((case.name, layout))
    assert skipped == {("and_tiles_sub_driver_of_1", layout) for layout in cc.LAYOUTS}
    assert {name for name, _ in skipped} == set(cc.DEGENERATE)
    assert all(c.degenerate is not None for c in cc.PATH_CASES if c.name in cc.DEGENERATE)


def test_capacities():
    assert cc.capacities(5) == [5, 4, 0] and cc.capacities(1) == [1, 0] and cc.capacities(0) == [0]


def test_the_bitmap_model():
    assert (cc.n_words([]), cc.last_word([])) == (0, 0)
    assert (cc.n_words([31]), cc.n_words([32]), cc.n_words([0xFFFFFFFF])) == (1, 2, 1 << 27)
    assert cc.last_word([1, 31, 32, 35]) == 0b1001 and cc.last_word([0, 31]) == 0x80000001
    assert cc.last_word(np.arange(64, 96)) == 0xFFFFFFFF


def test_the_merge_cases_count_both_leaves_and_neither():
    from tests import merge_cases as mc
    cases = [mc.BY_NAME[name] for name in cc.MERGE_CASES]
    events = [set(c.events()) for c in cases]
    assert events[:3] == [set(), set(), set()]
    assert ["bitmap" in c.plan().branches for c in cases[:3]] == [True, False, False]
    assert ["range" in c.plan().branches for c in cases[:3]] == [False, True, False]
    assert cases[2].plan().branches & {"small", "large"} == {"small"}              # small terms only
    assert {"leaf_bitmap", "leaf_sorted"} <= events[3] and "leaf_bitmap" in events[4]
    for c in cases:                                                                 # every layout fits the merged ids
        R = cc.every_id([v for _, v in c.segs()])
        assert all(cc.removed_for(layout, R, R) is not None for layout in cc.LAYOUTS), c.name


@pytest.mark.parametrize("case", RUN, ids=lambda c: c.name)
def test_every_layout_aims_where_it_says(sets, case):
    lists, R, E = sets(case)
    assert R.size >= 28 and np.all(np.isin(R, E))
    h = cc.middle(R)
    removed = {layout: cc.removed_for(layout, R, E) for layout in cc.LAYOUTS}
    assert all(r is not None and r.dtype == np.uint32 and np.all(np.diff(r.astype(np.int64)) > 0) for r in removed.values())
    survivors = {layout: cc.hits(pc.reference(case, lists, r)) for layout, r in removed.items()}
    for layout, S in survivors.items():
        assert np.array_equal(S, np.setdiff1d(R, removed[layout].astype(np.uint64))), layout
    # -- the layouts that end inside the lists: a bitmap that is there, ends below the lists' last id and below hits
    for layout in cc.ENDS_INSIDE:
        nw = cc.n_words(removed[layout])
        assert 0 < nw * 32 <= int(E[-1]), layout
        assert int(R[-1]) >= nw * 32, layout                              # hits above the last word
        assert np.count_nonzero(R >= nw * 32) == np.count_nonzero(survivors[layout] >= nw * 32) > 0, layout
    assert cc.n_words(removed["empty"]) == 0 and removed["empty"].size == 0
    # -- one bit in the last word, a hit; once in a word of even and once of odd index
    one, other = removed["one_hit_last"], removed["one_hit_last_other_parity"]
    assert one.tolist() == [h] and other.size == 1 and other[0] in R
    assert cc.last_word(one) == 1 << (h & 31) and cc.last_word(other) == 1 << (int(other[0]) & 31)
    assert ((h >> 5) & 1) != ((int(other[0]) >> 5) & 1)
    # -- a last word of all ones, hits removed below it
    full = removed["last_word_full"]
    assert cc.last_word(full) == 0xFFFFFFFF and cc.n_words(full) == (h >> 5) + 1
    assert np.count_nonzero(np.isin(full, R) & (full < (h & ~31))) > 0
    # -- the summary lies both ways
    near = removed["summary_neighbours"].astype(np.uint64)
    S = survivors["summary_neighbours"]
    not_hits, gone = np.setdiff1d(near, R), np.intersect1d(near, R)
    g = np.uint64(cc.GROUP_SHIFT)
    lied_to = S[np.isin(S >> g, not_hits >> g)]                           # survivors whose summary bit is set by a doc that is no hit
    assert lied_to.size > 0
    # a removed hit and a survivor in one summary word: everywhere but in the two cases whose hits lie thousands of docs apart
    shared = bool(np.any(np.isin(gone >> np.uint64(cc.SUMMARY_SHIFT), S >> np.uint64(cc.SUMMARY_SHIFT))))
    assert gone.size > 0 and shared == (case.name not in cc.NO_SHARED_SUMMARY_WORD)
    if not shared:
        assert (int(R[-1]) - int(R[0])) // R.size > 8 << cc.SUMMARY_SHIFT and "or.merge" not in case.expect
    # -- nothing left; a bitmap far past every list
    assert np.array_equal(removed["all_hits"].astype(np.uint64), R) and survivors["all_hits"].size == 0
    far = removed["far_beyond"]
    assert int(far[-1]) == min(int(E[-1]) + (1 << 20), cc.TOP) and cc.n_words(far) * 32 > int(E[-1])
    # -- every reference is a non-trivial strict part of R
    for layout, S in survivors.items():
        if layout == "empty":
            assert np.array_equal(S, R)
        elif layout != "all_hits":
            assert 0 < S.size < R.size and np.all(np.isin(S, R)), layout
