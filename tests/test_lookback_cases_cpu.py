"""CPU: the table of tests/lookback_cases.py reaches every branch of the look-back walk it is named for, and its decoys bite -
proved from the plain-Python specification alone, no device.  (tests/test_gpu_lookback_protocol.py then holds the kernels to
that specification.)"""
import numpy as np
import pytest

from tests import lookback_cases as lc

CASES = lc.CASES
OK_CASES = [c for c in CASES if not c.gives_up]


def _outcomes(case, rules=lc.SPEC):
    rec, live = case.records(), case.amounts()
    return [(k, i, lc.walk(rec, i, live[:k], rules)) for k in lc.SIZES for i in range(k)]


def test_names_are_unique_and_the_table_covers_the_branches():
    assert len(lc.BY_NAME) == len(CASES)
    have = {(c.G, c.windows, c.dist, c.gives_up) for c in CASES}
    # (group, windows, place of the prefix, gives up) - every row of the branch list
    for row in [(0, 0, lc.NO_PREFIX, False), (1, 0, lc.NO_PREFIX, False), (2, 1, lc.NO_PREFIX, False),          # no window / the smallest one
                (2, 1, 0, False), (33, 1, 0, False), (33, 1, 31, False),                                        # prefix at 0, in the last lane
                (33, 1, lc.NO_PREFIX, False), (34, 2, lc.NO_PREFIX, False),                                     # the window is left
                (35, 2, lc.NO_PREFIX, False), (66, 3, lc.NO_PREFIX, False), (67, 3, lc.NO_PREFIX, False),       # 2 and 3 windows
                (70, 2, 0, False), (70, 2, 5, False), (70, 2, 31, False),                                       # prefix in a later window
                (40, 1, 9, False), (40, 1, lc.NO_PREFIX, True),                                                 # stale / later; give-ups
                (40, 1, 2, False), (70, 3, lc.NO_PREFIX, False), (70, 1, 0, False), (80, 1, 0, False)]:         # 40-bit values; the last epoch
        assert row in have, row
    assert {c.G for c in CASES if c.epoch == lc.EPOCH_MAX} == {70, 80}
    assert sum(c.gives_up for c in CASES) == 3
    assert lc.SPIN_GIVE_UP < lc.SPIN <= 65536 and lc.LIVE_DELAY * 16 <= lc.SPIN and lc.LIVE_DELAY <= 256


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_case_reaches_its_branch(case):
    for k, i, w in _outcomes(case):
        if case.gives_up:
            assert w.prefix is None, (k, i)
            assert w.windows == case.windows                    # ... in the window the case names
        else:
            assert w.prefix is not None and (w.windows, w.dist) == (case.windows, case.dist), (k, i)
            assert w.prefix <= lc.MASK
    if case.last_prefix is not None:
        assert _outcomes(case)[-1][2].prefix == case.last_prefix
    # what the entry point takes: raw 40-bit values, amounts whose sum stays below 2^40
    state, value = case.records().seeds()
    assert state.size == value.size == 64 * case.G + 2 * case.G and int(value.max(initial=0)) <= lc.MASK
    assert int(case.amounts().sum()) <= lc.MASK


def test_the_windows_are_where_the_table_says():
    """the rows written out by hand: which groups a walk from group G visits, window by window"""
    def windows(G):
        out, top = [], G - 2
        while top >= 0:
            out.append((top, max(top - lc.WINDOW + 1, 0)))
            top -= lc.WINDOW
        return out
    assert windows(1) == [] and windows(2) == [(0, 0)] and windows(33) == [(31, 0)]
    assert windows(34) == [(32, 1), (0, 0)] and windows(35) == [(33, 2), (1, 0)]
    assert windows(66) == [(64, 33), (32, 1), (0, 0)] and windows(67) == [(65, 34), (33, 2), (1, 0)]
    assert windows(70) == [(68, 37), (36, 5), (4, 0)]
    for c in CASES:
        if not c.gives_up and c.dist == lc.NO_PREFIX:
            assert c.windows == len(windows(c.G)), c.name


@pytest.mark.parametrize("case", OK_CASES, ids=lambda c: c.name)
def test_the_result_tells_which_records_were_read(case):
    """Every record the walk reads moves the sum when it moves, no record it does not read changes anything - whatever state
    or value it takes - and no other choice of prefix record gives the same sum."""
    rec, live = case.records(), case.amounts()
    i = lc.GROUP - 1
    w = lc.walk(rec, i, live)
    for key in rec.keys():
        kind, at = key
        if kind == "agg" and at < lc.GROUP * (case.G - 1) and at % 61:      # (the amounts no walk looks at: a sample)
            continue
        st, v = rec.get(kind, at)
        if key in w.read:
            other = rec.copy()
            other.put(kind, at, st, v ^ 1)
            assert lc.walk(other, i, live).prefix == w.prefix + ((v ^ 1) - v), key
            continue
        if kind == "agg" or at == case.G - 1:      # (records no walk ever looks at: any state, any value)
            states = (lc.MISSING, lc.READY, lc.STALE, lc.LATER)
        elif kind == "amt":                          # (an amount behind the prefix that ended the walk, or of its group)
            states = (lc.MISSING, lc.READY, lc.STALE, lc.LATER)
        else:                                        # (a prefix record: one that is not ready stays not ready, one behind the end may be anything)
            behind = w.dist != lc.NO_PREFIX and at < min(j for k, j in w.read if k == "pre")
            states = (lc.MISSING, lc.READY, lc.STALE, lc.LATER) if behind else (lc.MISSING, lc.STALE, lc.LATER)
        for s in states:
            other = rec.copy()
            other.put(kind, at, s, (v + 12345) & lc.MASK)
            o = lc.walk(other, i, live)
            assert (o.prefix, o.windows, o.dist) == (w.prefix, w.windows, w.dist), (key, s)
    # any other group's prefix record, with the amounts of the groups between it and me, is a different number
    members = sum(int(x) for x in live[:i]) + sum(rec.get("agg", lc.GROUP * (case.G - 1) + k)[1] for k in range(lc.GROUP) if case.G >= 1)
    used = [j for k, j in w.read if k == "pre"]
    for j in range(case.G - 1):
        if rec.get("pre", j)[0] == lc.MISSING or j in used:
            continue
        alt = members + rec.get("pre", j)[1] + sum(rec.get("amt", x)[1] for x in range(j + 1, case.G - 1))
        assert alt != w.prefix, j
    # ... and so is the sum of all the groups' amounts where a prefix was used, and group G - 1 by its records
    if used:
        assert members + sum(rec.get("amt", x)[1] for x in range(case.G - 1)) != w.prefix
    if case.G >= 1:
        assert w.prefix - sum(rec.get("agg", lc.GROUP * (case.G - 1) + k)[1] for k in range(lc.GROUP)) + rec.get("amt", case.G - 1)[1] != w.prefix


@pytest.mark.parametrize("name", list(lc.WRONG), ids=lambda n: n.replace(" ", "_"))
def test_every_wrong_rule_changes_a_case(name):
    """Each way of getting the walk wrong gives, on the cases that name it, another sum (or gives up where the right walk does
    not, or the other way round) - for every launched size and workgroup."""
    pinned = [c for c in CASES if name in c.pins]
    assert pinned, name
    for case in pinned:
        for (k, i, right), (_, _, wrong) in zip(_outcomes(case), _outcomes(case, lc.WRONG[name])):
            assert right.prefix != wrong.prefix, (case.name, k, i)


def test_every_case_names_only_rules_that_exist():
    for c in CASES:
        assert set(c.pins) <= set(lc.WRONG), c.name


def test_live_grids():
    assert set(lc.LIVE_SIZES) >= {1, 2, 63, 64, 65, 127, 128, 129, 2112, 2176, 2177, 4096, 4097, 100_000}
    for n in lc.LIVE_SIZES:
        a = lc.live_amounts(n)
        assert a.size == n and int(a.sum()) <= lc.MASK
        assert int(a.max()) >= (1 << 32) - 1 and (n < 64 or np.count_nonzero(a == 0) > 0)
        assert n < 64 or not np.array_equal(a, lc.live_amounts(n, seed=1))
        pre, agg, grp = lc.live_expected(a, 5)
        assert pre[0] == 0 and int(pre[-1]) + int(a[-1]) == int(a.sum())
        assert agg.size == n and grp.size == 2 * ((n + 63) // 64)
        assert int(grp[-1]) == (5 << 40) | int(a.sum())                                  # the last (partial) group's inclusive prefix
        assert int(grp[-2]) == (5 << 40) | int(a[(n - 1) // 64 * 64:].sum())            # ... and its amount
        d = lc.live_delays(n)
        assert d.size == n and int(d.max(initial=0)) <= lc.LIVE_DELAY and np.count_nonzero(d) == n // 7
    # the 35th group (workgroups 2176 ..) is the first whose walk has a second window; the largest grid has walks of many
    assert (2176 // 64) - 2 == lc.WINDOW and 2177 in lc.LIVE_SIZES and max(lc.LIVE_SIZES) // 64 - 2 >= 2 * lc.WINDOW
