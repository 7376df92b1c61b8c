"""CPU: the path table of tests/path_cases.py is sound before it reaches a GPU - the library names its paths, every path id is
the expected path of at least one case, and no case's reference is trivial."""
import numpy as np
import pytest

from inverted_index_2_amd import _lib
from inverted_index_2_amd.engine import path_names
from tests import path_cases as pc


def test_path_names_are_unique_and_end_with_null():
    lib = _lib.load()
    names = path_names()
    assert len(names) >= 40 and all(names) and len(set(names)) == len(names)
    assert lib.ii2_path_name(len(names)) is None and lib.ii2_path_name(0xFFFFFFFF) is None
    assert lib.ii2_path_name(0) == names[0].encode()
    assert lib.ii2_ctx_paths(None, None, 0) == -1          # II2_EINVAL: the counters belong to a context


def test_every_path_has_a_case():
    names = set(path_names())
    expected = set()
    for case in pc.CASES:
        expected |= {k for k, v in case.expect.items() if v} | {k for k, v in (case.big or {}).items() if v}
    assert expected <= names, sorted(expected - names)                     # no case expects a path the library does not know
    assert len(pc.UNREACHABLE) <= 3 and set(pc.UNREACHABLE) <= names and all(pc.UNREACHABLE.values())
    assert not (expected & set(pc.UNREACHABLE)), "a path listed as unreachable has a case"
    assert names - expected - set(pc.UNREACHABLE) == set()


def test_cases_are_well_formed():
    for case in pc.CASES:
        assert set(case.options) <= set(pc.DEFAULTS), case.name
        assert all(isinstance(v, int) and v > 0 for v in case.expect.values()), case.name
        assert case.cap in (None, "exact") and case.layouts()[:2] == ["one", "two"], case.name
    # the large-dictionary dimension: every case of these entry points runs on the 65537-list segment too, and one ii2_intersect case
    for case in pc.CASES:
        if case.call[0] in ("intersect_ranges", "andnot", "batch", "gbatch") or "or.many" in case.expect:
            assert case.big is not None, case.name
    assert any(case.call[0] == "intersect" and case.big and case.big.get("span.fetch") for case in pc.CASES)


def test_layouts_name_the_same_lists():
    lists = tuple(np.arange(i, i + 3, dtype=np.uint32) for i in range(7))
    for kind in pc.LAYOUTS:
        lay = pc.Layout(kind, lists)
        for i, (s, j) in enumerate(lay.at):
            assert lay.segments[s][j] is lists[i]
        for a, b in [(0, 7), (1, 2), (2, 5), (3, 3), (0, 1), (1, 6)]:
            named = sorted(id(lay.segments[s][j]) for s, lo, hi in lay.ranges([(a, b)]) for j in range(lo, hi))
            assert named == sorted(id(l) for l in lists[a:b]), (kind, a, b)
        for s in range(len(lay.segments)):
            off, vals = lay.flat(s)
            assert off.size == lay.n_lists[s] + 1 and int(off[-1]) == vals.size
    assert pc.Layout("big", lists).n_lists == [pc.BIG_LISTS]


@pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
def test_reference_is_not_trivial(case):
    lists = case.lists()
    for l in lists:
        assert l.dtype == np.uint32 and l.size and np.all(l[1:] > l[:-1])              # a valid posting list
    plain = pc.reference(case, lists)
    for (op, operands), res in zip(pc.operands(case, lists), plain):
        assert res.dtype == np.uint64 and res.size > 0
        if op == "or":
            assert res.size > max(o.size for o in operands)
        elif case.degenerate is None:
            assert res.size < min(o.size for o in operands)
        else:
            assert min(o.size for o in operands) == 1, case.degenerate
    if case.tomb:
        removed = pc.removed_ids(case, lists)
        for res, left in zip(plain, pc.reference(case, lists, removed)):
            assert 0 < left.size < res.size
