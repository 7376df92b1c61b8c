"""CPU: every case of tests/atleast_cases.py has a non-trivial numpy reference - a threshold between OR and AND gives a result
strictly between theirs, and every tombstone set and exclusion removes an id and leaves one - so that a kernel that ignores the
threshold, the exclusion or the tombstones cannot pass tests/test_gpu_atleast_ranges.py."""
import numpy as np
import pytest

from tests import atleast_cases as ac


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_reference_is_not_trivial(case):
    n1 = case.n_counted
    want = ac.reference(case)
    assert all(int(l.max()) < 1 << 18 for l in case.lists if l.size)
    assert all(np.all(np.diff(l.astype(np.int64)) > 0) for l in case.lists)
    assert sum(l.size for g in case.groups + case.exclude for l in (case.lists[i] for i in g)) <= 8192
    if case.m > n1:
        assert want.size == 0
        return
    if 1 < case.m < n1:
        lower, upper = ac.reference(case, m=n1, exclude=False), ac.reference(case, m=1, exclude=False)
        mine = ac.reference(case, exclude=False)
        assert lower.size < mine.size < upper.size and mine.size
    if case.exclude:
        assert 0 < want.size < ac.reference(case, exclude=False).size
    assert case.removed
    assert 0 < ac.reference(case, tomb=True).size < want.size


def test_the_table_holds_the_cases_the_forms_need():
    names = set(ac.BY_NAME)
    assert {"basic_m1", "basic_m2", "basic_m3", "run_at_end", "exclusion", "empty_groups_m3", "empty_groups_m4", "small_capacity", "seams",
            "saturation_m2", "saturation_m3", "late_groups", "excluded_alone", "many_lists", "many_groups", "multi_block"} <= names
    forms = {ac.expected_form(c) for c in ac.CASES}
    assert forms == {ac.NONE, ac.SMALL, ac.COUNT, ac.AND, ac.OR}
    # a group of more than II2_MAX_LISTS lists, more than 64 groups, 64 lists exactly
    assert len(ac.BY_NAME["many_lists"].groups[0]) == 300 and ac.BY_NAME["many_groups"].m == 255
    c = ac.BY_NAME["small_capacity"]
    assert len(c.lists) == 64 and len(c.groups) == 40 and c.m == 20 and ac.expected_form(c) == ac.SMALL
    # the id in both lists of one group counts once
    assert 300 in ac.reference(ac.BY_NAME["basic_m1"]) and 300 not in ac.reference(ac.BY_NAME["basic_m2"])
    # n' = 3 of 5 groups
    assert ac.BY_NAME["empty_groups_m3"].n_counted == 3 and len(ac.BY_NAME["empty_groups_m3"].groups) == 5
    assert ac.expected_form(ac.BY_NAME["empty_groups_m4"]) == ac.NONE
    # the late-group case: the two largest groups are late, 100000 lies in them alone
    c = ac.BY_NAME["late_groups"]
    sizes = [c.ids(g).size for g in c.groups]
    assert sizes == sorted(sizes) and len(set(sizes)) == 4 and c.m == 3
    assert [100000 in c.ids(g) for g in c.groups] == [False, False, True, True]
    assert [20 in c.ids(g) for g in c.groups] == [False, True, True, True] and 20 in ac.reference(c)
