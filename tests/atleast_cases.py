"""The case table of ii2_atleast_ranges ("docs in at least m of n groups"), shared by tests/test_atleast_cases_cpu.py (every
reference is non-trivial) and tests/test_gpu_atleast_ranges.py (every case under every form).  Pure numpy: a case is its lists,
its groups as lists of list indices, the threshold and the removed ids; reference() is the plain count over np.unique'd groups.
All ids stay below 2^18 (at most 128 windows of 2048 docs) and a case holds at most a few thousand postings: every kernel of the
counting form runs as one workgroup here.  The wide regimes - several workgroups, a second grid-stride step, the windows of the default
union.many_window_log2, ids up to 0xFFFFFFFF - live in tests/wide_cases.py."""
from dataclasses import dataclass, field
from typing import List, Sequence

import numpy as np

EMPTY = np.empty(0, np.uint32)
MAX_LISTS, SMALL_POSTINGS, SMALL_BLOCKS, SMALL_WORK = 64, 8192, 128, 32768      # the one-launch form's limits (include/ii2.h)
NONE, SMALL, COUNT, AND, OR = range(5)                                            # II2_ATLEAST_*


def A(*ids):
    return np.asarray(ids, np.uint32)


@dataclass
class Case:
    name: str
    lists: List[np.ndarray]
    groups: List[List[int]]                 # required groups: indices into lists (an empty group is allowed)
    m: int
    exclude: List[List[int]] = field(default_factory=list)
    removed: Sequence[int] = ()             # the tombstones of the "with tombstones" run

    def ids(self, group):
        return np.unique(np.concatenate([self.lists[i] for i in group] + [EMPTY])).astype(np.uint32)

    @property
    def n_counted(self):
        return sum(1 for g in self.groups if self.ids(g).size)


def reference(case: Case, m=None, tomb=False, exclude=True):
    """np.unique per group, count per id over the groups, keep count >= m, setdiff1d the excluded lists and removed ids"""
    m = case.m if m is None else m
    per_group = [case.ids(g) for g in case.groups]
    ids, cnt = np.unique(np.concatenate(per_group + [EMPTY]), return_counts=True)
    keep = ids[cnt >= m].astype(np.uint32)
    drop = [case.lists[i] for g in case.exclude for i in g] if exclude else []
    if tomb:
        drop.append(np.asarray(case.removed, np.uint32))
    return np.setdiff1d(keep, np.concatenate(drop + [EMPTY])).astype(np.uint32)


def expected_form(case: Case, handoff=1, small=1):
    """the form the chooser of setop.cpp takes (stats.form)"""
    n1 = case.n_counted
    if not case.groups or case.m > n1:
        return NONE
    req = [case.lists[i] for g in case.groups for i in g if case.lists[i].size]
    lo, hi = min(int(l[0]) for l in req), max(int(l[-1]) for l in req)
    exc = [case.lists[i] for g in case.exclude for i in g if case.lists[i].size and int(case.lists[i][0]) <= hi and int(case.lists[i][-1]) >= lo]
    if case.m == n1 and (handoff or case.m > 255):
        return AND
    if case.m == 1 and not exc and handoff:
        return OR
    counted = req + exc
    postings, blocks = sum(l.size for l in counted), sum((l.size + 255) // 256 for l in counted)
    fits = n1 <= MAX_LISTS and len(counted) <= MAX_LISTS and postings <= SMALL_POSTINGS and blocks <= SMALL_BLOCKS
    if small and fits and (small == 2 or postings * len(counted) <= SMALL_WORK):
        return SMALL
    return COUNT


# ---- the cases -----------------------------------------------------------------------------------------------------------
# three groups of two lists; 300 sits in both lists of group 0 and nowhere else: it must not reach m = 2
_BASIC = [A(1, 5, 9, 20, 300), A(5, 30, 300), A(5, 9, 40), A(9, 50, 77), A(5, 60, 77), A(20, 77, 99)]
_BASIC_GROUPS = [[0, 1], [2, 3], [4, 5]]


def _small_capacity():
    """64 one-posting lists in 40 groups: 100 in 22 groups, 150 in 21 (and twice in two of them), 200 in 19"""
    lists, groups = [], []
    for g in range(40):
        mine = [A(100) if g < 22 else A(150)]
        if g < 24:
            mine.append(A(150) if g < 3 or g >= 22 else A(200))
        groups.append(list(range(len(lists), len(lists) + len(mine))))
        lists += mine
    assert len(lists) == 64
    return Case("small_capacity", lists, groups, 20, removed=[150, 7])


def _many_lists():
    """a group of 300 one-block lists (more than II2_MAX_LISTS) against two short groups"""
    lists = [A(3 * i, 3 * i + 1) for i in range(300)] + [A(0, 3, 7, 500), A(3, 500, 601)]
    return Case("many_lists", lists, [list(range(300)), [300], [301]], 2, removed=[7, 8])


def _many_groups():
    """260 groups, m = 255 (eight planes): 5 in every group, 6 in exactly 255, 7 in exactly 254"""
    lists = [A(*([5] + ([6] if g < 255 else []) + ([7] if g < 254 else []) + [1000 + g])) for g in range(260)]
    return Case("many_groups", lists, [[g] for g in range(260)], 255, removed=[5, 9])


CASES = [
    Case("basic_m1", _BASIC, _BASIC_GROUPS, 1, removed=[9, 12345]),
    Case("basic_m2", _BASIC, _BASIC_GROUPS, 2, removed=[9, 12345]),
    Case("basic_m3", _BASIC + [A(9, 20)], [[0, 1], [2, 3], [4, 5, 6]], 3, removed=[9, 12345]),
    # the ranked array of the one-launch form ends in a run of equal ids
    Case("run_at_end", [A(3, 1000), A(3, 7, 1000), A(1000)], [[0], [1], [2]], 2, removed=[3]),
    # an excluded group removes survivors 5 and 9; list 2 is both required and excluded
    Case("exclusion", _BASIC, _BASIC_GROUPS, 2, exclude=[[2]], removed=[20]),
    Case("two_exclusions", _BASIC + [A(9, 4000)], _BASIC_GROUPS, 2, exclude=[[2], [6]], removed=[20]),
    # n = 5 with two empty required groups - one without a range, one over an empty list: n' = 3
    Case("empty_groups_m3", _BASIC + [EMPTY, A(9, 20)], [[0, 1], [], [2, 3], [6], [4, 5, 7]], 3, removed=[9]),
    Case("empty_groups_m4", _BASIC + [EMPTY], [[0, 1], [], [2, 3], [6], [4, 5]], 4, removed=[5]),
    _small_capacity(),
    # chunk and window seams: one side in exactly m - 1 groups, the other in exactly m; 0 anchors the windows at multiples of 2048
    Case("seams", [A(0, 2047, 2048, 4095, 65535), A(0, 2048, 4096, 65535), A(0, 4095, 65536)], [[0], [1], [2]], 2, removed=[2048]),
    # the other way round, the windows anchored at 32
    Case("seams_shifted", [A(40, 2047, 2079, 65536), A(40, 2047, 2080, 65535, 65536), A(40, 2048, 2080)], [[0], [1], [2]], 2,
         removed=[65536]),
    # B = 2 planes: 10 in 7 of 7 groups (the counter stays at 3), 20 in exactly one, 30 in three
    Case("saturation_m2", [A(10, 20)] + [A(10, 30)] * 3 + [A(10)] * 3, [[g] for g in range(7)], 2, removed=[30]),
    # m = 3: docs in exactly 2, 3, 4 and 6 of 6 groups
    Case("saturation_m3", [A(100, 200, 300, 400), A(100, 200, 300, 400), A(200, 300, 400), A(300, 400), A(400), A(400, 401)],
         [[g] for g in range(6)], 3, removed=[300]),
    # n' = 4, m = 3: groups 2 and 3 (the largest) are late.  100000 lies in both of them only, alone in its 2048-doc chunk (cleared, not
    # added); 30 and 31 the same inside a chunk that early groups touched (added, 2 < 3); 20 in one early and both late groups (kept)
    Case("late_groups", [A(10, 50), A(10, 20, 60), A(10, 20, 30, 31, 100000), A(10, 20, 30, 31, 50, 100000)], [[0], [1], [2], [3]], 3,
         removed=[10]),
    # the excluded id 200000 is alone in a 2048-doc chunk that holds no required id
    Case("excluded_alone", [A(1, 5, 9, 20, 250000), A(5, 9, 40, 250000), A(5, 20, 77), A(9, 200000)], [[0], [1], [2]], 2,
         exclude=[[3]], removed=[20]),
    _many_lists(),
    _many_groups(),
    # a two-block list whose last block is not full (300 = 256 + 44) and friends
    Case("multi_block", [np.arange(0, 600, 2, dtype=np.uint32), np.arange(0, 900, 3, dtype=np.uint32), np.arange(0, 1000, 5, dtype=np.uint32)],
         [[0], [1], [2]], 2, removed=[0, 30]),
    # the same lists spread over groups of two, with an exclusion: more than 32768 postings x lists, so the default takes the counting form
    Case("multi_block_wide", [np.arange((k % 3) * 12, 6000, 4 * (3 + k % 4), dtype=np.uint32) for k in range(12)] + [np.arange(0, 6000, 28, dtype=np.uint32)],
         [[0, 1], [2, 3], [4, 5], [6, 7], [8, 9], [10, 11]], 3, exclude=[[12]], removed=[12, 24, 25]),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
