"""The case table of ii2_topk_ranges ("the k docs in the most groups"), shared by tests/test_topk_cases_cpu.py (every case cuts
inside a class, takes one whole and runs out of docs wherever its scores allow it) and tests/test_gpu_topk_ranges.py (every case x
every k, one window and many, one segment and two, with and without tombstones).  Pure numpy: a case is tests/atleast_cases' Case -
lists, groups as lists of list indices, excluded groups, removed ids - plus the values of k and min_match it runs at.
reference() is the plain count over np.unique'd groups and one lexsort.  It holds every case of atleast_cases.CASES with at most
255 groups that have postings, at min_match 1 and at the case's own m, and the cases written for the ranking below.  All ids stay
below 2^18 except in high_ids (a span of 32 docs), and a case holds at most a few ten thousand postings: every kernel of the ranked
query runs as one workgroup here and its count table fits one scan tile.  The wide regimes - several workgroups, a second grid-stride
step, a table of two scan tiles, the windows of the default union.many_window_log2 - live in tests/wide_cases.py."""
from dataclasses import dataclass
from typing import List

import numpy as np

from tests import atleast_cases as ac
from tests.atleast_cases import A, EMPTY, Case

N_SCORES = 256


@dataclass
class TopCase:
    case: Case
    ks: List[int]
    min_matches: List[int]
    strict: bool = True          # written for the ranking: some k must cut inside a class

    @property
    def name(self):
        return self.case.name


def scores_of(case: Case, min_match=1, tomb=False):
    """(ids ascending, their scores) of the eligible docs"""
    per_group = [case.ids(g) for g in case.groups]
    ids, cnt = np.unique(np.concatenate(per_group + [EMPTY]), return_counts=True)
    drop = [case.lists[i] for g in case.exclude for i in g]
    if tomb:
        drop.append(np.asarray(case.removed, np.uint32))
    keep = (cnt >= min_match) & ~np.isin(ids, np.concatenate(drop + [EMPTY]))
    return ids[keep].astype(np.uint32), cnt[keep].astype(np.uint32)


def reference(case: Case, k, min_match=1, tomb=False):
    """(ids, scores, hist): np.unique per group, np.unique(concat, return_counts) for the scores, drop score < min_match, the
    excluded and the removed ids, np.lexsort((ids, -scores))[:k]"""
    ids, scores = scores_of(case, min_match, tomb)
    hist = np.bincount(scores, minlength=N_SCORES).astype(np.uint64)
    order = np.lexsort((ids, -scores.astype(np.int64)))[:k]
    return ids[order], scores[order], hist


def cut(hist, k):
    """(max_score, cut_score, n_above, n_cut) as include/ii2.h defines them for ii2_topk_cut"""
    hist = np.asarray(hist, np.uint64)
    if k == 0 or not hist.any():
        return 0, 0, 0, 0
    present = np.nonzero(hist)[0]
    suffix = np.cumsum(hist[::-1].astype(object))[::-1]            # suffix[s] = docs of score >= s
    enough = [int(s) for s in present if suffix[s] >= k]
    c = max(enough) if enough else int(present[0])
    above = int(suffix[c]) - int(hist[c])
    return int(present[-1]), c, above, min(int(hist[c]), k - above)


def auto_ks(case: Case, min_matches):
    """at most eight values of k for a case that was not written for the ranking: 1, a whole class, a cut inside a class where
    one holds two docs, every eligible doc, one more"""
    ks = {1}
    for m in min_matches:
        _, _, hist = reference(case, 0, m)
        total, above = int(hist.sum()), 0
        for s in range(N_SCORES - 1, -1, -1):
            h = int(hist[s])
            if h >= 2 and len(ks) < 6:
                ks.add(above + 1)
            if h and len(ks) < 6:
                ks.add(above + h)
            above += h
        ks |= {max(total, 1), total + 1}
    return sorted(ks)


def _from_atleast(c: Case):
    mm = sorted({1, c.m})
    return TopCase(c, auto_ks(c, mm), mm, strict=False)


def _every_score_255():
    """255 groups: doc d in 1 .. 255 lies in groups 0 .. d - 1, docs 1000 .. 1009 in groups 0 .. 199 - class 200 holds 11 docs"""
    lists = [np.concatenate([np.arange(g + 1, 256), np.arange(1000, 1010) if g < 200 else EMPTY]).astype(np.uint32) for g in range(255)]
    return Case("every_score_255", lists, [[g] for g in range(255)], 1, removed=[255, 1000])


_SEAM_CLASS = A(31, 32, 2047, 2048, 65535, 65536, 131071, 131072)
_SEAM_LIST = np.union1d(_SEAM_CLASS, A(0, 200000)).astype(np.uint32)
_HI = 0xFFFFFFE0

NEW = [
    # the cut inside one bitmap word and between two words
    TopCase(Case("tie_in_word", [np.arange(40, dtype=np.uint32), np.arange(40, dtype=np.uint32), A(5, 17)], [[0], [1], [2]], 2, removed=[5, 3]),
            [1, 2, 3, 4, 33, 40, 41], [1, 3]),
    # one class across the lane, chunk, summary word and window seams, two docs of a higher class around it
    TopCase(Case("tie_across_seams", [_SEAM_LIST, _SEAM_LIST, A(0, 200000)], [[0], [1], [2]], 2, removed=[32, 65536]),
            list(range(1, 12)), [1, 2]),
    # multi-block lists; scores 3 / 2 / 1 in 200 / 1400 / 2800 docs; a quota cut in the middle of a class that spans many chunks
    TopCase(Case("dense_classes", [np.arange(0, 6000, 2, dtype=np.uint32), np.arange(0, 6000, 3, dtype=np.uint32), np.arange(0, 6000, 5, dtype=np.uint32)],
                 [[0], [1], [2]], 2, removed=[0, 30, 7, 4001]),
            [1, 200, 201, 1000, 1600, 1601, 4400, 5000], [1, 2]),
    # eight planes, every plane bit pattern; at k = 57 the cut is score 200 with n_cut 2: ids 200 and 1000
    TopCase(_every_score_255(), [1, 55, 57, 66, 67, 300], [1, 200]),
    # the best doc (10) excluded, the second best (20) removed, the excluded id 100000 alone in its chunk; 30 and 31 tie
    TopCase(Case("excluded_and_removed_top", [A(10, 20, 30, 31, 40), A(10, 20, 30, 31), A(10, 20), A(10, 100000)], [[0], [1], [2]], 1,
                 exclude=[[3]], removed=[20]),
            [1, 2, 3, 4, 5], [1, 2]),
    # a small span at the top of the id range (no removed ids: a tombstone bitmap covers every id below its largest)
    TopCase(Case("high_ids", [np.arange(_HI, 1 << 32, dtype=np.uint64).astype(np.uint32), np.arange(_HI, 1 << 32, 2, dtype=np.uint64).astype(np.uint32),
                              A(_HI, 0xFFFFFFFF)], [[0], [1], [2]], 1),
            [1, 2, 3, 10, 16, 17, 32, 33], [1, 2]),
    # required groups without a range and over an empty list (n' = 3), and min_match above n'
    TopCase(Case("empty_groups", ac.BY_NAME["empty_groups_m3"].lists, ac.BY_NAME["empty_groups_m3"].groups, 3, removed=[9]),
            [1, 2, 3, 9, 10, 11], [1, 3, 4]),
]

CASES = [_from_atleast(c) for c in ac.CASES if c.n_counted <= 255] + NEW
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
