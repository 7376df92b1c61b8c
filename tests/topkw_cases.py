"""The case table of ii2_topk_weighted_ranges ("the k docs of the highest weighted score"), shared by tests/test_topkw_cpu.py (the
table itself holds: every W' <= 255, the new cases are what they say) and tests/test_gpu_topk_weighted.py (every case x every k x
every min_score, one window and many, one segment and two, with and without tombstones).  Pure numpy.  A weighted case is a
tests/atleast_cases Case - lists, groups as lists of list indices, excluded groups, removed ids - plus one weight per group and the
values of k and min_score it runs at.  Every entry of tests/topk_cases.CASES appears under three weight vectors: all ones,
1 << (i % 3) (an add that skips the low planes), and 3, 5, 7, ... cycled (carries through several planes); where the weights of the
groups with postings would sum past 255 the vector is capped - from the last group back, weights become 1 - so that they do not.
reference() is np.unique per group, np.add.at of the weights, the drops, one lexsort."""
from dataclasses import dataclass
from typing import List

import numpy as np

from tests import topk_cases as tc
from tests.atleast_cases import A, EMPTY, Case

N_SCORES = 256
MAX_SCORE = 255
ODD = (3, 5, 7, 9, 11, 13)


@dataclass
class WCase:
    case: Case
    tag: str                     # which weight vector
    weights: List[int]           # one per group of case.groups
    ks: List[int]
    min_scores: List[int]

    @property
    def name(self):
        return f"{self.case.name}-{self.tag}"

    @property
    def counted(self):
        """indices of the groups that have postings"""
        return [g for g, idx in enumerate(self.case.groups) if self.case.ids(idx).size]

    @property
    def total_weight(self):
        return sum(self.weights[g] for g in self.counted)

    @property
    def postings(self):
        """postings of each counted group: the sizes of its lists, summed"""
        return [sum(int(self.case.lists[i].size) for i in self.case.groups[g]) for g in self.counted]


def scores_of(case: Case, weights, min_score=1, tomb=False):
    """(ids ascending, their scores) of the eligible docs"""
    per_group = [case.ids(g) for g in case.groups]
    ids = np.unique(np.concatenate(per_group + [EMPTY])).astype(np.uint32)
    score = np.zeros(ids.size, np.int64)
    for g, w in zip(per_group, weights):
        np.add.at(score, np.searchsorted(ids, g), int(w))
    drop = [case.lists[i] for g in case.exclude for i in g]
    if tomb:
        drop.append(np.asarray(case.removed, np.uint32))
    keep = (score >= min_score) & ~np.isin(ids, np.concatenate(drop + [EMPTY]))
    return ids[keep], score[keep].astype(np.uint32)


def reference(case: Case, weights, k, min_score=1, tomb=False):
    """(ids, scores, hist): per-group np.unique, the scores by np.add.at with the weights, score < min_score, the excluded and the
    removed ids dropped, np.lexsort((ids, -scores))[:k]"""
    ids, scores = scores_of(case, weights, min_score, tomb)
    hist = np.bincount(scores, minlength=N_SCORES).astype(np.uint64)
    order = np.lexsort((ids, -scores.astype(np.int64)))[:k]
    return ids[order], scores[order], hist


def late_rule(weights, postings, min_score):
    """the late flags of the counted groups (include/ii2.h): in descending order of postings, ties by index, the longest prefix
    whose weights sum to at most min_score - 1; nothing when min_score is above the total"""
    late = [0] * len(weights)
    if min_score > sum(weights):
        return late
    acc = 0
    for g in sorted(range(len(weights)), key=lambda g: (-postings[g], g)):
        if acc + weights[g] > min_score - 1:
            break
        acc += weights[g]
        late[g] = 1
    return late


def capped(case: Case, weights):
    """weights with W' <= 255: from the last group back, a weight becomes 1 until the counted groups' sum fits"""
    weights = list(weights)
    counted = [g for g, idx in enumerate(case.groups) if case.ids(idx).size]
    for g in reversed(counted):
        if sum(weights[c] for c in counted) <= MAX_SCORE:
            break
        weights[g] = 1
    return weights


def mid_score(case: Case, weights):
    """a score in the middle of those the case's docs take (1 when it has none)"""
    _, scores = scores_of(case, weights)
    distinct = np.unique(scores)
    return int(distinct[distinct.size // 2]) if distinct.size else 1


def auto_ks(case: Case, weights, min_scores, limit=5):
    """at most `limit` + 2 values of k: 1, a cut inside a class where one holds two docs, a whole class, every eligible doc, one more"""
    ks = {1}
    for m in min_scores:
        _, _, hist = reference(case, weights, 0, m)
        total, above = int(hist.sum()), 0
        for s in range(N_SCORES - 1, -1, -1):
            h = int(hist[s])
            if h >= 2 and len(ks) < limit:
                ks.add(above + 1)
            if h and len(ks) < limit:
                ks.add(above + h)
            above += h
        ks |= {max(total, 1), total + 1}
    return sorted(ks)[:limit + 2]


def _vectors(case: Case):
    n = len(case.groups)
    out, seen = [], set()
    for tag, w in (("ones", [1] * n), ("pow2", [1 << (i % 3) for i in range(n)]), ("odd", [ODD[i % len(ODD)] for i in range(n)])):
        w = capped(case, w)
        if tuple(w) not in seen:                                   # (a capped vector may have become all ones)
            seen.add(tuple(w))
            out.append((tag, w))
    return out


def _weighted(case: Case, tag, weights, ks=None, min_scores=None):
    t = WCase(case, tag, list(weights), [], [])
    t.min_scores = sorted(set(min_scores if min_scores is not None else [1, mid_score(case, weights), max(t.total_weight, 1)]))
    t.ks = list(ks) if ks is not None else auto_ks(case, weights, t.min_scores)
    return t


# ---- the cases written for the weights -------------------------------------------------------------------------------------------
_COPY = 65536 + 2048             # the second copy of every_score_binary's docs starts behind a summary word and a chunk


def _every_score_binary():
    """8 groups of weights 128 .. 1: doc d in 1 .. 255 lies in the group of weight 2^b iff bit b of d is set, so score(d) = d and
    every score 1 .. 255 is taken once; a copy of the docs, doc d at _COPY + 17 d, crosses chunk seams above the first summary
    word - every score is taken once more"""
    d = np.arange(1, 256, dtype=np.uint32)
    lists = [np.concatenate([d[(d >> b) & 1 == 1], _COPY + 17 * d[(d >> b) & 1 == 1]]).astype(np.uint32) for b in range(7, -1, -1)]
    return Case("every_score_binary", lists, [[g] for g in range(8)], 1, removed=[255, _COPY + 17 * 128])


def _late_stopwords():
    """a stop-word: 6000 ids (every fifth up to 30000: 15 chunks of 2048 docs) of weight 1, and two rare terms of weights 6 and 9 that
    sit in chunks 0, 1, 5 and 7 only - the other chunks hold docs of the late group alone.  23 lies under the rare terms and not under
    the stop-word; 10240 under all three"""
    stop = np.arange(0, 30000, 5, dtype=np.uint32)
    six = np.unique(np.concatenate([np.arange(0, 400, 10), A(23, 2050, 2055, 10240, 14336, 14340, 14341)])).astype(np.uint32)
    nine = np.unique(np.concatenate([np.arange(5, 300, 15), A(23, 2055, 2056, 10240, 14340)])).astype(np.uint32)
    assert six.size < 50 and nine.size < 50 and six.size > nine.size
    return Case("late_stopwords", [stop, six, nine], [[0], [1], [2]], 1, removed=[10240, 5])


NEW = [
    _weighted(_every_score_binary(), "binary", [128, 64, 32, 16, 8, 4, 2, 1], ks=[1, 2, 3, 100, 509, 510, 511], min_scores=[1, 128, 255]),
    # 127 + 1 ripples through seven planes into the eighth (docs of groups 0 and 2), 127 + 127 + 1 fills all eight to exactly 255
    _weighted(Case("full_carry", [A(1, 2, 3, 4, 70000), A(2, 3, 5, 70000), A(3, 4, 5, 6, 70000)], [[0], [1], [2]], 1, removed=[3]),
              "carry", [127, 127, 1], ks=[1, 2, 3, 6, 7, 8], min_scores=[1, 128, 255]),
    _weighted(_late_stopwords(), "stop", [1, 6, 9], ks=[1, 2, 5, 40, 80, 7000], min_scores=[1, 2, 7, 16]),
    # a tie at the cut between docs whose equal scores come from different weight sets: 4 + 1 (docs 10, 3000) against 3 + 2 (docs 9,
    # 2999, 70000); 5000 holds all four weights
    _weighted(Case("tie_mixed_sets", [A(10, 3000, 5000), A(10, 3000, 5000, 6000), A(9, 2999, 5000, 70000), A(9, 2999, 5000, 70000, 70001)],
                   [[0], [1], [2], [3]], 1, removed=[2999]),
              "mixed", [4, 1, 3, 2], ks=[1, 2, 3, 4, 5, 6, 7, 9, 10], min_scores=[1, 5, 10]),
]

CASES = [_weighted(t.case, tag, w) for t in tc.CASES for tag, w in _vectors(t.case)] + NEW
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert all(c.total_weight <= MAX_SCORE for c in CASES)
