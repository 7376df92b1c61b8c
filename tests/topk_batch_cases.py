"""The cases of ii2_topk_batch ("many ranked queries in one launch") that tests/topkw_cases.py does not hold: the seams of the batch
kernel (topk_batch.hip) - the capacity of either size class and one posting more, one score shared by every doc of a full stage, 255
score classes in the 1024-thread form, a group whose lists share ids, a doc that is required and excluded, the highest id - shared by
tests/test_topk_batch_cpu.py (the table is sound: every reference is non-trivial, every case takes the form it names) and
tests/test_gpu_topk_batch.py.  Pure numpy but for Laid, which wants a context.  A case is a tests/topkw_cases WCase plus the form
the host planner must pick for it; sizes() restates what the planner counts, form_of() asks the library's plan export."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from tests import topkw_cases as wc
from tests.atleast_cases import A, Case

FORMS = ["empty", "tiny", "small", "single"]                 # II2_TOPK_BATCH_*


@dataclass
class BCase:
    w: wc.WCase
    form: str

    @property
    def name(self):
        return self.w.case.name


def sizes(case: Case):
    """(counted lists, their postings, their blocks, required groups with postings, the postings of those groups): the non-empty lists
    of the required groups, and the non-empty excluded lists whose doc span meets the span of all required lists"""
    if case.name not in _SIZES:
        _SIZES[case.name] = _sizes(case)
    return _SIZES[case.name]


_SIZES = {}                      # by case name (the names of this table and of tests/topkw_cases.py differ)


def _sizes(case: Case):
    req = [case.lists[i] for g in case.groups for i in g if case.lists[i].size]
    if not req:
        return 0, 0, 0, 0, 0
    lo, hi = min(int(l[0]) for l in req), max(int(l[-1]) for l in req)
    exc = [case.lists[i] for g in case.exclude for i in g if case.lists[i].size and int(case.lists[i][0]) <= hi and int(case.lists[i][-1]) >= lo]
    counted = req + exc
    return (len(counted), sum(int(l.size) for l in counted), sum((int(l.size) + 255) // 256 for l in counted), case.n_counted,
            sum(int(l.size) for l in req))


def plan(lib, n_lists, postings, blocks, n_counted, req_postings, k, topk=1, tiny=1):
    """(form name, bound) of ii2_topk_batch_plan"""
    form, bound = C.c_uint32(99), C.c_uint64(99)
    assert lib.ii2_topk_batch_plan(n_lists, postings, blocks, n_counted, req_postings, k, topk, tiny, C.byref(form), C.byref(bound)) == 0
    return FORMS[form.value], bound.value


def form_of(lib, t: wc.WCase, k, min_score, topk=1, tiny=1):
    """(form name, bound) of one query of the case: nothing runs when min_score is above W'"""
    if min_score > t.total_weight:
        return "empty", 0
    return plan(lib, *sizes(t.case), k, topk, tiny)


class Laid:
    """a case's lists in n_segs segments (list i in segment i % n_segs): its groups as the ranges the entry points take"""

    def __init__(self, ctx, case, n_segs):
        self.case = case
        per = [[l for i, l in enumerate(case.lists) if i % n_segs == s] for s in range(n_segs)]
        self.segs = [ctx.encode_lists(p) for p in per]
        self.n_segs = n_segs
        self.groups = [self.ranges(g) for g in case.groups]
        self.exclude = [self.ranges(g) for g in case.exclude]
        self.tomb = ctx.tombstones(np.asarray(case.removed, np.uint32)) if len(case.removed) else None

    def ranges(self, group):
        out = []
        for i in group:
            s, j = self.segs[i % self.n_segs], i // self.n_segs
            if out and out[-1][0] is s and out[-1][2] == j:
                out[-1] = (s, out[-1][1], j + 1)              # consecutive lists of one segment: one range
            else:
                out.append((s, j, j + 1))
        return out


# ---- the seams ------------------------------------------------------------------------------------------------------------------------
FIB = [1, 2, 3, 5, 8, 13, 21, 34]


def _capacity(extra):
    """(a) 64 lists x 128 postings = 8192, the small form's capacity, in 8 groups of 8 lists with weights 1 .. 34: every list a random
    sample of 0 .. 2999, so ~2800 docs of many score classes lie interleaved in id order - every wave of the counting sort holds
    several classes.  (b) extra = 1: list 0 holds one posting more, which no workgroup takes"""
    rng = np.random.default_rng(20250)
    lists = [np.sort(rng.choice(3000, 128, replace=False)).astype(np.uint32) for _ in range(64)]
    if extra:
        lists[0] = np.union1d(lists[0], A(3001)).astype(np.uint32)
    return Case("capacity_8192" if not extra else "capacity_8193", lists, [list(range(8 * g, 8 * g + 8)) for g in range(8)], 1, removed=[int(lists[5][7]), 2999])


def _one_class():
    """(c) one group of 32 lists x 256 ids, list j holding j, j + 32, ...: 8192 distinct docs of one score - the stable order of the
    counting sort crosses all 16 waves"""
    return Case("one_class", [np.arange(j, 8192, 32, dtype=np.uint32) for j in range(32)], [list(range(32))], 1, removed=[0, 4097, 8191])


def _binary_padded():
    """(d) every_score_binary - 255 score classes, each taken twice, in exactly 2048 postings - with an excluded list of ten ids that no
    doc has inside its span: 2058 postings, so the 255 classes run in the 1024-thread form"""
    base = wc.BY_NAME["every_score_binary-binary"].case
    pad = np.arange(300, 310, dtype=np.uint32)
    assert not np.isin(pad, np.concatenate(base.lists)).any()
    return Case("binary_padded", list(base.lists) + [pad], base.groups, 1, exclude=[[8]], removed=base.removed)


def _tiny(extra):
    """(g) the tiny form's capacity: 32 lists x 64 postings = 2048 in 32 blocks, four groups of eight lists; extra = 1: one more list
    of one posting in a fifth group - 2049 postings in 33 blocks, the 1024-thread form"""
    rng = np.random.default_rng(77)
    lists = [np.sort(rng.choice(1500, 64, replace=False)).astype(np.uint32) for _ in range(32)]
    groups = [list(range(8 * g, 8 * g + 8)) for g in range(4)]
    if extra:
        lists.append(A(int(lists[0][3])))
        groups.append([32])
    return Case("tiny_2048" if not extra else "tiny_2049", lists, groups, 1, removed=[int(lists[2][9])])


def _case(case, weights, ks, min_scores, form):
    return BCase(wc.WCase(case, "seam", list(weights), list(ks), list(min_scores)), form)


def _eligible(case, weights, m=1):
    return int(wc.reference(case, weights, 0, m)[2].sum())


_CAP, _ONE = _capacity(0), _one_class()
_E = _eligible(_CAP, FIB)

CASES = [
    _case(_CAP, FIB, [1, 63, 64, 65, 511, 512, 513, _E - 1, _E, _E + 1], [1, 20], "small"),
    _case(_capacity(1), FIB, [1, 513, _E + 1], [1, 20], "single"),
    _case(_ONE, [7], [1, 512, 513, 8191, 8192, 8193], [1, 7], "small"),
    _case(_binary_padded(), [128, 64, 32, 16, 8, 4, 2, 1], [1, 2, 3, 100, 509, 510, 511], [1, 128, 255], "small"),
    # (e) 2, 3 and 10 lie in both lists of group 0, weight 7: it is added once - 3 scores 7 + 2, not 14 + 2
    _case(Case("shared_ids", [A(1, 2, 3, 10), A(2, 3, 4, 10), A(3, 4, 5)], [[0, 1], [2]], 1, removed=[4]), [7, 2], [1, 2, 5, 6], [1, 7, 9], "tiny"),
    # (f) 3 and 10 are required and excluded; 99 and 0 are excluded alone
    _case(Case("required_and_excluded", [A(1, 2, 3, 10), A(2, 3, 4, 10), A(3, 4, 5), A(0, 3, 10, 99)], [[0, 1], [2]], 1, exclude=[[3]], removed=[4]),
          [7, 2], [1, 2, 4, 5], [1, 7, 9], "tiny"),
    _case(_tiny(0), [1, 2, 4, 8], [1, 10, 700, 1400], [1, 6, 15], "tiny"),
    _case(_tiny(1), [1, 2, 4, 8, 16], [1, 10, 700, 1400], [1, 6, 17], "small"),
    # (h) the highest id there is
    _case(Case("highest_id", [A(0, 5, 0xFFFFFFFE, 0xFFFFFFFF), A(5, 0xFFFFFFFF), A(0xFFFFFFFE)], [[0], [1]], 1, exclude=[[2]], removed=[5]),
          [3, 4], [1, 2, 3, 4], [1, 4, 7], "tiny"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
assert not set(BY_NAME) & {t.case.name for t in wc.CASES}           # (the GPU test caches segments and sizes by case name)
