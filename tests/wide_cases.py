"""The wide cases of the threshold and ranked queries (ii2_atleast_ranges' counting form, ii2_topk_ranges, ii2_topk_weighted_ranges):
the regimes that tests/atleast_cases.py, tests/topk_cases.py and tests/topkw_cases.py never reach because their ids stay below 2^18 -
more than one workgroup, a ragged last workgroup, a second grid-stride step, a count table larger than one scan tile, the windows of
the default union.many_window_log2, ids up to 0xFFFFFFFF.  Shared by tests/test_wide_cases_cpu.py (every case reaches the regime it
names, by arithmetic) and tests/test_gpu_wide_counting.py (every case through the three entry points, bit for bit).  Pure numpy: a
case is tests/atleast_cases' Case wrapped as tests/topk_cases' TopCase and tests/topkw_cases' WCase, so ac.reference, tc.reference
and wc.reference are the references, unchanged.  The lists stay tiny - a case holds at most a few thousand postings; the kernels
skip summary words without bits, so a wide span costs memory, not time."""
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import numpy as np

from tests import topk_cases as tc
from tests import topkw_cases as wc
from tests.atleast_cases import Case

# ---- the launch constants of the six kernels, mirrored ---------------------------------------------------------------------------
SW = 65536               # docs per summary word - setop.cpp, um_set_window: p.n_sum = (uint32_t)((docs + 65535) / 65536)
CHUNK = 2048             # docs per summary bit - topk.hip / atleast.hip: wi = (sw * 32u + chunk) * 64u + l, 64 words of 32 docs
WAVES = 4                # waves (summary words) per workgroup - topk.hip / atleast.hip: sw = blockIdx.x * 4u + (threadIdx.x >> 6)
GRID_CUS = 8             # workgroups per CU at most - setop.cpp, topk_count: min((p.n_sum + 3) / 4, cu_count * 8u)
#                          (atleast_count asks for min((p.n_sum + 1 + 3) / 4, cu_count * 8u): one more summary word, for the count)
HIST_CUS = 2             # ... of k_top_hist - setop.cpp, topk_count: launch_top_hist(t, min(grid, cu_count * 2u), ...)
SCAN_TILE = 4096         # entries per scan tile - scan.hip: SCAN_TILE = SCAN_THREADS * SCAN_PER_THREAD = 256 * 16
CUS = 256                # the compute units of an MI355X, what the CPU test does its arithmetic with

COUNTING = {"atleast.handoff": 0, "atleast.small": 0}      # the options that force ii2_atleast_ranges to its counting form


def grid_of(n_sum, cus=CUS, per_cu=GRID_CUS, extra=0):
    """workgroups of a launch over n_sum summary words (extra = 1: the threshold query's launches)"""
    return min((n_sum + extra + WAVES - 1) // WAVES, cus * per_cu)


def steps_of(n_sum, cus=CUS, per_cu=GRID_CUS):
    """grid-stride steps the busiest wave takes"""
    return -(-n_sum // (grid_of(n_sum, cus, per_cu) * WAVES))


def window_span(case: Case):
    """(base, hi) of the required groups with postings: the windows start at base = lo & ~31"""
    spans = [(int(ids[0]), int(ids[-1])) for ids in (case.ids(g) for g in case.groups) if ids.size]
    return min(a for a, _ in spans) & ~31, max(b for _, b in spans)


def n_sum_of(case: Case, window):
    """summary words of the largest window"""
    base, hi = window_span(case)
    return (min(hi - base + 1, window) + SW - 1) // SW


def n_windows_of(case: Case, window):
    base, hi = window_span(case)
    return -(-(hi - base + 1) // window)


def skipped(case: Case, window):
    """{group index: the windows that hold none of its docs} over the groups with postings (setop.cpp: G.hi < wlo || G.lo > whi)"""
    base, _ = window_span(case)
    out = {}
    for g, idx in enumerate(case.groups):
        ids = case.ids(idx)
        if ids.size:
            out[g] = [w for w in range(n_windows_of(case, window)) if int(ids[-1]) < base + w * window or int(ids[0]) > base + (w + 1) * window - 1]
    return out


def word_of(case: Case, ids):
    """the summary word of each id, inside its window when the windows hold a whole number of them"""
    base, _ = window_span(case)
    return (np.asarray(ids, np.int64) - base) // SW


@dataclass
class Wide:
    top: tc.TopCase                              # the ranked query: the case, its values of k and min_match
    weighted: List[wc.WCase]                     # its weighted twins
    atleast: List[Tuple[Case, int]]              # the threshold runs: (case, min_match), forced to the counting form
    regime: Dict[str, object]                    # what the case is meant to reach (tests/test_wide_cases_cpu.py proves it)
    named: Dict[str, np.ndarray] = field(default_factory=dict)      # the docs the regime speaks of

    @property
    def name(self):
        return self.top.name

    @property
    def case(self):
        return self.top.case


def _lists(n_groups, docs):
    """docs: (id, bit mask of the groups the doc lies in) pairs -> one sorted list per group"""
    out = [[] for _ in range(n_groups)]
    for d, mask in docs:
        assert 0 < mask < (1 << n_groups) and 0 <= d <= 0xFFFFFFFF
        for g in range(n_groups):
            if (mask >> g) & 1:
                out[g].append(d)
    return [np.unique(np.asarray(l, np.uint64)).astype(np.uint32) for l in out]


def _u32(ids):
    return np.unique(np.asarray(ids, np.uint64)).astype(np.uint32)


def _largest_group_weight(case: Case, weights):
    """the weight of the group the late rule takes first: most postings, lowest index among equals"""
    counted = [g for g, idx in enumerate(case.groups) if case.ids(idx).size]
    post = {g: sum(int(case.lists[i].size) for i in case.groups[g]) for g in counted}
    return weights[min(counted, key=lambda g: (-post[g], g))]


def _twins(t: tc.TopCase, limit=4):
    """the weighted twins: an odd-weight and a power-of-two vector, capped to W' <= 255, at min_score 1 and at one that makes the
    largest group late"""
    out = []
    n = len(t.case.groups)
    for tag, w in (("odd", [wc.ODD[i % len(wc.ODD)] for i in range(n)]), ("pow2", [1 << (i % 3) for i in range(n)])):
        w = wc.capped(t.case, w)
        ms = [1, _largest_group_weight(t.case, w) + 1]
        x = wc.WCase(t.case, tag, w, [], ms)
        x.ks = wc.auto_ks(t.case, w, ms, limit=limit)
        out.append(x)
    return out


# ---- three_workgroups --------------------------------------------------------------------------------------------------------------
_TW_BASE = 1000000                 # a multiple of 32, not of 2^18
_TW_LO = _TW_BASE + 7              # the first id: not a multiple of 32, so the windows start at lo & ~31


def _three_workgroups():
    """n' = 3 (B = 2), nine summary words from 1000000 on: three workgroups, the last with one busy wave.  Groups 0, 1, 2; group 3
    is excluded.  Class 1: the first and the last id of every word.  Class 2 (groups 0 and 1): nine docs in words 0, 3, 4 and 8.
    Class 3: one doc in word 1 and one in word 7.  The excluded list holds the class-1 doc that ends word 5 and an id that is alone in
    its 2048-doc chunk of word 6."""
    b = _TW_BASE
    edge = [(_TW_LO, 0b001)] + [(b + j * SW, 0b001 << (j % 3)) for j in range(1, 9)] + [(b + (j + 1) * SW - 1, 0b100 >> (j % 3)) for j in range(9)]
    tie = _u32([b + 100, b + 40000, b + 3 * SW + 31, b + 3 * SW + 65000, b + 4 * SW + 32, b + 4 * SW + 2048, b + 8 * SW + 5, b + 8 * SW + 2047,
                b + 8 * SW + 30000])
    top = _u32([b + SW + 4097, b + 7 * SW + 63])
    docs = edge + [(int(d), 0b011) for d in tie] + [(int(d), 0b111) for d in top]
    alone = b + 6 * SW + 20 * CHUNK + 77
    lists = _lists(3, docs) + [_u32([b + 6 * SW - 1, alone])]
    removed = [int(top[0]), int(tie[3]), b + 2 * SW, 999]
    case = Case("three_workgroups", lists, [[0], [1], [2]], 2, exclude=[[3]], removed=removed)
    ks = [1, 2, 2 + 4, 2 + 6 + 2, 2 + 9 + 1, 40]
    t = tc.TopCase(case, ks, [1, 2])
    regime = dict(n_planes=2, window_log2=29, n_windows=1, n_sum=9, workgroups=3, ragged=True, steps=1,
                  tie_words=[0, 3, 4, 8], top_words=[1, 7], alone_word=6,
                  cuts={6: "between the tie class's word-3 and word-4 members", 10: "inside word 8", 12: "one past the tie class"})
    return Wide(t, _twins(t), [(case, 1), (case, 2), (case, 3)], regime, dict(tie=tie, top=top, alone=_u32([alone])))


# ---- two_scan_tiles ----------------------------------------------------------------------------------------------------------------
_ST_PER_CLASS = 5
_ST_SPOTS = (0, 31, 32, 2047, 2048, 40000, 65535)


def _two_scan_tiles():
    """n' = 40 single-list groups (B = 6, windows of 2^27 docs), 128 summary words from 64 on.  Five docs per class s = 1 .. 40, each
    in exactly the groups 0 .. s - 1; doc i of the 200 sits in word i mod 128 (round robin), and two more class-1 docs pin both ends.  With
    k = every doc the count table holds 40 x 128 + 1 = 5121 entries (two scan tiles), with cut_score 9 it holds 4097, with 10 3969."""
    base = 64
    docs, by_class = [(base + 1, 1), (base + 128 * SW - 1, 1)], {}
    for i in range(40 * _ST_PER_CLASS):
        s = i // _ST_PER_CLASS + 1
        d = base + (i % 128) * SW + _ST_SPOTS[i % len(_ST_SPOTS)]
        docs.append((d, (1 << s) - 1))
        by_class.setdefault(s, []).append(d)
    lists = _lists(40, docs)
    removed = [by_class[40][0], by_class[9][1], 70]
    case = Case("two_scan_tiles", lists, [[g] for g in range(40)], 2, removed=removed)
    total = len(docs)
    ks = [31 * _ST_PER_CLASS - 2, 31 * _ST_PER_CLASS + 2, total]          # cut_score 10, cut_score 9, every doc
    t = tc.TopCase(case, ks, [1])
    regime = dict(n_planes=6, window_log2=27, n_windows=1, n_sum=128, workgroups=32, ragged=False, steps=1,
                  tables={ks[0]: (10, 3969), ks[1]: (9, 4097), ks[2]: (1, 5121)})
    return Wide(t, _twins(t, limit=2), [(case, 2), (case, 33)], regime, {f"class{s}": _u32(v) for s, v in by_class.items()})


# ---- hist_stride -------------------------------------------------------------------------------------------------------------------
_MASKS3 = (0b001, 0b011, 0b111, 0b110, 0b100, 0b101, 0b010, 0b011)


def _hist_stride():
    """n' = 3 (B = 2, windows of 2^29 docs), 2^27 + 2 x 65536 docs from 96 on: 2050 summary words, more than the 2048 waves of
    k_top_hist's 2 x CUs workgroups - the waves of words 0 and 1 go on to words 2048 and 2049.  Docs of every score in words 0, 1,
    2046, 2047, 2048 and 2049."""
    base = 96
    docs, by_word = [(base + 3, 0b010)], {}
    for n, j in enumerate((0, 1, 2046, 2047, 2048, 2049)):
        for i, spot in enumerate((40, 41, 2047, 2048, 30000, 30031, 65000, 65535)):
            d = base + j * SW + spot
            docs.append((d, _MASKS3[(i + n) % len(_MASKS3)]))
            by_word.setdefault(j, []).append(d)
    lists = _lists(3, docs)
    removed = [by_word[2048][2], by_word[0][1], 5]
    case = Case("hist_stride", lists, [[0], [1], [2]], 2, removed=removed)
    t = tc.TopCase(case, [], [1, 2])
    t.ks = tc.auto_ks(case, t.min_matches)
    regime = dict(n_planes=2, window_log2=29, n_windows=1, n_sum=2050, workgroups=513, ragged=True, steps=1, hist_steps=2,
                  pairs=[(0, 2048), (1, 2049)])
    return Wide(t, _twins(t), [(case, 1), (case, 2)], regime, {f"word{j}": _u32(v) for j, v in by_word.items()})


# ---- full_stride -------------------------------------------------------------------------------------------------------------------
_FS_WORDS = (0, 1, 4095, 8191, 8192, 8193, 12287, 16383)


def _full_stride():
    """B = 1 (windows of 2^30 docs): just under 2^30 docs from 160 on, 16384 summary words - more than the 8192 waves of 8 x CUs
    workgroups, so every wave of every kernel takes a second step and the waves of words 0, 1, 4095 and 8191 meet docs in both.  The
    ranked query has one required group of three overlapping lists (every score is 1: the rank is the id order), an excluded list
    and removed ids; the threshold query has five groups over the same docs at min_match 1."""
    base = 160
    docs, by_word = [(base + 9, 0b00001)], {}
    for n, j in enumerate(_FS_WORDS):
        for i, spot in enumerate((11, 2047, 2048, 9000, 33333, 65535 - 40 * n)):
            d = base + j * SW + spot
            docs.append((d, (0b00111, 0b00001, 0b01010, 0b10100, 0b00110, 0b11000)[(i + n) % 6]))
            by_word.setdefault(j, []).append(d)
    assert base + 2 ** 30 - 65536 < docs[-1][0] < base + 2 ** 30 - 1
    five = _lists(5, docs)
    three = _lists(3, [(d, ((m | (m >> 3)) & 0b111) or 0b001) for d, m in docs])
    excluded = _u32([by_word[8192][1], by_word[1][0], base + 5000 * SW + 7])
    removed = [by_word[0][2], by_word[8192][3], by_word[16383][0], 3]
    ranked = Case("full_stride", three + [excluded], [[0, 1, 2]], 1, exclude=[[3]], removed=removed)
    n_before = sum(len(by_word[j]) for j in (0, 1, 4095, 8191)) + 1 - 1                   # the docs in front of word 8192, less one excluded
    t = tc.TopCase(ranked, [1, n_before + 3, 45, 60], [1])
    thr = Case("full_stride_five", five + [excluded], [[0], [1], [2], [3], [4]], 1, exclude=[[5]], removed=removed)
    one = wc.WCase(ranked, "one", [1], list(t.ks), [1])
    regime = dict(n_planes=1, window_log2=30, n_windows=1, n_sum=16384, workgroups=2048, ragged=False, steps=2,
                  pairs=[(0, 8192), (1, 8193), (4095, 12287), (8191, 16383)], cut_in_word={n_before + 3: 8192})
    return Wide(t, [one], [(thr, 1), (ranked, 1)], regime, {f"word{j}": _u32(v) for j, v in by_word.items()})


# ---- default_windows ---------------------------------------------------------------------------------------------------------------
_DW = 1 << 28


def _default_windows():
    """n' = 5 (B = 3): ids 0 .. 0xFFFFFFFF in 16 windows of 2^28 docs at the default union.many_window_log2.  Class 2 (groups 0 and
    1) has exactly one doc per window; class 3 (groups 0, 1, 2) the first id of windows 1 .. 15; class 4 (groups 0 .. 3), the highest,
    two docs of the last window; class 1 the last id of windows 0 .. 14, in group 4 (windows 0 and 1: it is confined to them), group 2
    (windows 2 .. 4) or group 3 (windows 5 .. 14: it is confined to 5 .. 15).  The excluded list holds the last id of window 3 and
    the first of window 4; the removed ids lie below 2^29."""
    W = _DW
    tie = [w * W + 1000 + 3 * CHUNK * w + w for w in range(16)]
    docs = [(d, 0b00011) for d in tie]
    docs += [(w * W, 0b00111) for w in range(1, 16)]
    docs += [(w * W - 1, 0b10000 if w <= 2 else 0b00100 if w <= 5 else 0b01000) for w in range(1, 16)]
    top = [15 * W + 5000, 0xFFFFFFFF]
    docs += [(d, 0b01111) for d in top]
    docs += [(0, 0b10000), (64, 0b00100), (W + 70000, 0b10000)]
    lists = _lists(5, docs) + [_u32([4 * W - 1, 4 * W])]
    removed = [W - 1, W, 2 * W - 1, 12345]
    case = Case("default_windows", lists, [[0], [1], [2], [3], [4]], 2, exclude=[[5]], removed=removed)
    n3 = 15 - 1                                                            # class 3 less the excluded first id of window 4
    ks = [1, 2, 2 + n3 + 8, 2 + n3 + 16, 60]
    t = tc.TopCase(case, ks, [1, 2])
    regime = dict(n_planes=3, window_log2=28, n_windows=16, n_sum=4096, workgroups=1024, ragged=False, steps=1,
                  skipped={0: [], 1: [], 2: [], 3: [0, 1, 2, 3, 4], 4: list(range(2, 16))}, excluded_windows=[3, 4],
                  cuts={2 + n3 + 8: "the tie class after its members of windows 0 .. 7"})
    return Wide(t, _twins(t), [(case, 1), (case, 2)], regime, dict(tie=_u32(tie), top=_u32(top)))


CASES = [_three_workgroups(), _two_scan_tiles(), _hist_stride(), _full_stride(), _default_windows()]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
