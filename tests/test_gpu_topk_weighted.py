"""GPU: ii2_topk_weighted_ranges - the k docs of the highest weighted score, with their scores, in rank order - against numpy
(np.unique per group, np.add.at of the weights, the excluded and removed ids dropped, one lexsort), bit-identical: every case of
tests/topkw_cases.py at every k and min_score with one window and with 2048-doc windows, the lists in one segment and in two, with
and without tombstones; the stats; all-one weights against ii2_topk_ranges; topk.late 0 against 1; call hygiene; the scratch left
zero; the error table; the calls that launch nothing."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import atleast_cases as ac
from tests import topk_cases as tc
from tests import topkw_cases as wc
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
OK, EINVAL, ERANGE = 0, -1, -5
DEFAULTS = {"atleast.small": 1, "atleast.handoff": 1, "union.many_window_log2": 30, "union.many": 0, "topk.late": 1}
WINDOWS = [30, 11]
WHO = "ii2_topk_weighted_ranges: "
N_FIELDS = len(_lib.TopkwStats._fields_)


class Options:
    def __init__(self, ctx, kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set_option(k, DEFAULTS[k])


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


@pytest.fixture(scope="module")
def laid(ctx):
    cache = {}

    def get(case, n_segs=1):
        if (case.name, n_segs) not in cache:
            cache[case.name, n_segs] = Laid(ctx, case, n_segs)
        return cache[case.name, n_segs]
    return get


_REF = {}


def ref(t, k, m, tomb):
    """the reference, computed once per (case, weights, k, min_score, tomb) and shared"""
    key = (t.name, k, m, tomb)
    if key not in _REF:
        _REF[key] = wc.reference(t.case, t.weights, k, m, tomb)
    return _REF[key]


def host_cut(ctx, hist, k):
    mx, c, above, n_cut = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert ctx.lib.ii2_topk_cut(np.ascontiguousarray(hist, np.uint64).ctypes.data_as(_lib.u64p), k, C.byref(mx), C.byref(c), C.byref(above), C.byref(n_cut)) == OK
    return mx.value, c.value, n_cut.value


def host_plan(ctx, t, min_score, wlog2):
    """(total_weight, n_planes, window_docs, n_late) of ii2_topkw_plan for the case's counted groups"""
    weights, postings = [t.weights[g] for g in t.counted], t.postings
    n = len(weights)
    late = (C.c_uint8 * max(n, 1))()
    total, planes, win, n_late = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
    assert ctx.lib.ii2_topkw_plan(n, (C.c_uint32 * max(n, 1))(*weights), (C.c_uint64 * max(n, 1))(*postings), min_score, wlog2, C.byref(total),
                                  C.byref(planes), C.byref(win), late, C.byref(n_late)) == OK
    assert list(late)[:n] == wc.late_rule(weights, postings, min_score)
    return total.value, planes.value, win.value, n_late.value


def expected_marks(case, win, emitted):
    """(windows, mark launches): per window the groups whose doc span meets it, both passes when several windows are emitted from"""
    spans = [(int(ids[0]), int(ids[-1])) for ids in (case.ids(g) for g in case.groups) if ids.size]
    base, hi = min(a for a, _ in spans) & ~31, max(b for _, b in spans)
    n_win = -(-(hi - base + 1) // win)
    marks = sum(1 for w in range(n_win) for a, b in spans if b >= base + w * win and a <= base + (w + 1) * win - 1)
    return n_win, marks * (2 if n_win > 1 and emitted else 1)


# ---- every case x every weight vector x every k ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", wc.CASES, ids=lambda t: t.name)
def test_every_case_weighted(ctx, laid, t):
    case = t.case
    W = t.total_weight
    for n_segs in (1, 2):
        L = laid(case, n_segs)
        for wlog2 in WINDOWS:
            for m in t.min_scores:
                total, planes, win, n_late = host_plan(ctx, t, m, wlog2)
                assert (total, planes) == (W, W.bit_length())
                for tomb in ((False, True) if len(case.removed) else (False,)):
                    for k in t.ks:
                        with Options(ctx, {"union.many_window_log2": wlog2}), path_delta(ctx) as took:
                            ids, scores, n, hist, st = ctx.topk_weighted_ranges(L.groups, t.weights, k, m, L.exclude, tomb=L.tomb if tomb else None,
                                                                                stats=True)
                        want_ids, want_scores, want_hist = ref(t, k, m, tomb)
                        what = (t.name, n_segs, wlog2, tomb, m, k)
                        print(*what, "count", n, "eligible", st.n_eligible, "cut", st.cut_score, st.n_cut, "windows", st.n_windows, "marks", st.n_marks,
                              "late", st.n_late)
                        assert took == {}, what
                        assert n == want_ids.size, what
                        assert np.array_equal(ids.download(n), want_ids), what
                        assert np.array_equal(scores.download(n), want_scores), what
                        assert np.array_equal(hist, want_hist), what
                        assert st.n_counted == case.n_counted and st.total_weight == W and st.n_eligible == int(want_hist.sum()), what
                        assert (st.max_score, st.cut_score, st.n_cut) == host_cut(ctx, want_hist, k), what
                        n_win, marks = expected_marks(case, win, n > 0)
                        assert (st.n_planes, st.n_windows, st.n_marks, st.n_late) == (W.bit_length(), n_win, marks, n_late), what
                        if wlog2 == 30:
                            assert n_win == 1 and marks == case.n_counted


# ---- all-one weights are ii2_topk_ranges ------------------------------------------------------------------------------------------------
EQUIV = ["basic_m2", "exclusion", "two_exclusions", "seams", "excluded_alone", "multi_block_wide", "tie_across_seams", "dense_classes", "empty_groups"]


@pytest.mark.parametrize("name", EQUIV)
@pytest.mark.parametrize("wlog2", WINDOWS)
def test_all_one_weights_are_the_unweighted_query(ctx, laid, name, wlog2):
    t = tc.BY_NAME[name]
    L = laid(t.case, 2)
    for tomb in (None, L.tomb):
        for m in t.min_matches:
            for k in t.ks[::2] + [0]:
                with Options(ctx, {"union.many_window_log2": wlog2}):
                    ids, scores, n, hist, st = ctx.topk_ranges(L.groups, k, m, L.exclude, tomb=tomb, stats=True)
                    for weights in ([1] * len(L.groups), None):
                        w_ids, w_scores, w_n, w_hist, w_st = ctx.topk_weighted_ranges(L.groups, weights, k, m, L.exclude, tomb=tomb, stats=True)
                        what = (name, wlog2, tomb is not None, m, k, weights is None)
                        assert w_n == n and np.array_equal(w_ids.download(n), ids.download(n)) and np.array_equal(w_scores.download(n), scores.download(n)), what
                        assert np.array_equal(w_hist, hist), what
                        assert (w_st.n_counted, w_st.n_eligible, w_st.n_cut, w_st.max_score, w_st.cut_score, w_st.n_windows, w_st.n_marks) == \
                               (st.n_counted, st.n_eligible, st.n_cut, st.max_score, st.cut_score, st.n_windows, st.n_marks), what
                        assert w_st.total_weight == t.case.n_counted and w_st.n_planes == st.n_planes and (m > 1 or w_st.n_late == 0), what


# ---- topk.late 0 against 1 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,min_scores", [("late_stopwords-stop", [2, 7, 16]), ("dense_classes-odd", [4, 8]), ("tie_across_seams-odd", [4, 9])])
@pytest.mark.parametrize("wlog2", WINDOWS)
def test_late_mode_changes_nothing_but_the_work(ctx, laid, name, min_scores, wlog2):
    t = wc.BY_NAME[name]
    L = laid(t.case, 1)
    for m in min_scores:
        for tomb in (None, L.tomb):
            for k in t.ks:
                got = {}
                for late in (1, 0):
                    with Options(ctx, {"union.many_window_log2": wlog2, "topk.late": late}):
                        ids, scores, n, hist, st = ctx.topk_weighted_ranges(L.groups, t.weights, k, m, L.exclude, tomb=tomb, stats=True)
                    got[late] = (n, ids.download(n), scores.download(n), hist, st.n_late)
                what = (name, wlog2, m, tomb is not None, k)
                want_ids, want_scores, want_hist = ref(t, k, m, tomb is not None)
                for late in (1, 0):
                    n, ids, scores, hist, _ = got[late]
                    assert n == want_ids.size and np.array_equal(ids, want_ids) and np.array_equal(scores, want_scores) and np.array_equal(hist, want_hist), (what, late)
                assert got[1][4] > 0 and got[0][4] == 0, what
                assert got[1][4] == host_plan(ctx, t, m, wlog2)[3], what


# ---- raw calls ---------------------------------------------------------------------------------------------------------------------------
def raw(ctx, groups, flags, weights, m, k, ids, scores, tomb=None, group_first=None, hist=None, stats=None):
    """(return code, count) of one ii2_topk_weighted_ranges call: flags = None (group_not == NULL) or one byte per group, weights =
    None (group_weight == NULL) or one entry per group"""
    ranges = [r for g in groups for r in g]
    n = len(ranges)
    gf = [0]
    for g in groups:
        gf.append(gf[-1] + len(g))
    gf = group_first if group_first is not None else gf
    c_gf = (C.c_uint64 * len(gf))(*gf)
    c_flags = (C.c_uint8 * max(len(groups), 1))(*flags) if flags is not None else None
    c_weights = (C.c_uint32 * max(len(groups), 1))(*weights) if weights is not None else None
    segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
    first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
    end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
    cnt = C.c_uint64(12345)
    rc = ctx.lib.ii2_topk_weighted_ranges(ctx.h, len(groups), c_gf, c_flags, c_weights, m, k, segs, first, end, tomb.h if tomb else None,
                                          ids.data_ptr() if ids is not None else None, scores.data_ptr() if scores is not None else None,
                                          C.byref(cnt), hist.ctypes.data_as(_lib.u64p) if hist is not None else None,
                                          C.byref(stats) if stats is not None else None)
    return rc, cnt.value


def sentinel_buffer(ctx, n):
    return ctx.empty(n).upload(np.full(n, SENTINEL, np.uint32))


def fields(st):
    return [getattr(st, f[0]) for f in st._fields_]


@pytest.mark.parametrize("name,k,m", [("tie_mixed_sets-mixed", 3, 1), ("dense_classes-odd", 1000, 1), ("tie_across_seams-pow2", 5, 1),
                                      ("every_score_binary-binary", 300, 1), ("late_stopwords-stop", 40, 7)])
@pytest.mark.parametrize("wlog2", WINDOWS)
def test_call_hygiene(ctx, laid, name, k, m, wlog2):
    t = wc.BY_NAME[name]
    L = laid(t.case, 2)
    want_ids, want_scores, want_hist = ref(t, k, m, False)
    n_want = want_ids.size
    with Options(ctx, {"union.many_window_log2": wlog2}):
        # the buffers hold k + 8 entries: nothing behind count is written, in [count, k) or past k
        ids, scores = sentinel_buffer(ctx, k + 8), sentinel_buffer(ctx, k + 8)
        with path_delta(ctx) as took:
            assert raw(ctx, L.groups, None, t.weights, m, k, ids, scores) == (OK, n_want)
        assert took == {}
        got_ids, got_scores = ids.download(), scores.download()
        assert np.array_equal(got_ids[:n_want], want_ids) and np.all(got_ids[n_want:] == SENTINEL)
        assert np.array_equal(got_scores[:n_want], want_scores) and np.all(got_scores[n_want:] == SENTINEL)
        # d_scores == NULL
        ids = sentinel_buffer(ctx, k + 8)
        assert raw(ctx, L.groups, None, t.weights, m, k, ids, None) == (OK, n_want)
        got_ids = ids.download()
        assert np.array_equal(got_ids[:n_want], want_ids) and np.all(got_ids[n_want:] == SENTINEL)
        # k = 0: the histogram and stats only, d_ids may be NULL
        hist = np.full(256, 7, np.uint64)
        st = _lib.TopkwStats()
        assert raw(ctx, L.groups, None, t.weights, m, 0, None, None, hist=hist, stats=st) == (OK, 0)
        assert np.array_equal(hist, want_hist)
        assert (st.n_eligible, st.max_score, st.cut_score, st.n_cut) == (int(want_hist.sum()), 0, 0, 0)
        total, planes, win, n_late = host_plan(ctx, t, m, wlog2)
        assert (st.n_counted, st.total_weight, st.n_planes, st.n_late) == (t.case.n_counted, total, planes, n_late)
        assert st.n_marks == expected_marks(t.case, win, False)[1]


# ---- the scratch is left zero ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(ctx):
    """lists over the cases' id range that share no id with any case"""
    used = np.unique(np.concatenate([l for t in wc.CASES for l in t.case.lists]))
    near = np.asarray([2046, 2049, 4094, 4097, 65534, 65537, 99999, 100001, 131070, 131073, 199999, 200001], np.uint32)
    a = np.setdiff1d(np.union1d(np.arange(2, 1 << 18, 4099, dtype=np.uint32), near), used).astype(np.uint32)
    b = np.setdiff1d(np.arange(11, 30000, 13, dtype=np.uint32), used).astype(np.uint32)
    seg = ctx.encode_lists([a, b])
    return seg, np.union1d(a, b).astype(np.uint32)


COUNTING = {"atleast.handoff": 0, "atleast.small": 0}


@pytest.mark.parametrize("name", ["basic_m2-odd", "seams-pow2", "excluded_alone-odd", "many_lists-pow2", "multi_block_wide-odd", "tie_across_seams-odd",
                                  "dense_classes-pow2", "every_score_binary-binary", "full_carry-carry", "late_stopwords-stop", "tie_mixed_sets-mixed"])
@pytest.mark.parametrize("wlog2", WINDOWS)
def test_scratch_is_left_zero(ctx, laid, probe, name, wlog2):
    t = wc.BY_NAME[name]
    case = t.case
    L = laid(case, 1)
    seg, probe_union = probe
    # a success that emits, a k = 0 call, a call with nothing eligible behind the marks (everything removed by the exclusion), and
    # a call in late mode (min_score above the smallest weight: some group is late wherever the weights allow it)
    everything = [[r for g in L.groups for r in g]]
    late_m = t.min_scores[len(t.min_scores) // 2] if len(t.min_scores) > 2 else t.min_scores[-1]
    runs = [("emit", dict(k=t.ks[len(t.ks) // 2], min_score=1, exclude=L.exclude)), ("k = 0", dict(k=0, min_score=1, exclude=L.exclude)),
            ("none eligible", dict(k=5, min_score=1, exclude=everything)), ("late", dict(k=t.ks[-1], min_score=late_m, exclude=L.exclude))]
    for what, kw in runs:
        with Options(ctx, {"union.many_window_log2": wlog2}):
            ids, scores, n, hist, st = ctx.topk_weighted_ranges(L.groups, t.weights, stats=True, **kw)
        if what == "none eligible":
            assert n == 0 and st.n_eligible == 0 and st.n_marks > 0
        if what == "late" and name == "late_stopwords-stop":
            assert st.n_late == 1 and n > 0
        # a leftover bitmap, plane or summary bit shows up as a ghost id: in the block-wise union over other lists ...
        with Options(ctx, {"union.many": 1, "union.many_window_log2": wlog2}):
            u, n = ctx.union_ranges([(seg, 0, 2)])
        assert np.array_equal(u.download(n), probe_union), (name, what)
        # ... and in the counting form of ii2_atleast_ranges on the same query
        with Options(ctx, dict(COUNTING, **{"union.many_window_log2": wlog2})):
            out, n, ast = ctx.atleast_ranges(L.groups, min(2, case.n_counted), L.exclude, stats=True)
        assert ast.form == ac.COUNT
        assert np.array_equal(out.download(n), ac.reference(case, m=min(2, case.n_counted))), (name, what)


# ---- nothing to do -------------------------------------------------------------------------------------------------------------------
def test_empty_queries_launch_nothing(ctx, laid):
    t = wc.BY_NAME["empty_groups-odd"]                                   # five groups, n' = 3: weights 3, (5), 7, (9), 11 - W' = 21
    L = laid(t.case, 1)
    assert t.weights == [3, 5, 7, 9, 11] and t.total_weight == 21
    for wlog2 in WINDOWS:
        with Options(ctx, {"union.many_window_log2": wlog2}), path_delta(ctx) as took:
            st = _lib.TopkwStats()
            hist = np.full(256, 7, np.uint64)
            assert raw(ctx, L.groups, None, t.weights, 22, 10, None, None, hist=hist, stats=st) == (OK, 0)     # min_score above W': the pointers may be NULL
            assert not hist.any() and fields(st) == [3, 0, 0, 21] + [0] * (N_FIELDS - 4)
            hist[:] = 7
            assert raw(ctx, [], None, None, 1, 10, None, None, group_first=[0], hist=hist, stats=st) == (OK, 0)   # no group
            assert not hist.any() and fields(st) == [0] * N_FIELDS
            assert raw(ctx, [[], []], [0, 1], [4, 0], 1, 10, None, None, stats=st) == (OK, 0)                   # groups without ranges
            assert fields(st) == [0] * N_FIELDS
            assert raw(ctx, [[(L.segs[0], 6, 7)]], [0], [9], 1, 10, None, None, stats=st) == (OK, 0)            # a group over an empty list
            assert fields(st) == [0] * N_FIELDS
        assert took == {}
    # an excluded group without postings is ignored, whatever its weight says
    ids = sentinel_buffer(ctx, 16)
    rc, n = raw(ctx, L.groups + [[(L.segs[0], 6, 7)], []], [0] * 5 + [1, 1], t.weights + [0, 999], 1, 16, ids, None)
    assert rc == OK and np.array_equal(ids.download()[:n], wc.reference(L.case, t.weights, 16, 1)[0])
    # at min_score = W' exactly the call runs
    ids, scores, n, hist, st = ctx.topk_weighted_ranges(L.groups, t.weights, 10, 21, stats=True)
    assert st.n_planes == 5 and n == wc.reference(L.case, t.weights, 10, 21)[0].size


# ---- the error table ----------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(ctx, laid):
    L = laid(tc.BY_NAME["basic_m2"].case, 1)
    seg = L.segs[0]
    G = L.groups
    other = [[(seg, 0, 1)], [(seg, 1, 2)]]
    lists = [ac.A(5, 1000 + g) for g in range(256)]
    wide = ctx.encode_lists(lists)
    many = [[(wide, g, g + 1)] for g in range(256)]
    table = [
        ("min_score 0", dict(groups=G, flags=None, weights=[1, 2, 3], m=0, k=4), EINVAL, "min_score"),
        ("weight 0", dict(groups=G, flags=None, weights=[1, 0, 3], m=1, k=4), EINVAL, "group 1 has weight 0 (drop the group instead)"),
        ("weight 256", dict(groups=G, flags=None, weights=[1, 2, 256], m=1, k=4), ERANGE, "group 2"),
        ("W' = 256 from two groups", dict(groups=other, flags=None, weights=[128, 128], m=1, k=4), ERANGE, "255"),
        ("W' = 256 with a third group excluded", dict(groups=G, flags=[0, 1, 0], weights=[200, 1, 56], m=1, k=4), ERANGE, "255"),
        ("no required group", dict(groups=other, flags=[1, 1], weights=[1, 1], m=1, k=4), EINVAL, ""),
        ("a flag of 2", dict(groups=other, flags=[0, 2], weights=[1, 1], m=1, k=4), EINVAL, ""),
        ("a range that ends before it begins", dict(groups=[[(seg, 2, 1)]], flags=None, weights=[1], m=1, k=4), EINVAL, ""),
        ("a range past the segment's lists", dict(groups=[[(seg, 0, 1)], [(seg, 5, 7)]], flags=[0, 1], weights=None, m=1, k=4), EINVAL, ""),
        ("group_first does not ascend", dict(groups=other, flags=None, weights=[1, 1], m=1, k=4, group_first=[0, 2, 1]), EINVAL, ""),
        ("256 groups with postings", dict(groups=many, flags=None, weights=None, m=1, k=4), ERANGE, "255"),
        ("k above II2_TOPK_MAX", dict(groups=G, flags=None, weights=[1, 2, 3], m=1, k=_lib.II2_TOPK_MAX + 1), ERANGE, "II2_TOPK_MAX"),
    ]
    for wlog2 in WINDOWS:
        for what, kw, code, says in table:
            ids, scores = sentinel_buffer(ctx, 64), sentinel_buffer(ctx, 64)
            st = _lib.TopkwStats(*([7] * N_FIELDS))
            hist = np.full(256, 7, np.uint64)
            with Options(ctx, {"union.many_window_log2": wlog2}), path_delta(ctx) as took:
                rc, n = raw(ctx, ids=ids, scores=scores, hist=hist, stats=st, **kw)
            assert (rc, n) == (code, 12345), what                                           # count untouched
            msg = ctx.lib.ii2_last_error(ctx.h).decode()
            assert msg.startswith(WHO) and says in msg, (what, msg)
            assert np.all(ids.download() == SENTINEL) and np.all(scores.download() == SENTINEL) and took == {}, what
            assert np.all(hist == 7) and fields(st) == [7] * N_FIELDS, what                 # hist and stats untouched
    # a result to write and nowhere to write it
    scores = sentinel_buffer(ctx, 64)
    assert raw(ctx, G, None, [1, 2, 3], 1, 4, None, scores) == (EINVAL, 12345)
    assert ctx.lib.ii2_last_error(ctx.h).decode() == WHO + "output buffer is NULL"
    assert np.all(scores.download() == SENTINEL)
    # an excluded group's weight of 0 or 1000 is ignored; W' = 255 and k = II2_TOPK_MAX are inside the limits
    ids = sentinel_buffer(ctx, 8)
    assert raw(ctx, G, [0, 1, 0], [2, 0, 3], 1, 8, ids, None)[0] == OK and raw(ctx, G, [0, 1, 0], [2, 1000, 3], 1, 8, ids, None)[0] == OK
    ids, scores, n = ctx.topk_weighted_ranges(other, [128, 127], _lib.II2_TOPK_MAX)
    want_ids, want_scores, _ = wc.reference(ac.Case("w255", [L.case.lists[0], L.case.lists[1]], [[0], [1]], 1), [128, 127], _lib.II2_TOPK_MAX)
    assert n == want_ids.size and np.array_equal(ids.download(n), want_ids) and np.array_equal(scores.download(n), want_scores) and want_scores[0] == 255
    ids, scores, n = ctx.topk_weighted_ranges(many[:255], None, _lib.II2_TOPK_MAX)
    assert n == 256 and ids.download(1).tolist() == [5] and scores.download(2).tolist() == [255, 1]
