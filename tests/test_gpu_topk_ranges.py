"""GPU: ii2_topk_ranges - the k docs that lie in the most groups, with their scores, in rank order - against numpy (np.unique per
group, a count per id, the excluded and removed ids dropped, one lexsort), bit-identical: every case of tests/topk_cases.py at every
k with one window and with 2048-doc windows, the lists in one segment and in two, with and without tombstones; the stats; call
hygiene; the equivalences with ii2_atleast_ranges and ii2_andnot_ranges; the scratch left zero; the error table."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import atleast_cases as ac
from tests import topk_cases as tc
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
OK, EINVAL, ERANGE = 0, -1, -5
DEFAULTS = {"atleast.small": 1, "atleast.handoff": 1, "union.many_window_log2": 30, "union.many": 0}
WINDOWS = [30, 11]


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

    def get(name, n_segs=1):
        if (name, n_segs) not in cache:
            cache[name, n_segs] = Laid(ctx, tc.BY_NAME[name].case, n_segs)
        return cache[name, n_segs]
    return get


_REF = {}


def ref(t, k, m, tomb):
    """the reference, computed once per (case, k, min_match, tomb) and shared"""
    key = (t.name, k, m, tomb)
    if key not in _REF:
        _REF[key] = tc.reference(t.case, k, m, tomb)
    return _REF[key]


def host_cut(ctx, hist, k):
    mx, c, above, n_cut = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert ctx.lib.ii2_topk_cut(np.ascontiguousarray(hist, np.uint64).ctypes.data_as(_lib.u64p), k, C.byref(mx), C.byref(c), C.byref(above), C.byref(n_cut)) == OK
    return mx.value, c.value, above.value, n_cut.value


def window_docs(ctx, n_counted, wlog2):
    planes, win, late = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert ctx.lib.ii2_atleast_plan(n_counted, n_counted, wlog2, C.byref(planes), C.byref(win), C.byref(late)) == OK
    assert planes.value == int(n_counted).bit_length()
    return win.value


def expected_marks(case, win, emitted):
    """(windows, mark launches): per window the groups whose doc span meets it, both passes when several windows are emitted from"""
    spans = [(int(ids[0]), int(ids[-1])) for ids in (case.ids(g) for g in case.groups) if ids.size]
    base, hi = min(a for a, _ in spans) & ~31, max(b for _, b in spans)
    n_win = -(-(hi - base + 1) // win)
    marks = sum(1 for w in range(n_win) for a, b in spans if b >= base + w * win and a <= base + (w + 1) * win - 1)
    return n_win, marks * (2 if n_win > 1 and emitted else 1)


# ---- every case x every k ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", tc.CASES, ids=lambda t: t.name)
def test_every_case_at_every_k(ctx, laid, t):
    case = t.case
    n1 = case.n_counted
    for n_segs in (1, 2):
        L = laid(t.name, n_segs)
        for wlog2 in WINDOWS:
            for tomb in ((False, True) if len(case.removed) else (False,)):
                for m in t.min_matches:
                    for k in t.ks:
                        with Options(ctx, {"union.many_window_log2": wlog2}), path_delta(ctx) as took:
                            ids, scores, n, hist, st = ctx.topk_ranges(L.groups, k, m, L.exclude, tomb=L.tomb if tomb else None, stats=True)
                        want_ids, want_scores, want_hist = ref(t, k, m, tomb)
                        what = (t.name, n_segs, wlog2, tomb, m, k)
                        print(*what, "count", n, "eligible", st.n_eligible, "cut", st.cut_score, st.n_cut, "windows", st.n_windows, "marks", st.n_marks)
                        assert took == {}, what
                        assert n == want_ids.size, what
                        assert np.array_equal(ids.download(n), want_ids), what
                        assert np.array_equal(scores.download(n), want_scores), what
                        assert np.array_equal(hist, want_hist), what
                        assert st.n_counted == n1 and st.n_eligible == int(want_hist.sum()), what
                        if m > n1:
                            assert (st.n_planes, st.n_windows, st.n_marks, st.max_score, st.cut_score, st.n_cut) == (0,) * 6, what
                            continue
                        mx, c, _, n_cut = host_cut(ctx, want_hist, k)
                        assert (st.max_score, st.cut_score, st.n_cut) == (mx, c, n_cut) == tc.cut(want_hist, k)[:2] + (tc.cut(want_hist, k)[3],), what
                        n_win, marks = expected_marks(case, window_docs(ctx, n1, wlog2), n > 0)
                        assert (st.n_planes, st.n_windows, st.n_marks) == (n1.bit_length(), n_win, marks), what
                        if wlog2 == 30:
                            assert n_win == 1 and marks == n1


def test_the_small_windows_are_many():
    """the 2048-doc run is a many-window run for the cases that are about seams"""
    for name in ("tie_across_seams", "seams", "excluded_alone"):
        case = tc.BY_NAME[name].case
        assert expected_marks(case, 2048, True)[0] > 1


# ---- raw calls ---------------------------------------------------------------------------------------------------------------------------
def raw(ctx, groups, flags, m, k, ids, scores, tomb=None, group_first=None, hist=None, stats=None):
    """(return code, count) of one ii2_topk_ranges call: flags = None (group_not == NULL) or one byte per group"""
    ranges = [r for g in groups for r in g]
    n = len(ranges)
    gf = [0]
    for g in groups:
        gf.append(gf[-1] + len(g))
    gf = group_first if group_first is not None else gf
    c_gf = (C.c_uint64 * len(gf))(*gf)
    c_flags = (C.c_uint8 * max(len(groups), 1))(*flags) if flags is not None else None
    segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
    first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
    end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
    cnt = C.c_uint64(12345)
    rc = ctx.lib.ii2_topk_ranges(ctx.h, len(groups), c_gf, c_flags, m, k, segs, first, end, tomb.h if tomb else None,
                                 ids.data_ptr() if ids is not None else None, scores.data_ptr() if scores is not None else None, C.byref(cnt),
                                 hist.ctypes.data_as(_lib.u64p) if hist is not None else None, C.byref(stats) if stats is not None else None)
    return rc, cnt.value


def sentinel_buffer(ctx, n):
    return ctx.empty(n).upload(np.full(n, SENTINEL, np.uint32))


@pytest.mark.parametrize("name,k", [("tie_in_word", 4), ("dense_classes", 1000), ("tie_across_seams", 5), ("every_score_255", 300)])
@pytest.mark.parametrize("wlog2", WINDOWS)
def test_call_hygiene(ctx, laid, name, k, wlog2):
    t = tc.BY_NAME[name]
    L = laid(name, 2)
    want_ids, want_scores, want_hist = ref(t, k, 1, False)
    n_want = want_ids.size
    with Options(ctx, {"union.many_window_log2": wlog2}):
        # the buffers hold k + 8 entries: nothing behind count is written, in [count, k) or past k
        ids, scores = sentinel_buffer(ctx, k + 8), sentinel_buffer(ctx, k + 8)
        with path_delta(ctx) as took:
            assert raw(ctx, L.groups, None, 1, k, ids, scores) == (OK, n_want)
        assert took == {}
        got_ids, got_scores = ids.download(), scores.download()
        assert np.array_equal(got_ids[:n_want], want_ids) and np.all(got_ids[n_want:] == SENTINEL)
        assert np.array_equal(got_scores[:n_want], want_scores) and np.all(got_scores[n_want:] == SENTINEL)
        # d_scores == NULL
        ids = sentinel_buffer(ctx, k + 8)
        assert raw(ctx, L.groups, None, 1, k, ids, None) == (OK, n_want)
        got_ids = ids.download()
        assert np.array_equal(got_ids[:n_want], want_ids) and np.all(got_ids[n_want:] == SENTINEL)
        # k = 0: the histogram and stats only, d_ids may be NULL
        hist = np.full(256, 7, np.uint64)
        st = _lib.TopkStats()
        assert raw(ctx, L.groups, None, 1, 0, None, None, hist=hist, stats=st) == (OK, 0)
        assert np.array_equal(hist, want_hist)
        assert (st.n_eligible, st.max_score, st.cut_score, st.n_cut) == (int(want_hist.sum()), 0, 0, 0)
        assert st.n_counted == t.case.n_counted and st.n_planes == t.case.n_counted.bit_length()
        assert st.n_marks == expected_marks(t.case, window_docs(ctx, t.case.n_counted, wlog2), False)[1]


# ---- equivalences -----------------------------------------------------------------------------------------------------------------
EQUIV = ["basic_m2", "exclusion", "two_exclusions", "seams", "excluded_alone", "multi_block_wide", "tie_across_seams", "dense_classes", "empty_groups"]


@pytest.mark.parametrize("name", EQUIV)
@pytest.mark.parametrize("wlog2", WINDOWS)
def test_equivalences(ctx, laid, name, wlog2):
    t = tc.BY_NAME[name]
    L = laid(name, 2)
    case = t.case
    n1 = case.n_counted
    k = int(tc.reference(case, 0, 1)[2].sum()) + 3
    nonempty = [g for g, idx in zip(L.groups, case.groups) if case.ids(idx).size]
    for tomb in (None, L.tomb):
        with Options(ctx, {"union.many_window_log2": wlog2}):
            # k >= eligible: the ids, sorted, are ii2_atleast_ranges' at the same min_match
            for m in sorted({1, case.m, n1}):
                ids, scores, n = ctx.topk_ranges(L.groups, k, m, L.exclude, tomb=tomb)
                out, n_at = ctx.atleast_ranges(L.groups, m, L.exclude, tomb=tomb)
                assert n == n_at and np.array_equal(np.sort(ids.download(n)), out.download(n_at)), (name, m)
            # the ids of score n' are ii2_andnot_ranges' over the groups that have postings (ascending: one class)
            ids, scores, n = ctx.topk_ranges(L.groups, k, 1, L.exclude, tomb=tomb)
            got_ids, got_scores = ids.download(n), scores.download(n)
            out, n_and = ctx.andnot_ranges(nonempty, L.exclude, tomb=tomb)
            assert np.array_equal(got_ids[got_scores == n1], out.download(n_and)), name


# ---- the scratch is left zero ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(ctx):
    """lists over the cases' id range that share no id with any case"""
    used = np.unique(np.concatenate([l for t in tc.CASES for l in t.case.lists]))
    near = np.asarray([2046, 2049, 4094, 4097, 65534, 65537, 99999, 100001, 131070, 131073, 199999, 200001], np.uint32)
    a = np.setdiff1d(np.union1d(np.arange(2, 1 << 18, 4099, dtype=np.uint32), near), used).astype(np.uint32)
    b = np.setdiff1d(np.arange(11, 7000, 13, dtype=np.uint32), used).astype(np.uint32)
    seg = ctx.encode_lists([a, b])
    return seg, np.union1d(a, b).astype(np.uint32)


COUNTING = {"atleast.handoff": 0, "atleast.small": 0}


@pytest.mark.parametrize("name", ["basic_m2", "seams", "excluded_alone", "many_lists", "multi_block_wide", "tie_across_seams", "dense_classes",
                                  "every_score_255", "excluded_and_removed_top"])
@pytest.mark.parametrize("wlog2", WINDOWS)
def test_scratch_is_left_zero(ctx, laid, probe, name, wlog2):
    t = tc.BY_NAME[name]
    L = laid(name, 1)
    case = t.case
    seg, probe_union = probe
    # a success that emits, a k = 0 call, and a call with nothing eligible behind the marks (everything removed by the exclusion)
    everything = [[r for g in L.groups for r in g]]
    runs = [("emit", dict(k=t.ks[len(t.ks) // 2], exclude=L.exclude)), ("k = 0", dict(k=0, exclude=L.exclude)), ("none eligible", dict(k=5, exclude=everything))]
    for what, kw in runs:
        with Options(ctx, {"union.many_window_log2": wlog2}):
            ids, scores, n, hist, st = ctx.topk_ranges(L.groups, min_match=1, stats=True, **kw)
        if what == "none eligible":
            assert n == 0 and st.n_eligible == 0 and st.n_marks > 0
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
    L = laid("empty_groups", 1)
    for wlog2 in WINDOWS:
        with Options(ctx, {"union.many_window_log2": wlog2}), path_delta(ctx) as took:
            st = _lib.TopkStats()
            hist = np.full(256, 7, np.uint64)
            assert raw(ctx, L.groups, None, 4, 10, None, None, hist=hist, stats=st) == (OK, 0)      # min_match above n' = 3: the pointers may be NULL
            assert not hist.any() and [getattr(st, f[0]) for f in st._fields_] == [3] + [0] * 8
            hist[:] = 7
            assert raw(ctx, [], None, 1, 10, None, None, group_first=[0], hist=hist, stats=st) == (OK, 0)   # no group
            assert not hist.any() and [getattr(st, f[0]) for f in st._fields_] == [0] * 9
            assert raw(ctx, [[], []], [0, 1], 1, 10, None, None, stats=st) == (OK, 0)                       # groups without ranges
            assert raw(ctx, [[(L.segs[0], 6, 7)]], [0], 1, 10, None, None, stats=st) == (OK, 0)             # a group over an empty list
        assert took == {}
    # an excluded group without postings is ignored
    ids = sentinel_buffer(ctx, 16)
    rc, n = raw(ctx, L.groups + [[(L.segs[0], 6, 7)], []], [0] * 5 + [1, 1], 1, 16, ids, None)
    assert rc == OK and np.array_equal(ids.download()[:n], tc.reference(L.case, 16, 1)[0])


# ---- the error table ----------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(ctx, laid):
    L = laid("basic_m2", 1)
    seg = L.segs[0]
    G = L.groups
    other = [[(seg, 0, 1)], [(seg, 1, 2)]]
    lists = [ac.A(5, 1000 + g) for g in range(256)]
    wide = ctx.encode_lists(lists)
    many = [[(wide, g, g + 1)] for g in range(256)]
    table = [
        ("min_match 0", dict(groups=G, flags=None, m=0, k=4), EINVAL),
        ("no required group", dict(groups=other, flags=[1, 1], m=1, k=4), EINVAL),
        ("a flag of 2", dict(groups=other, flags=[0, 2], m=1, k=4), EINVAL),
        ("a range that ends before it begins", dict(groups=[[(seg, 2, 1)]], flags=None, m=1, k=4), EINVAL),
        ("a range past the segment's lists", dict(groups=[[(seg, 0, 1)], [(seg, 5, 7)]], flags=[0, 1], m=1, k=4), EINVAL),
        ("group_first does not ascend", dict(groups=other, flags=None, m=1, k=4, group_first=[0, 2, 1]), EINVAL),
        ("256 groups with postings", dict(groups=many, flags=None, m=1, k=4), ERANGE),
        ("k above II2_TOPK_MAX", dict(groups=G, flags=None, m=1, k=_lib.II2_TOPK_MAX + 1), ERANGE),
    ]
    for wlog2 in WINDOWS:
        for what, kw, code in table:
            ids, scores = sentinel_buffer(ctx, 64), sentinel_buffer(ctx, 64)
            st = _lib.TopkStats(*([7] * 9))
            hist = np.full(256, 7, np.uint64)
            with Options(ctx, {"union.many_window_log2": wlog2}), path_delta(ctx) as took:
                rc, n = raw(ctx, ids=ids, scores=scores, hist=hist, stats=st, **kw)
            assert (rc, n) == (code, 12345), what                                           # count untouched
            assert ctx.lib.ii2_last_error(ctx.h).decode().startswith("ii2_topk_ranges: "), what
            assert np.all(ids.download() == SENTINEL) and np.all(scores.download() == SENTINEL) and took == {}, what
            assert np.all(hist == 7) and [getattr(st, f[0]) for f in st._fields_] == [7] * 9, what   # hist and stats untouched
    # a result to write and nowhere to write it
    scores = sentinel_buffer(ctx, 64)
    assert raw(ctx, G, None, 1, 4, None, scores) == (EINVAL, 12345)
    assert ctx.lib.ii2_last_error(ctx.h).decode() == "ii2_topk_ranges: output buffer is NULL"
    assert np.all(scores.download() == SENTINEL)
    # 255 groups with postings and k = II2_TOPK_MAX are inside the limits
    ids, scores, n = ctx.topk_ranges(many[:255], _lib.II2_TOPK_MAX)
    assert n == 256 and ids.download(1).tolist() == [5] and scores.download(2).tolist() == [255, 1]
