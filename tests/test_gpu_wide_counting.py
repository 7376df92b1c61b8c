"""GPU: the threshold and ranked queries beyond one workgroup - every case of tests/wide_cases.py (several workgroups, a ragged last
one, a second grid-stride step, a count table of two scan tiles, the sixteen windows of the default union.many_window_log2 up to id
0xFFFFFFFF) through ii2_atleast_ranges forced to its counting form, ii2_topk_ranges at every k and min_match of the case and
ii2_topk_weighted_ranges at topk.late 0 and 1, the lists in one segment and in two, with and without tombstones, at the default
window - against numpy (tests/atleast_cases, topk_cases and topkw_cases: np.unique, bincount, lexsort), bit for bit: ids, scores,
count, histogram and stats.  The path counters do not move, nothing is written behind count in buffers of k + 8 entries, and after
every call the scratch is all zero: a block-wise union over a probe list of the same span returns the probe's ids and nothing else."""
import ctypes as C

import numpy as np
import pytest
import torch

from inverted_index_2_amd import _lib
from tests import atleast_cases as ac
from tests import topk_cases as tc
from tests import topkw_cases as wc
from tests import wide_cases as wd
from tests.gpu_util import ctx, path_delta  # noqa: F401
from tests.test_gpu_topk_ranges import SENTINEL, Laid, expected_marks, host_cut, sentinel_buffer

pytestmark = pytest.mark.gpu

OK = 0
DEFAULTS = {"atleast.small": 1, "atleast.handoff": 1, "union.many_window_log2": 30, "union.many": 0, "topk.late": 1}
SEGS = [1, 2]


class Options:
    """the options set on entry go back to their defaults on exit, whatever happens in between"""

    def __init__(self, ctx, kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set_option(k, DEFAULTS[k])


@pytest.fixture(scope="module")
def laid(ctx):
    cache = {}

    def get(case, n_segs=1):
        if (case.name, n_segs) not in cache:
            cache[case.name, n_segs] = Laid(ctx, case, n_segs)
        return cache[case.name, n_segs]
    yield get
    for k in DEFAULTS:
        ctx.set_option(k, DEFAULTS[k])


class Probe:
    """a list over exactly the span of a case's required groups - its first and last id, and the free neighbours of every id the
    case uses - and the check that the scratch is all zero: the block-wise union over it, with the windows of the call before, returns
    its ids and nothing else (a bitmap, plane or summary bit left behind shows up as a ghost id or a missing one)"""

    def __init__(self, ctx, case):
        used = np.unique(np.concatenate(case.lists).astype(np.int64))
        base, hi = wd.window_span(case)
        lo = min(int(ids[0]) for ids in (case.ids(g) for g in case.groups) if ids.size)
        near = np.setdiff1d(np.concatenate([used - 1, used + 1, used + wd.CHUNK, used - 33]), used)
        near = near[(near > lo) & (near < hi)]
        self.ids = np.union1d(near, [lo, hi]).astype(np.uint32)
        self.seg = ctx.encode_lists([self.ids])
        self.ctx = ctx

    def scratch_is_zero(self, window, what):
        wlog2 = int(window).bit_length() - 1
        assert 1 << wlog2 == window
        with Options(self.ctx, {"union.many": 1, "union.many_window_log2": wlog2}):
            u, n = self.ctx.union_ranges([(self.seg, 0, 1)])
        assert n == self.ids.size and np.array_equal(u.download(n), self.ids), ("scratch left dirty", what)


@pytest.fixture(scope="module")
def probe(ctx):
    cache = {}

    def get(case):
        if case.name not in cache:
            cache[case.name] = Probe(ctx, case)
        return cache[case.name]
    return get


_REF = {}


def ref(key, fn):
    """a reference, computed once and shared"""
    if key not in _REF:
        _REF[key] = fn()
    return _REF[key]


def atleast_plan(ctx, n_counted, m):
    planes, win, late = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert ctx.lib.ii2_atleast_plan(n_counted, m, DEFAULTS["union.many_window_log2"], C.byref(planes), C.byref(win), C.byref(late)) == OK
    return planes.value, win.value, late.value


def topkw_plan(ctx, t, min_score):
    """(total_weight, n_planes, window_docs, n_late) of ii2_topkw_plan for the case's counted groups"""
    weights, postings = [t.weights[g] for g in t.counted], t.postings
    n = len(weights)
    late = (C.c_uint8 * n)()
    total, planes, win, n_late = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
    assert ctx.lib.ii2_topkw_plan(n, (C.c_uint32 * n)(*weights), (C.c_uint64 * n)(*postings), min_score, DEFAULTS["union.many_window_log2"],
                                  C.byref(total), C.byref(planes), C.byref(win), late, C.byref(n_late)) == OK
    assert list(late) == wc.late_rule(weights, postings, min_score)
    return total.value, planes.value, win.value, n_late.value


def check_ranked(got, want, k, what):
    """ids, scores, count and histogram against the reference; nothing written behind count in the buffers of k + 8 entries"""
    ids, scores, n, hist = got
    want_ids, want_scores, want_hist = want
    got_ids, got_scores = ids.download(), scores.download()
    assert got_ids.size == got_scores.size == k + 8
    assert n == want_ids.size, what
    assert np.array_equal(got_ids[:n], want_ids), (what, got_ids[:n].tolist(), want_ids.tolist())
    assert np.array_equal(got_scores[:n], want_scores), what
    assert np.all(got_ids[n:] == SENTINEL) and np.all(got_scores[n:] == SENTINEL), what
    assert np.array_equal(hist, want_hist), what


# ---- the device is the one the cases were made for ---------------------------------------------------------------------------------
def test_the_stride_cases_stride_on_this_device(ctx):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for name, per_cu in (("hist_stride", wd.GRID_CUS), ("full_stride", 4 * wd.GRID_CUS)):
        c = wd.BY_NAME[name]
        _, win, _ = atleast_plan(ctx, c.case.n_counted, c.case.n_counted)
        n_sum = wd.n_sum_of(c.case, win)
        print(name, "n_sum", n_sum, "compute units", cus)
        assert n_sum > per_cu * cus, f"{name}: {n_sum} summary words do not exceed {per_cu} x {cus} compute units - the case does not reach its regime on this device"
    assert wd.steps_of(wd.BY_NAME["full_stride"].regime["n_sum"], cus) >= 2
    assert wd.steps_of(wd.BY_NAME["hist_stride"].regime["n_sum"], cus, wd.HIST_CUS) >= 2


# ---- the threshold query, counting form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_segs", SEGS)
@pytest.mark.parametrize("c", wd.CASES, ids=lambda c: c.name)
def test_atleast_counting_form(ctx, laid, probe, c, n_segs):
    for case, m in c.atleast:
        L, P = laid(case, n_segs), probe(case)
        n1 = case.n_counted
        planes, win, first_late = atleast_plan(ctx, n1, m)
        for tomb in (False, True):
            with Options(ctx, wd.COUNTING), path_delta(ctx) as took:
                out, n, st = ctx.atleast_ranges(L.groups, m, L.exclude, tomb=L.tomb if tomb else None, stats=True)
            want = ref(("atleast", case.name, m, tomb), lambda: ac.reference(case, m=m, tomb=tomb))
            what = (case.name, n_segs, m, tomb)
            print(*what, "count", n, "form", st.form, "planes", st.n_planes, "windows", st.n_windows, "late", st.n_late)
            assert took == {}, what
            assert st.form == ac.COUNT, what
            got = out.download(n)
            assert n == want.size and np.array_equal(got, want), (what, np.setxor1d(got, want).tolist())
            assert (st.n_counted, st.n_planes, st.n_windows, st.n_late) == (n1, planes, wd.n_windows_of(case, win), n1 - first_late) == \
                   (n1, m.bit_length(), wd.n_windows_of(case, win), m - 1), what
            P.scratch_is_zero(win, what)


# ---- the ranked query ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_segs", SEGS)
@pytest.mark.parametrize("c", wd.CASES, ids=lambda c: c.name)
def test_topk_ranges(ctx, laid, probe, c, n_segs):
    t, case = c.top, c.case
    L, P = laid(case, n_segs), probe(case)
    n1 = case.n_counted
    _, win, _ = atleast_plan(ctx, n1, n1)
    for tomb in (False, True):
        for m in t.min_matches:
            for k in t.ks:
                out = (sentinel_buffer(ctx, k + 8), sentinel_buffer(ctx, k + 8))
                with path_delta(ctx) as took:
                    ids, scores, n, hist, st = ctx.topk_ranges(L.groups, k, m, L.exclude, tomb=L.tomb if tomb else None, stats=True, out=out)
                want = ref(("topk", t.name, k, m, tomb), lambda: tc.reference(case, k, m, tomb))
                what = (t.name, n_segs, tomb, m, k)
                print(*what, "count", n, "eligible", st.n_eligible, "cut", st.cut_score, st.n_cut, "windows", st.n_windows, "marks", st.n_marks)
                assert took == {}, what
                check_ranked((ids, scores, n, hist), want, k, what)
                want_hist = want[2]
                assert st.n_counted == n1 and st.n_eligible == int(want_hist.sum()), what
                mx, cs, _, n_cut = host_cut(ctx, want_hist, k)
                assert (st.max_score, st.cut_score, st.n_cut) == (mx, cs, n_cut) == tc.cut(want_hist, k)[:2] + (tc.cut(want_hist, k)[3],), what
                n_win, marks = expected_marks(case, win, n > 0)
                assert (st.n_planes, st.n_windows, st.n_marks) == (n1.bit_length(), n_win, marks) and n_win == c.regime["n_windows"], what
                P.scratch_is_zero(win, what)


# ---- the weighted ranked query -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_segs", SEGS)
@pytest.mark.parametrize("c", wd.CASES, ids=lambda c: c.name)
def test_topk_weighted_ranges(ctx, laid, probe, c, n_segs):
    case = c.case
    L, P = laid(case, n_segs), probe(case)
    for t in c.weighted:
        W = t.total_weight
        for m in t.min_scores:
            total, planes, win, n_late = topkw_plan(ctx, t, m)
            assert (total, planes) == (W, W.bit_length())
            for tomb in (False, True):
                for k in t.ks:
                    want = ref(("topkw", t.name, k, m, tomb), lambda: wc.reference(case, t.weights, k, m, tomb))
                    want_hist = want[2]
                    for late in (1, 0):
                        out = (sentinel_buffer(ctx, k + 8), sentinel_buffer(ctx, k + 8))
                        with Options(ctx, {"topk.late": late}), path_delta(ctx) as took:
                            ids, scores, n, hist, st = ctx.topk_weighted_ranges(L.groups, t.weights, k, m, L.exclude, tomb=L.tomb if tomb else None,
                                                                                stats=True, out=out)
                        what = (t.name, n_segs, tomb, m, k, "late", late)
                        print(*what, "count", n, "eligible", st.n_eligible, "cut", st.cut_score, st.n_cut, "windows", st.n_windows, "marks", st.n_marks,
                              "late groups", st.n_late)
                        assert took == {}, what
                        check_ranked((ids, scores, n, hist), want, k, what)
                        assert st.n_counted == case.n_counted and st.total_weight == W and st.n_eligible == int(want_hist.sum()), what
                        mx, cs, _, n_cut = host_cut(ctx, want_hist, k)
                        assert (st.max_score, st.cut_score, st.n_cut) == (mx, cs, n_cut), what
                        n_win, marks = expected_marks(case, win, n > 0)
                        assert (st.n_planes, st.n_windows, st.n_marks, st.n_late) == (W.bit_length(), n_win, marks, n_late if late else 0), what
                        P.scratch_is_zero(win, what)
