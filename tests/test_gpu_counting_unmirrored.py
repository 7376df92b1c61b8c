"""GPU: the counting forms where the host mirrors no doc spans.  A segment of more than ii2_seg::SPAN_MIRROR_MAX lists
(path_cases.Layout("big")) leaves ii2_atleast_ranges, ii2_topk_ranges and ii2_topk_weighted_ranges to fetch the span of its groups
from the device (one reduction and a wait) and to mark every such group in every window.  Three required groups and an excluded
one: A in a small, mirrored segment; B, C and the excluded group in one segment of 65537 lists, B starting below and ending above
A's span - both fetched bounds win over the mirrored ones - and C overlapping both.  Each query at one window and at 65, against
numpy and against the same query with every list in small segments, bit for bit; n_windows is that of the true span."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import path_cases as pc
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

OK = 0
DEFAULTS = {"atleast.small": 1, "atleast.handoff": 1, "union.many_window_log2": 30, "topk.late": 1}
COUNTING = {"atleast.handoff": 0, "atleast.small": 0}
WINDOWS = [30, 11]
WEIGHTS = (1, 2, 4)
K_ALL = 1 << 16                      # more than the eligible docs


def _lists():
    rng = np.random.default_rng(65537)
    pick = lambda n, lo, hi: rng.choice(np.arange(lo, hi, dtype=np.uint32), n, replace=False)
    join = lambda fixed, more: np.union1d(np.array(fixed, np.uint32), more).astype(np.uint32)
    a = join([5, 2047, 2048, 3000, 70000], pick(600, 6, 70000))
    b = join([0, 2048, 3000, 70000, 131073], pick(900, 1, 131073))
    c = join([5, 2048, 2049, 3000, 69999, 70000, 131073], pick(700, 6, 131073))
    x = join([2048], pick(200, 1, 131073))
    x = np.setdiff1d(x, [5, 3000, 70000, 131073]).astype(np.uint32)     # (the tombstoned docs, the ends of A's span and of the whole span)
    return a, b, c, x


A, B, CC, X = _lists()
REQUIRED = (A, B, CC)
# a few tombstones: a doc in two groups, one in all three, one in no list
REMOVED = np.array([5, 3000, 131072], np.uint32)
LO, HI = 0, 131073


def scores_of(weights):
    """(ids, scores) of the docs that no excluded list and no tombstone removes, ids ascending"""
    ids = np.unique(np.concatenate(REQUIRED))
    score = np.zeros(ids.size, np.uint32)
    for l, w in zip(REQUIRED, weights):
        score += np.isin(ids, l).astype(np.uint32) * np.uint32(w)
    keep = ~np.isin(ids, X) & ~np.isin(ids, REMOVED)
    return ids[keep], score[keep]


def want_atleast(m):
    ids, score = scores_of((1, 1, 1))
    return ids[score >= m]


def want_ranked(weights, k, min_score=1):
    ids, score = scores_of(weights)
    ids, score = ids[score >= min_score], score[score >= min_score]
    hist = np.bincount(score, minlength=256).astype(np.uint64)
    order = np.lexsort((ids, -score.astype(np.int64)))[:k]
    return ids[order], score[order], hist


def n_windows(ctx, top, wlog2):
    """the windows of the true span [LO, HI] with counters that reach `top`"""
    planes, win, late = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert ctx.lib.ii2_atleast_plan(255, top, wlog2, C.byref(planes), C.byref(win), C.byref(late)) == OK
    assert planes.value == int(top).bit_length()
    base = LO & ~31
    return (HI - base + 1 + win.value - 1) // win.value


@pytest.fixture(scope="module")
def laid(ctx):
    """{"big" | "small": (groups, exclude)}, the tombstones"""
    b0, b1 = B[0::2], B[1::2]                                       # group B: a range of two lists
    seg_a = ctx.encode_lists([A])
    big = pc.Layout("big", [b0, b1, CC, X])
    seg_big = ctx.encode(*big.flat(0))
    assert seg_big.info.n_lists == pc.BIG_LISTS
    small = [ctx.encode_lists([b0, b1]), ctx.encode_lists([CC]), ctx.encode_lists([X])]
    tomb = ctx.tombstones(REMOVED)
    yield {"big": ([[(seg_a, 0, 1)], [(seg_big, 0, 2)], [(seg_big, 2, 3)]], [[(seg_big, 3, 4)]]),
           "small": ([[(seg_a, 0, 1)], [(small[0], 0, 2)], [(small[1], 0, 1)]], [[(small[2], 0, 1)]])}, tomb
    for k, v in DEFAULTS.items():
        ctx.set_option(k, v)
    tomb.free()
    for s in [seg_a, seg_big] + small:
        s.free()


def with_options(ctx, kv, fn):
    try:
        for k, v in kv.items():
            ctx.set_option(k, v)
        return fn()
    finally:
        for k in kv:
            ctx.set_option(k, DEFAULTS[k])


def test_the_case_is_what_it_says():
    assert (min(l[0] for l in REQUIRED), max(l[-1] for l in REQUIRED)) == (LO, HI)
    assert B[0] < A[0] and B[-1] > A[-1] and CC[0] <= A[-1] and CC[-1] > A[-1]
    assert 2048 in X and all(2048 in l for l in REQUIRED) and 2048 not in want_atleast(2)
    assert 5 in np.intersect1d(A, CC) and all(3000 in l for l in REQUIRED) and not np.isin(REMOVED, X).any()
    assert not np.isin(REMOVED[:2], want_atleast(1)).any()
    assert 70000 in want_atleast(2) and 131073 in want_atleast(2) and want_atleast(2).size > 3
    assert want_ranked((1, 1, 1), K_ALL)[0].size < K_ALL


@pytest.mark.parametrize("wlog2", WINDOWS)
def test_atleast_counting_form(ctx, laid, wlog2):
    layouts, tomb = laid
    want = want_atleast(2)
    got = {}
    for name, (groups, exclude) in layouts.items():
        out, n, st = with_options(ctx, dict(COUNTING, **{"union.many_window_log2": wlog2}),
                                  lambda: ctx.atleast_ranges(groups, 2, exclude, tomb=tomb, stats=True))
        print("atleast", name, wlog2, "count", n, "form", st.form, "windows", st.n_windows)
        got[name] = out.download(n)
        assert st.form == _lib.II2_ATLEAST_COUNT and st.n_counted == 3, name
        assert st.n_windows == n_windows(ctx, 2, wlog2) == (1 if wlog2 == 30 else 65), name
        assert n == want.size and np.array_equal(got[name], want), (name, np.setxor1d(got[name], want).tolist())
    assert got["big"].tobytes() == got["small"].tobytes()


def check_ranked(ctx, layouts, call, want, top, wlog2, what):
    want_ids, want_scores, want_hist = want
    got = {}
    for name, (groups, exclude) in layouts.items():
        ids, scores, n, hist, st = with_options(ctx, {"union.many_window_log2": wlog2}, lambda: call(groups, exclude))
        print(*what, name, wlog2, "count", n, "eligible", st.n_eligible, "windows", st.n_windows, "marks", st.n_marks)
        got[name] = (ids.download(n).tobytes(), scores.download(n).tobytes(), hist.tobytes(), n)
        assert st.n_windows == n_windows(ctx, top, wlog2) == (1 if wlog2 == 30 else 65), (what, name)
        assert n == want_ids.size and st.n_eligible == int(want_hist.sum()), (what, name)
        assert np.array_equal(ids.download(n), want_ids) and np.array_equal(scores.download(n), want_scores), (what, name)
        assert np.array_equal(hist, want_hist), (what, name)
    assert got["big"] == got["small"], what


@pytest.mark.parametrize("wlog2", WINDOWS)
@pytest.mark.parametrize("k", [3, K_ALL])
def test_topk_ranges(ctx, laid, k, wlog2):
    layouts, tomb = laid
    check_ranked(ctx, layouts, lambda groups, exclude: ctx.topk_ranges(groups, k, 1, exclude, tomb=tomb, stats=True),
                 want_ranked((1, 1, 1), k), 3, wlog2, ("topk", k))


@pytest.mark.parametrize("wlog2", WINDOWS)
@pytest.mark.parametrize("late", [1, 0])
def test_topk_weighted_ranges(ctx, laid, late, wlog2):
    layouts, tomb = laid
    call = lambda groups, exclude: with_options(ctx, {"topk.late": late}, lambda: ctx.topk_weighted_ranges(groups, WEIGHTS, 3, 1, exclude, tomb=tomb, stats=True))
    check_ranked(ctx, layouts, call, want_ranked(WEIGHTS, 3), sum(WEIGHTS), wlog2, ("topkw", "late", late))
