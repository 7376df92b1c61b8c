"""GPU: the two contracts of every query entry point, on every kernel path (tests/contract_cases.py).

Tombstones: each distinct case of the path table runs under every layout of removed ids - a bitmap of no words, one that ends in
the middle of the results with one bit or with 32 in its last word, summary bits that lie about their neighbours, every hit removed,
a bitmap far past every list - and must return the numpy reference bit for bit, write nothing behind the result and take the path
the table names.  The readers the path table does not reach run under the same layouts with their own references: the three
instances of the one-launch two-list AND, ii2_merge_segments (direct and packed), ii2_count_ranges (against a set, and every doc),
ii2_histogram_ranges (both forms, under an axis for each of its sinks), ii2_histogram_ids, ii2_atleast_ranges (one launch, and
counting) and the three ranked entry points.

Capacity: each case runs at exactly enough, one too few and none, into a buffer that is always allocated at the generous size and
filled with a sentinel - a store past `cap` lands inside the allocation, where the test sees it.  The range and batch entry points
are all-or-nothing and report the size needed; ii2_intersect / ii2_union promise only that nothing is written at or past `cap`."""
import dataclasses

import numpy as np
import pytest

from tests import atleast_cases as ac
from tests import contract_cases as cc
from tests import hist_cases as hc
from tests import merge_cases as mc
from tests import path_cases as pc
from tests import topk_batch_cases as bc
from tests import topk_cases as tc
from tests import topkw_cases as wc
from tests import wide_cases as wd
from tests.gpu_util import SENTINEL, call_case, case_capacity, ctx, path_delta, raw_call_case, sorted_unique  # noqa: F401
from tests.test_gpu_count_ranges import truth as count_truth

pytestmark = pytest.mark.gpu

OK, ECAPACITY = 0, -4
ONE_LAUNCH_AND = {"and.and2_fused": 1}
REPEATED = {"and.and2_fused": 1, "and.and2_split": 1}           # (a look-back wait that ran out repeats the call)
ALL_OR_NOTHING = ("union_ranges", "intersect_ranges", "andnot", "batch", "gbatch")
RUN = [c for c in cc.PATH_CASES if c.name not in cc.DEGENERATE]


def took_the_path(case, delta):
    want = case.expect_in("one")
    return delta == want or (want == ONE_LAUNCH_AND and delta == REPEATED)


class Options:
    """the options set on entry go back to the given defaults on exit, whatever happens in between"""

    def __init__(self, ctx, kv, defaults):
        self.ctx, self.kv, self.defaults = ctx, kv, defaults

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set_option(k, self.defaults[k])


def layouts_of(R, E):
    """(layout, removed ids) for every layout R can carry (a reader's case of a handful of hits in one word cannot carry all)"""
    out = [(layout, cc.removed_for(layout, R, E)) for layout in cc.LAYOUTS]
    return [(layout, removed) for layout, removed in out if removed is not None]


# ---- the path table under the tombstone layouts ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", RUN, ids=lambda c: c.name)
def test_tombstone_layouts(ctx, case):
    lists = case.lists()
    lay = pc.Layout("one", lists)
    R, E = cc.sets_of(case, lists)
    segs = [ctx.encode(*lay.flat(s)) for s in range(len(lay.segments))]
    try:
        with Options(ctx, case.options, pc.DEFAULTS):
            for layout in cc.LAYOUTS:
                removed = cc.removed_for(layout, R, E)
                want = pc.reference(case, lists, removed)
                tomb = ctx.tombstones(removed)
                try:
                    with path_delta(ctx) as took:
                        got, off = call_case(ctx, case, segs, lay, tomb, want)      # (asserts the sentinel behind the result)
                finally:
                    tomb.free()
                print(case.name, layout, "removed", removed.size, "words", cc.n_words(removed), "count", int(off[-1]), took)
                assert list(off) == list(np.cumsum([0] + [w.size for w in want])), layout
                for q, (g, w) in enumerate(zip(got, want)):
                    assert g.dtype == np.uint32 and np.array_equal(g.astype(np.uint64), w), (layout, q, np.setxor1d(g.astype(np.uint64), w)[:8].tolist())
                assert took_the_path(case, took), (layout, took)
    finally:
        for s in segs:
            s.free()


# ---- the path table under the capacities -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cc.PATH_CASES, ids=lambda c: c.name)
def test_capacities(ctx, case):
    lists = case.lists()
    lay = pc.Layout("one", lists)
    want = pc.reference(case, lists)
    sizes = list(np.cumsum([0] + [w.size for w in want]))
    n = int(sizes[-1])
    kind = case.call[0]
    size = case_capacity(case, lay) + 64                                            # what call_case allocates
    fill = np.full(size, SENTINEL, np.uint32)
    segs = [ctx.encode(*lay.flat(s)) for s in range(len(lay.segments))]
    out = ctx.empty(size)
    try:
        with Options(ctx, case.options, pc.DEFAULTS):
            for cap in cc.capacities(n):
                out.upload(fill)
                with path_delta(ctx) as took:
                    rc, count, off = raw_call_case(ctx, case, segs, lay, out, cap)
                got = out.download()
                print(case.name, "cap", cap, "of", n, "rc", rc, "count", count, took)
                what = (cap, rc, count)
                if cap == n:
                    assert rc == OK and list(off) == sizes, what
                    assert np.array_equal(got[:n].astype(np.uint64), np.concatenate(want)), what
                    assert np.all(got[n:] == SENTINEL), (what, "ids written behind the result")
                    if kind in ("intersect", "union"):                              # (their choosers do not read the capacity)
                        assert took_the_path(case, took), took
                    continue
                assert rc == ECAPACITY, what
                assert np.all(got[cap:] == SENTINEL), (what, "ids written at or past the capacity", np.flatnonzero(got[cap:] != SENTINEL)[:8].tolist())
                if kind in ALL_OR_NOTHING:
                    assert np.all(got == SENTINEL), (what, "written despite II2_ECAPACITY")
                    assert count == n and list(off) == sizes, (what, list(off))     # the size needed; a batch's offsets completely filled
                else:
                    assert count > cap, what
    finally:
        out.free()
        for s in segs:
            s.free()


# ---- the three instances of the one-launch two-list AND ---------------------------------------------------------------------------
AND2_DEFAULTS = {"intersect.dense_form": 1, "intersect.and2_tiles": 0}
AND2_INSTANCES = {"marking": {"intersect.dense_form": 0},                                           # the marking kernel
                  "dense_form_one_tile": {"intersect.dense_form": 2, "intersect.and2_tiles": 1},    # k_and2_fused<true>
                  "dense_form_two_tiles": {"intersect.dense_form": 2, "intersect.and2_tiles": 2}}   # k_and2_fused_x2


@pytest.fixture(scope="module")
def and2(ctx):
    case = next(c for c in cc.PATH_CASES if c.name == "and_and2_fused_1024_blocks")
    lists = case.lists()
    lay = pc.Layout("one", lists)
    segs = [ctx.encode(*lay.flat(0))]
    yield case, lists, lay, segs, cc.sets_of(case, lists)
    segs[0].free()


@pytest.mark.parametrize("instance", AND2_INSTANCES)
def test_two_list_and_instances(ctx, and2, instance):
    case, lists, lay, segs, (R, E) = and2
    with Options(ctx, AND2_INSTANCES[instance], AND2_DEFAULTS):
        if instance != "marking":
            call_case(ctx, case, segs, lay, None, pc.reference(case, lists))       # (the first call makes the form)
            assert segs[0].dense_form(0, words=False) is not None or segs[0].dense_form(1, words=False) is not None
        for layout in cc.LAYOUTS:
            removed = cc.removed_for(layout, R, E)
            want = pc.reference(case, lists, removed)
            tomb = ctx.tombstones(removed)
            try:
                with path_delta(ctx) as took:
                    got, off = call_case(ctx, case, segs, lay, tomb, want)
            finally:
                tomb.free()
            print(instance, layout, "count", int(off[-1]), took)
            assert int(off[-1]) == want[0].size and np.array_equal(got[0].astype(np.uint64), want[0]), (layout, np.setxor1d(got[0].astype(np.uint64), want[0])[:8].tolist())
            assert took in (ONE_LAUNCH_AND, REPEATED), (layout, took)


# ---- ii2_merge_segments ----------------------------------------------------------------------------------------------------------
OFF_SENTINEL = 0xABCDEF0123456789


@pytest.mark.parametrize("name", cc.MERGE_CASES)
def test_merge_segments(ctx, name):
    case = mc.BY_NAME[name]
    host = case.segs()
    T, n_in = host[0][0].size - 1, int(sum(v.size for _, v in host))
    R = cc.every_id([v for _, v in host])                                           # the merged ids without tombstones
    segs = [ctx.encode(o, v) for o, v in host]
    out_off = ctx.empty(T + 1, np.uint64)
    out_vals = ctx.empty(n_in + 64)
    try:
        with Options(ctx, dict(case.options, **{"merge.direct": 1}), mc.DEFAULTS):
            for layout, removed in layouts_of(R, R):
                w_off, w_vals = mc.reference(host, removed)
                n_out = int(w_off[-1])
                tomb = ctx.tombstones(removed)
                try:
                    for direct in (1, 0):
                        ctx.set_option("merge.direct", direct)
                        out_off.upload(np.full(T + 1, OFF_SENTINEL, np.uint64))
                        out_vals.upload(np.full(n_in + 64, SENTINEL, np.uint32))
                        out_vals.count = n_in                                       # (what the entry point takes as the capacity)
                        before = ctx.merge_events()
                        try:
                            _, _, st = ctx.merge(segs, tomb, out_off, out_vals)
                        finally:
                            out_vals.count = n_in + 64
                        after = ctx.merge_events()
                        delta = {k: after[k] - before[k] for k in after if after[k] != before[k]}
                        got = out_vals.download()
                        what = (name, layout, "direct" if direct else "packed")
                        print(*what, "removed", removed.size, "out", st.n_out, delta)
                        assert np.array_equal(out_off.download(), w_off), what
                        assert np.array_equal(got[:n_out].astype(np.uint64), w_vals), (what, np.setxor1d(got[:n_out].astype(np.uint64), w_vals)[:8].tolist())
                        assert np.all(got[n_out:] == SENTINEL), (what, "ids written behind the result")
                        assert (st.n_in, st.n_out, st.n_tiles) == (n_in, n_out, case.plan().n_tiles), what
                        assert delta == case.events(), what
                finally:
                    tomb.free()
    finally:
        out_off.free()
        out_vals.free()
        for s in segs:
            s.free()


# ---- ii2_count_ranges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["set", "every_doc"])
def test_count_ranges(ctx, form):
    rng = np.random.default_rng(41)
    D = 60_000
    lists = [sorted_unique(rng, n, D) for n in (255, 256, 1025)]
    ids = sorted_unique(rng, 4097, D) if form == "set" else None
    E = cc.every_id(lists)
    R = E if ids is None else np.intersect1d(E, ids.astype(np.uint64))             # the ids of the set, or of the lists, that hit
    assert R.size > 100
    seg = ctx.encode_lists(lists)
    dset = ctx.empty(ids.size).upload(ids) if ids is not None else None
    try:
        for layout in cc.LAYOUTS:
            removed = cc.removed_for(layout, R, E)
            tomb = ctx.tombstones(removed)
            try:
                got, st = ctx.count_ranges([(seg, 0, len(lists))], dset, None if dset is None else ids.size, tomb=tomb)
            finally:
                tomb.free()
            want = count_truth(lists, ids, removed)
            print(form, layout, got.tolist(), want.tolist())
            assert np.array_equal(got, want) and st.n_hits == int(want.sum()), (form, layout)
            if layout == "all_hits":
                assert not want.any()
    finally:
        seg.free()
        if dset is not None:
            dset.free()


# ---- ii2_histogram_ranges, ii2_histogram_ids ---------------------------------------------------------------------------------------
HIST_D = 60_000
# axis -> (edges, the sink the blocks of these lists must reach under it: a whole block in one bucket, up to 64 buckets, more)
HIST_AXES = {"one_bucket": ([0, hc.TOP], "n_whole"), "24_buckets": (hc.uniform(0, HIST_D, 24), "n_split"), "4096_buckets": (hc.uniform(0, HIST_D, 4096), "n_wide")}


@pytest.mark.parametrize("axis", HIST_AXES)
@pytest.mark.parametrize("form", ["set", "every_doc"])
def test_histogram_ranges(ctx, form, axis):
    """test_count_ranges' lists and set per bucket of an axis: k_hs_count<true> (every doc) tests each decoded id, k_hs_count<false>
    relies on the facet count's marks"""
    rng = np.random.default_rng(41)
    lists = [sorted_unique(rng, n, HIST_D) for n in (255, 256, 1025)]
    ids = sorted_unique(rng, 4097, HIST_D) if form == "set" else None
    edges, sink = HIST_AXES[axis]
    E = cc.every_id(lists)
    R = E if ids is None else np.intersect1d(E, ids.astype(np.uint64))
    assert R.size > 100
    seg = ctx.encode_lists(lists)
    dset = ctx.empty(ids.size).upload(ids) if ids is not None else None
    n_set = None if dset is None else ids.size
    try:
        with Options(ctx, {"count.summary_skip": 0}, {"count.summary_skip": 1}):
            got, st = ctx.histogram_ranges([(seg, 0, len(lists))], edges, dset, n_set)
            print(form, axis, "whole", st.n_whole, "split", st.n_split, "wide", st.n_wide)
            assert getattr(st, sink) > 0 and np.array_equal(got, hc.truth(lists, ids, edges)), (form, axis)
            for layout in cc.LAYOUTS:
                removed = cc.removed_for(layout, R, E)
                tomb = ctx.tombstones(removed)
                try:
                    got, st = ctx.histogram_ranges([(seg, 0, len(lists))], edges, dset, n_set, tomb=tomb)
                finally:
                    tomb.free()
                want = hc.truth(lists, ids, edges, removed)
                print(form, axis, layout, "removed", removed.size, "hits", int(want.sum()))
                assert np.array_equal(got, want), (form, axis, layout, np.argwhere(got != want)[:8].tolist())
                assert st.n_hits == int(want.sum()), (form, axis, layout)
                if layout == "all_hits":
                    assert not want.any()
    finally:
        seg.free()
        if dset is not None:
            dset.free()


def test_histogram_ids(ctx):
    """k_hs_ids_tomb: runs of equal buckets that end inside and across waves where the bitmap ends"""
    rng = np.random.default_rng(41)
    ids = sorted_unique(rng, 4097, HIST_D)
    R = ids.astype(np.uint64)
    dset = ctx.empty(ids.size).upload(ids)
    try:
        for name, edges in (("edge_at_the_middle_hit", [0, cc.middle(R), HIST_D]), ("160_buckets", hc.uniform(0, HIST_D, 160))):
            for layout in cc.LAYOUTS:
                removed = cc.removed_for(layout, R, R)
                tomb = ctx.tombstones(removed)
                try:
                    got = ctx.histogram_ids(dset, ids.size, edges, tomb=tomb)
                finally:
                    tomb.free()
                want = hc.truth([ids], None, edges, removed)[0]
                print(name, layout, "removed", removed.size, "left", int(want.sum()))
                assert got.dtype == np.uint64 and np.array_equal(got, want), (name, layout, np.flatnonzero(got != want)[:8].tolist())
                if layout == "all_hits":
                    assert not want.any()
    finally:
        dset.free()


# ---- the threshold and ranked queries -----------------------------------------------------------------------------------------------
class Laid:
    """a case's lists in one segment: its groups as the ranges the entry points take"""

    def __init__(self, ctx, case):
        self.seg = ctx.encode_lists(case.lists)
        self.groups = [[(self.seg, i, i + 1) for i in g] for g in case.groups]
        self.exclude = [[(self.seg, i, i + 1) for i in g] for g in case.exclude]

    def free(self):
        self.seg.free()


def with_removed(case, removed):
    return dataclasses.replace(case, removed=[int(x) for x in removed])


ATLEAST_DEFAULTS = {"atleast.small": 1, "atleast.handoff": 1}
ATLEAST = [("basic_m2", ac.BY_NAME["basic_m2"], [2], {}, ac.SMALL),
           ("three_workgroups", wd.BY_NAME["three_workgroups"].case, [m for _, m in wd.BY_NAME["three_workgroups"].atleast], wd.COUNTING, ac.COUNT)]


@pytest.mark.parametrize("name,case,ms,options,form", ATLEAST, ids=[a[0] for a in ATLEAST])
def test_atleast_ranges(ctx, name, case, ms, options, form):
    E = cc.every_id(case.lists)
    L = Laid(ctx, case)
    try:
        with Options(ctx, options, ATLEAST_DEFAULTS):
            for m in ms:
                R = ac.reference(case, m=m).astype(np.uint64)                       # the eligible docs without tombstones
                for layout, removed in layouts_of(R, E):
                    want = ac.reference(with_removed(case, removed), m=m, tomb=True)
                    tomb = ctx.tombstones(removed)
                    out = ctx.empty(R.size + 64).upload(np.full(R.size + 64, SENTINEL, np.uint32))
                    out.count = R.size
                    try:
                        _, n, st = ctx.atleast_ranges(L.groups, m, L.exclude, tomb=tomb, out=out, stats=True)
                    finally:
                        tomb.free()
                        out.count = R.size + 64
                    got = out.download()
                    print(name, "m", m, layout, "count", n, "form", st.form)
                    assert st.form == form, (m, layout)
                    assert n == want.size and np.array_equal(got[:n], want), (m, layout, np.setxor1d(got[:n], want)[:8].tolist())
                    assert np.all(got[n:] == SENTINEL), (m, layout)
                    out.free()
    finally:
        L.free()


def _postings(case):
    return sum(int(l.size) for l in case.lists)


TOP_SMALLEST = min(tc.CASES, key=lambda t: _postings(t.case))
TOP_WIDE = wd.BY_NAME["three_workgroups"]
RANKED = [(TOP_SMALLEST.name, TOP_SMALLEST.case, TOP_SMALLEST.ks, next(w for w in wc.CASES if w.case.name == TOP_SMALLEST.name).weights),
          (TOP_WIDE.name, TOP_WIDE.case, TOP_WIDE.top.ks, TOP_WIDE.weighted[0].weights)]


@pytest.mark.parametrize("name,case,ks,weights", RANKED, ids=[r[0] for r in RANKED])
def test_ranked_queries(ctx, name, case, ks, weights):
    """ii2_topk_ranges and ii2_topk_weighted_ranges at min_match / min_score 1: R is every eligible doc"""
    E = cc.every_id(case.lists)
    R = tc.scores_of(case)[0].astype(np.uint64)
    assert np.array_equal(R, wc.scores_of(case, weights)[0].astype(np.uint64))
    L = Laid(ctx, case)
    try:
        for layout, removed in layouts_of(R, E):
            gone = with_removed(case, removed)
            tomb = ctx.tombstones(removed)
            try:
                for k in ks:
                    for weighted in (False, True):
                        want_ids, want_scores, want_hist = wc.reference(gone, weights, k, 1, True) if weighted else tc.reference(gone, k, 1, True)
                        ids = ctx.empty(k + 8).upload(np.full(k + 8, SENTINEL, np.uint32))
                        scores = ctx.empty(k + 8).upload(np.full(k + 8, SENTINEL, np.uint32))
                        if weighted:
                            _, _, n, hist, _ = ctx.topk_weighted_ranges(L.groups, weights, k, 1, L.exclude, tomb=tomb, stats=True, out=(ids, scores))
                        else:
                            _, _, n, hist, _ = ctx.topk_ranges(L.groups, k, 1, L.exclude, tomb=tomb, stats=True, out=(ids, scores))
                        got_ids, got_scores = ids.download(), scores.download()
                        what = (name, layout, k, "weighted" if weighted else "plain")
                        assert n == want_ids.size and np.array_equal(got_ids[:n], want_ids), (what, got_ids[:n].tolist()[:8], want_ids.tolist()[:8])
                        assert np.array_equal(got_scores[:n], want_scores), what
                        assert np.all(got_ids[n:] == SENTINEL) and np.all(got_scores[n:] == SENTINEL), what
                        assert np.array_equal(hist, want_hist), what
                        ids.free()
                        scores.free()
            finally:
                tomb.free()
            print(name, layout, "removed", removed.size, "eligible", int(want_hist.sum()))
    finally:
        L.free()


# the smallest case of the table (a handful of ids in one word), and the smallest that fills each form of the batch kernel over many words
BATCHED = [min(bc.CASES, key=lambda b: _postings(b.w.case)).name, "tiny_2048", "capacity_8192"]


@pytest.mark.parametrize("name", BATCHED)
def test_topk_batch(ctx, name):
    t = bc.BY_NAME[name].w
    case = t.case
    E = cc.every_id(case.lists)
    R = wc.scores_of(case, t.weights)[0].astype(np.uint64)
    items = [(k, m) for m in t.min_scores for k in t.ks]
    L = Laid(ctx, case)
    try:
        for layout, removed in layouts_of(R, E):
            gone = with_removed(case, removed)
            tomb = ctx.tombstones(removed)
            total = sum(k for k, _ in items)
            ids = ctx.empty(total + 8).upload(np.full(total + 8, SENTINEL, np.uint32))
            scores = ctx.empty(total + 8).upload(np.full(total + 8, SENTINEL, np.uint32))
            ids.count = scores.count = total                                        # (what the entry point takes as the capacity)
            try:
                _, _, off, eligible, st = ctx.topk_batch([(L.groups, t.weights, k, m, L.exclude) for k, m in items], tomb=tomb, stats=True, out=(ids, scores))
            finally:
                tomb.free()
                ids.count = scores.count = total + 8
            got_ids, got_scores = ids.download(), scores.download()
            print(name, layout, "removed", removed.size, "results", int(off[-1]), "tiny", st.n_tiny, "small", st.n_small, "single", st.n_single)
            for q, (k, m) in enumerate(items):
                want_ids, want_scores, want_hist = wc.reference(gone, t.weights, k, m, True)
                a, b = int(off[q]), int(off[q + 1])
                what = (name, layout, k, m)
                assert b - a == want_ids.size and np.array_equal(got_ids[a:b], want_ids), what
                assert np.array_equal(got_scores[a:b], want_scores) and int(eligible[q]) == int(want_hist.sum()), what
            assert np.all(got_ids[int(off[-1]):] == SENTINEL) and np.all(got_scores[int(off[-1]):] == SENTINEL), (name, layout)
            ids.free()
            scores.free()
    finally:
        L.free()
