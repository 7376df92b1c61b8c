"""GPU: the readers that came after tests/test_gpu_segment_kinds.py, on every way of making a segment (tests/segment_kinds.py),
against plain numpy over the plan's slots alone.

Each of them reads a segment's derived arrays with code of its own:
  - ii2_explain_ranges walks blk_list, skip[b + 1] and last_doc in k_ex_match, window by window;
  - ii2_histogram_ranges runs on the facet count's walk (tests/test_gpu_histogram_ranges.py: test_segment_kinds has that call);
  - the one-workgroup forms - ii2_intersect / ii2_union of short lists, ii2_query_batch, ii2_query_batch_groups, ii2_topk_batch,
    ii2_explain_batch, the one-launch form of ii2_atleast_ranges - build their list descriptors on the host from the block-offset
    and count mirrors, which a view and a segment of 65537 lists fetch lazily;
  - the group path of ii2_intersect_ranges probes or marks by the host span mirror, or without one.
What is asked is segment_kinds.queries(kind): lists chosen by their lengths so that the 256-thread form, the 1024-thread form and
the fallback are each taken (tests/test_segment_kinds_cpu.py proves the sizes for every kind)."""
import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import explain_cases as xc
from tests import segment_kinds as sk
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = list(sk.KINDS)
PROBE, MARK = {"intersect.ranges_mark": 0}, {"intersect.ranges_mark": 1 << 40}     # tests/path_cases.py: ir_probe / ir_mark
RANGES_MARK_DEFAULT = 64


@pytest.fixture(scope="module")
def made(ctx):
    """(kind, shape) -> (segment, plan, queries): every kind's segment of a shape, made once."""
    cache, keep = {}, []

    def get(kind, shape=sk.READER_SHAPE):
        if (kind, shape) not in cache:
            p = sk.plan(kind, shape)
            seg, alive = sk.make(ctx, p)
            keep.extend(alive)
            # (queries caches by its arguments as they are written: the readers' shape as the other test files ask for it)
            cache[kind, shape] = (seg, p, sk.queries(kind) if shape == sk.READER_SHAPE else sk.queries(kind, shape))
        return cache[kind, shape]
    yield get
    for seg, _, _ in cache.values():
        seg.free()
    for s in keep:
        s.free()


class Options:
    def __init__(self, ctx, values, defaults):
        self.ctx, self.values, self.defaults = ctx, values, defaults

    def __enter__(self):
        for k, v in self.values.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.ctx.set_option(k, self.defaults[k])


WALK_DEFAULTS = {"union.many_window_log2": 30, "count.summary_skip": 1}


def every_slot(seg, p):
    """the ranges that name every slot, and the slots they name; of the 65537 slots of `big` the ones around its lists and the last two"""
    n = len(p.slots)
    if p.kind != "big":
        return [(seg, 0, n)], list(range(n))
    end = max(i for i, l in enumerate(p.slots) if len(l)) + 3
    return [(seg, 0, end), (seg, n - 2, n)], list(range(end)) + [n - 2, n - 1]


def one(seg, i):
    return [(seg, i, i + 1)]


def same(out, n, want):
    got = out.download(n)
    return n == want.size and got.dtype == np.uint32 and np.array_equal(got, want)


def paths_are(d, want, p):
    """the delta shows exactly `want`; a segment without a span mirror may fetch or bound its spans in addition"""
    rest = {k: v for k, v in d.items() if k not in want}
    return all(d.get(k) == v for k, v in want.items()) and (not rest or (not p.mirrored and set(rest) <= {"span.bounds", "span.fetch"}))


def batch_paths(prefix, classes):
    """the paths of a batch whose queries have these size classes: one launch per form taken, every large query on its own"""
    want = {prefix + ".pack": 1}
    for name, path in (("tiny", ".tiny"), ("small", ".small")):
        if name in classes:
            want[prefix + path] = 1
    if "large" in classes:
        want[prefix + ".single"] = classes.count("large")
    return want


def explain(ctx, seg, q, options):
    page = ctx.empty(q.page.size).upload(q.page)
    groups = [[(seg, a, b)] for a, b in q.explain_groups]
    try:
        with Options(ctx, options, WALK_DEFAULTS):
            masks, st = ctx.explain_ranges(groups, page, stats=True)
        got = masks.download(q.page.size).reshape(q.page.size, 1)
        assert got.dtype == np.uint64 and np.array_equal(got, q.explain_masks), (options, np.flatnonzero(got != q.explain_masks)[:8].tolist())
        assert (st.n_ids, st.n_hits, st.n_words) == (q.page.size, xc.popcount(q.explain_masks), 1), options
        masks.free()
        return st
    finally:
        page.free()


@pytest.mark.parametrize("kind", KINDS)
def test_explain_ranges(ctx, made, kind):
    seg, p, q = made(kind)
    for log2 in (30, 11):
        for skip in (1, 0):
            st = explain(ctx, seg, q, {"union.many_window_log2": log2, "count.summary_skip": skip})
            assert (st.n_windows == 1) == (log2 == 30), (log2, st.n_windows)


@pytest.mark.parametrize("kind", KINDS)
def test_explain_ranges_at_the_top_of_the_id_space(ctx, made, kind):
    seg, p, q = made(kind, "high")
    st = explain(ctx, seg, q, {"union.many_window_log2": 11})
    assert st.n_windows > 4


@pytest.mark.parametrize("kind", KINDS)
def test_histogram_ranges_in_windows_and_at_the_top_of_the_id_space(ctx, made, kind):
    from tests import hist_cases as hc
    seg, p, q = made(kind)
    R, named = every_slot(seg, p)
    lists = [p.slots[i] for i in named]
    edges = hc.uniform(3000, sk.SPAN - 5000, 50)
    dset = ctx.empty(q.dset.size).upload(q.dset)
    tomb = ctx.tombstones(q.removed)
    try:
        with Options(ctx, {"union.many_window_log2": 11}, WALK_DEFAULTS):
            got, st = ctx.histogram_ranges(R, edges, dset, q.dset.size, tomb=tomb)
            assert st.n_windows > 4 and np.array_equal(got, hc.truth(lists, q.dset, edges, q.removed))
            got, _ = ctx.histogram_ranges(R, edges, None, tomb=tomb)
            assert np.array_equal(got, hc.truth(lists, None, edges, q.removed))
    finally:
        dset.free()
        tomb.free()
    seg, p, q = made(kind, "high")
    R, named = every_slot(seg, p)
    lists = [p.slots[i] for i in named]
    dset = ctx.empty(q.dset.size).upload(q.dset)
    tomb = ctx.tombstones(q.removed)
    try:
        for t, removed in ((None, ()), (tomb, q.removed)):
            got, _ = ctx.histogram_ranges(R, q.top_edges, dset, q.dset.size, tomb=t)
            assert np.array_equal(got, hc.truth(lists, q.dset, q.top_edges, removed))
            got, _ = ctx.histogram_ranges(R, q.top_edges, None, tomb=t)
            want = hc.truth(lists, None, q.top_edges, removed)
            assert np.array_equal(got, want)
            assert t is not None or (want[:, -1].sum() >= 1 and want.sum() == sum(len(l) for l in lists))      # 0xFFFFFFFF has a bucket of its own
    finally:
        dset.free()
        tomb.free()


@pytest.mark.parametrize("kind", KINDS)
def test_and_or_of_three_short_lists(ctx, made, kind):
    seg, p, q = made(kind)
    lists = [(seg, i) for i in q.trio]
    for order in (lists, lists[::-1]):
        with path_delta(ctx) as d:
            out, n = ctx.intersect(order)
        assert paths_are(d, {"and.small": 1}, p), d
        assert same(out, n, q.trio_and)
        out.free()
        with path_delta(ctx) as d:
            out, n = ctx.union(order)
        assert paths_are(d, {"or.small": 1}, p), d
        assert same(out, n, q.trio_or)
        out.free()


def results(out, off, want):
    got = out.download(int(off[-1])) if int(off[-1]) else np.empty(0, np.uint32)
    assert off.tolist() == np.cumsum([0] + [w.size for w in want]).tolist(), off
    for k, w in enumerate(want):
        assert got.dtype == np.uint32 and np.array_equal(got[int(off[k]):int(off[k + 1])], w), k


@pytest.mark.parametrize("kind", KINDS)
def test_query_batch(ctx, made, kind):
    seg, p, q = made(kind)
    s = p.slots
    queries = [("and", q.trio), ("or", q.trio), ("or", q.short), ("and", [q.trio[0], q.long])]
    want = [q.trio_and, q.trio_or, sk.union_of([s[i] for i in q.short]), np.intersect1d(s[q.trio[0]], s[q.long]).astype(np.uint32)]
    classes = [sk.size_class([s[i] for i in slots]) for _, slots in queries]
    assert classes[:3] == ["tiny", "tiny", "small"] and classes[3] == ("tiny" if kind == "merge_small" else "large")
    with path_delta(ctx) as d:
        out, off = ctx.query_batch([(op, [r for i in slots for r in one(seg, i)]) for op, slots in queries])
    batch = {k: v for k, v in d.items() if k.startswith("batch.")}
    rest = [k for k in d if not k.startswith("batch.")]
    assert batch == batch_paths("batch", classes), d
    # the fallback is one two-list AND through a single-query path; nothing else may show but an unmirrored segment's spans
    assert sum(d[k] for k in rest if k.startswith("and.")) == classes.count("large"), d
    assert all(k.startswith("and.") or (not p.mirrored and k in ("span.bounds", "span.fetch")) for k in rest), d
    results(out, off, want)
    assert 0 < want[3].size < len(s[q.trio[0]])
    out.free()


@pytest.mark.parametrize("kind", KINDS)
def test_query_batch_groups(ctx, made, kind):
    seg, p, q = made(kind)
    s = p.slots
    (groups, exclude), answer = q.gq
    wider = [groups[0] + [q.long], groups[1]]
    t0, t1, t2 = (s[i] for i in q.trio)
    want = [answer, np.setdiff1d(np.intersect1d(sk.union_of([t0, t1, s[q.long]]), t2), s[q.not_slot]).astype(np.uint32)]
    as_ranges = lambda gs: [[r for i in g for r in one(seg, i)] for g in gs]
    classes = [sk.size_class([s[i] for g in gs + exclude for i in g]) for gs in (groups, wider)]
    assert classes[0] == "tiny" and classes[1] == ("small" if kind == "merge_small" else "large")
    with path_delta(ctx) as d:
        out, off = ctx.query_batch_groups([(as_ranges(groups), as_ranges(exclude)), (as_ranges(wider), as_ranges(exclude))])
    assert {k: v for k, v in d.items() if k.startswith("gbatch.")} == batch_paths("gbatch", classes), d
    general = [k for k in d if not k.startswith("gbatch.") and not k.startswith("span.")]
    assert bool(general) == ("large" in classes) and (p.mirrored is False or not [k for k in d if k.startswith("span.")]), d
    results(out, off, want)
    assert want[0].size < want[1].size
    out.free()


@pytest.mark.parametrize("kind", KINDS)
def test_topk_batch_and_explain_batch_of_its_pages(ctx, made, kind):
    seg, p, q = made(kind)
    s = p.slots
    slot_groups = [[[i] for i in q.short], [[i] for i in q.trio], [[i] for i in q.short] + [[q.long]]]
    classes = [sk.size_class([s[i] for g in gs for i in g]) for gs in slot_groups]
    assert classes[:2] == ["small", "tiny"] and classes[2] == ("small" if kind == "merge_small" else "large")
    n_table, n_single = sum(c != "large" for c in classes), classes.count("large")
    want = [q.short_top] + [sk.ranked([[s[i] for i in g] for g in gs], 10) for gs in slot_groups[1:]]
    queries = [[[r for i in g for r in one(seg, i)] for g in gs] for gs in slot_groups]
    ids, scores, off, eligible, st = ctx.topk_batch([(g, None, 10, 1, []) for g in queries], stats=True)
    assert off.tolist() == [0, 10, 20, 30] and (st.n_tiny + st.n_small, st.n_single, st.n_empty) == (n_table, n_single, 0)
    assert (st.n_tiny > 0) == ("tiny" in classes) and (st.n_small > 0) == ("small" in classes)
    got_ids, got_scores = ids.download(30), scores.download(30)
    for k, (w_ids, w_scores, w_eligible) in enumerate(want):
        assert np.array_equal(got_ids[10 * k:10 * k + 10], w_ids) and np.array_equal(got_scores[10 * k:10 * k + 10], w_scores), k
        assert int(eligible[k]) == w_eligible, k
    masks, mask_off, xst = ctx.explain_batch(queries, ids, off, stats=True)          # the device ids and offsets, fed as they are
    truth = [xc.truth([[s[i] for i in g] for g in gs], w[0]) for gs, w in zip(slot_groups, want)]
    assert mask_off.tolist() == [0, 10, 20, 30] and all(t.shape == (10, 1) for t in truth)
    assert np.array_equal(masks.download(30), np.concatenate(truth).ravel())
    assert (xst.n_tiny + xst.n_small, xst.n_single, xst.n_empty) == (n_table, n_single, 0)
    assert (xst.n_rows, xst.n_words, xst.n_hits) == (30, 30, sum(xc.popcount(t) for t in truth))
    assert xst.n_hits == int(sum(int(w[1].sum()) for w in want))                       # a row's bits are its score
    for a in (ids, scores, masks):
        a.free()


@pytest.mark.parametrize("kind", KINDS)
def test_atleast_ranges_in_one_launch(ctx, made, kind):
    seg, p, q = made(kind)
    with Options(ctx, {"atleast.small": 1}, {"atleast.small": 1}):      # (the default, whatever a test before left)
        out, n, st = ctx.atleast_ranges([one(seg, i) for i in q.short], 2, stats=True)
    assert st.form == _lib.II2_ATLEAST_SMALL and same(out, n, q.short_atleast2)
    out.free()


@pytest.mark.parametrize("kind", KINDS)
def test_intersect_ranges_group_path(ctx, made, kind):
    seg, p, q = made(kind)
    groups = [one(seg, i) for i in q.trio] + [every_slot(seg, p)[0]]
    for options, path in ((PROBE, "ir.probe"), (MARK, "ir.mark")):
        with Options(ctx, options, {"intersect.ranges_mark": RANGES_MARK_DEFAULT}):
            with path_delta(ctx) as d:
                out, n = ctx.intersect_ranges(groups)
        assert d.get("ir.groups") == 1 and d.get(path) == 3, d
        rest = [k for k in d if k not in ("ir.groups", path)]
        assert len([k for k in rest if k.startswith("or.")]) <= 1 and sum(d[k] for k in rest if k.startswith("or.")) <= 1, d
        assert all(k.startswith("or.") or (not p.mirrored and k in ("span.bounds", "span.fetch")) for k in rest), d
        assert same(out, n, q.trio_and), path
        out.free()
