"""GPU: the readers of a segment's derived arrays - cnt, last_doc, blk_list, the host span mirror, a view's window - run on every
way of making a segment (tests/segment_kinds.py), against plain numpy.

The calls are a fixed handful chosen so that every derived array is really read (segment_kinds.queries):
  - the block-wise union in 2048-doc windows reads blk_list and last_doc for every block (a single window skips them);
  - the facet count walks blk_list for the counter of every block, its "every doc" form answers from the host count mirror;
  - the counting forms of the threshold and the ranked query share the union's mark kernels;
  - a two-list AND takes its path by the host counts, spans and last_doc;
  - a NOT clips excluded lists by their spans: one that misses the required span and one that touches it by a single doc;
  - a merge reads cnt, blk_list (batch tiles) and, for a view, its window."""
import numpy as np
import pytest

from tests import segment_kinds as sk
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = list(sk.KINDS)
II2_ATLEAST_COUNT = 2


@pytest.fixture(scope="module")
def made(ctx):
    """kind -> (segment, plan, queries): every kind's segment of the readers' shape, made once."""
    cache, keep = {}, []

    def get(kind):
        if kind not in cache:
            p = sk.plan(kind, sk.READER_SHAPE)
            seg, alive = sk.make(ctx, p)
            keep.extend(alive)
            cache[kind] = (seg, p, sk.queries(kind))
        return cache[kind]
    yield get
    for seg, _, _ in cache.values():
        seg.free()
    for s in keep:
        s.free()


@pytest.fixture(scope="module")
def tombs(ctx):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = ctx.tombstones(sk.queries(kind).removed)
        return cache[kind]
    yield get
    for t in cache.values():
        t.free()


def _same(out, n, want):
    got = out.download(n)
    return n == want.size and got.dtype == np.uint32 and np.array_equal(got, want)


@pytest.mark.parametrize("kind", KINDS)
def test_windowed_union_reads_block_owners_and_last_docs(ctx, made, tombs, kind):
    seg, p, q = made(kind)
    every = [(seg, 0, len(p.slots))]
    try:
        ctx.set_option("union.many", 1)
        ctx.set_option("union.many_window_log2", 11)
        with path_delta(ctx) as d:
            out, n = ctx.union_ranges(every)
        assert d["or.many"] == 1 and d["or.many_window"] > 4, d        # several windows: every block asks blk_list / last_doc
        assert _same(out, n, q.union)
        out, n = ctx.union_ranges(every, tomb=tombs(kind))
        assert _same(out, n, q.union_tomb)
        ctx.set_option("union.many_window_log2", 30)                   # once with the default window
        with path_delta(ctx) as d:
            out, n = ctx.union_ranges(every, tomb=tombs(kind))
        assert d["or.many_window"] == 1 and _same(out, n, q.union_tomb)
    finally:
        ctx.set_option("union.many", 0)
        ctx.set_option("union.many_window_log2", 30)


@pytest.mark.parametrize("kind", KINDS)
def test_facet_counts_per_list(ctx, made, tombs, kind):
    seg, p, q = made(kind)
    every = [(seg, 0, len(p.slots))]
    dset = ctx.empty(q.dset.size).upload(q.dset)
    counts, st = ctx.count_ranges(every, dset, tomb=tombs(kind))
    assert counts.dtype == np.uint64 and np.array_equal(counts, q.counts) and st.n_lists == len(p.slots)
    counts, st = ctx.count_ranges(every)                               # d_set = NULL, tomb = NULL: the host count mirror
    assert np.array_equal(counts, q.lens)
    dset.free()


@pytest.mark.parametrize("kind", KINDS)
def test_threshold_and_ranked_counting_forms(ctx, made, kind):
    seg, p, q = made(kind)
    groups = [[(seg, a, b)] for a, b in q.groups]
    try:
        ctx.set_option("atleast.small", 0)
        ctx.set_option("atleast.handoff", 0)
        out, n, st = ctx.atleast_ranges(groups, 2, stats=True)
        assert st.form == II2_ATLEAST_COUNT and _same(out, n, q.atleast2)
        ids, scores, n = ctx.topk_ranges(groups, 10)
        assert n == 10 and np.array_equal(ids.download(n), q.top_ids) and np.array_equal(scores.download(n), q.top_scores)
    finally:
        ctx.set_option("atleast.small", 1)
        ctx.set_option("atleast.handoff", 1)


@pytest.mark.parametrize("kind", KINDS)
def test_two_list_and_of_the_long_lists(ctx, made, kind):
    seg, p, q = made(kind)
    out, n = ctx.intersect([(seg, q.pair[0]), (seg, q.pair[1])])
    assert _same(out, n, q.pair_and)
    out, n = ctx.intersect([(seg, q.pair[1]), (seg, q.pair[0])])
    assert _same(out, n, q.pair_and)


@pytest.mark.parametrize("kind", KINDS)
def test_not_clips_excluded_lists_by_their_spans(ctx, made, kind):
    seg, p, q = made(kind)
    s = p.slots
    try:
        for small in (1, 0):                                           # the one-launch form and the general one
            ctx.set_option("andnot.small", small)
            r, e = q.miss                                              # the excluded list starts behind the required one: nothing leaves
            out, n = ctx.andnot_ranges([[(seg, r, r + 1)]], [[(seg, e, e + 1)]])
            assert _same(out, n, s[r]), small
            r, e = q.touch                                             # their spans share one doc, and that doc leaves
            out, n = ctx.andnot_ranges([[(seg, r, r + 1)]], [[(seg, e, e + 1)]])
            assert _same(out, n, s[r][:-1]), small
            out, n = ctx.andnot_ranges([[(seg, e, e + 1)]], [[(seg, r, r + 1)]])
            assert _same(out, n, s[e][1:]), small
    finally:
        ctx.set_option("andnot.small", 1)


@pytest.mark.parametrize("kind", KINDS)
def test_merge_with_a_plain_segment_of_the_same_slots(ctx, made, tombs, kind):
    seg, p, q = made(kind)
    other = ctx.encode(*sk.csr(q.other))
    want_off, want = sk.csr(q.merged)
    try:
        for segs in ([seg, other], [other, seg]):
            out_off, out_vals, st = ctx.merge(segs)
            assert st.n_out == want.size and np.array_equal(out_off.download(), want_off)
            assert np.array_equal(out_vals.download(int(st.n_out)), want)
        out_off, out_vals, st = ctx.merge([seg, other], tomb=tombs(kind))
        k_off, k_vals = sk.csr([np.setdiff1d(l, q.removed).astype(np.uint32) if len(l) else l for l in q.merged])
        assert np.array_equal(out_off.download(), k_off) and np.array_equal(out_vals.download(int(st.n_out)), k_vals)
    finally:
        other.free()


@pytest.mark.parametrize("kind", [k for k in KINDS if sk.KINDS[k][2]])
def test_whole_segment_entry_points_refuse_views(ctx, made, kind):
    from inverted_index_2_amd.engine import II2Error
    seg, p, q = made(kind)
    plain = ctx.encode_lists([[1, 2, 3]])
    for call in (lambda: ctx.seg_concat([seg, plain]), lambda: ctx.seg_concat([plain, seg]), lambda: ctx.seg_allgather(seg)):
        with pytest.raises(II2Error) as e:
            call()
        assert e.value.code == -1 and "view" in str(e.value)
    plain.free()
