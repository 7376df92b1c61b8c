"""GPU: ii2_explain_batch - many result pages explained in one call - against plain Python (tests/explain_batch_cases.py) AND word
for word against ii2_explain_ranges run per query, under (batch.explain, batch.tiny) = (1, 1), (1, 0), (0, 1), (0, 0).  Masks,
mask_off and stats are compared exactly; guard words around the rows keep their fill."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import explain_batch_cases as bc
from tests.gpu_util import ctx, path_delta, sorted_unique  # noqa: F401

pytestmark = pytest.mark.gpu

PATTERN = 0xA5A5A5A5DEADBEEF
GUARD = 8
OK, EINVAL, ECAPACITY, ERANGE = 0, -1, -4, -5
WHO = "ii2_explain_batch: "
FIELDS = [f[0] for f in _lib.ExplainBatchStats._fields_]
CASES = bc.cases()                                 # (built without the library: nothing is loaded while the tests are collected)
BY_NAME = {c.name: c for c in CASES}


class Options:
    def __init__(self, ctx, explain, tiny):
        self.ctx, self.values = ctx, {"batch.explain": explain, "batch.tiny": tiny}

    def __enter__(self):
        for k, v in self.values.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.values:
            self.ctx.set_option(k, 1)


def fields(st):
    return {f: getattr(st, f) for f in FIELDS}


def build(ctx, case):
    """the case's segments on the device (views through ii2_seg_select) and its queries over them"""
    segs = {s: ctx.encode_lists(lists) for s, lists in enumerate(case.segments) if s not in case.views}
    for v, (base, src) in case.views.items():
        segs[v] = ctx.select(segs[base], src)
    return [[[(segs[s], a, b) for s, a, b in g] for g in groups] for groups, _ in case.queries]


def explain_batch(ctx, queries, ids, ids_off, total):
    """(the packed words [total], mask_off, stats) of one call whose buffer has GUARD pattern words in front and behind"""
    d_ids = ctx.empty(max(ids.size, 1)).upload(ids)
    buf = ctx.empty(total + 2 * GUARD, np.uint64).upload(np.full(total + 2 * GUARD, PATTERN, np.uint64))
    view = ctx.empty(1, np.uint64)                 # the rows' place inside buf, as a DeviceArray that owns nothing
    view.free()
    view.ptr, view.count = buf.ptr + 8 * GUARD, total
    try:
        with path_delta(ctx) as d:
            _, off, st = ctx.explain_batch(queries, d_ids, ids_off, stats=True, out=view)
        assert d == {}                             # not a set operation: no kernel path
    finally:
        view.ptr = 0
    got = buf.download()
    assert np.all(got[:GUARD] == PATTERN) and np.all(got[GUARD + total:] == PATTERN), "words written around the rows"
    return got[GUARD:GUARD + total], off, st


def single(ctx, groups, ids):
    """ii2_explain_ranges on one query: its words, flat"""
    n_out = ids.size * ((len(groups) + 63) // 64)
    if not n_out:
        return np.empty(0, np.uint64)
    d_ids = ctx.empty(ids.size).upload(ids)
    return ctx.explain_ranges(groups, d_ids, ids.size).download(n_out)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case(ctx, case):
    queries = build(ctx, case)
    want, want_off = case.expect(), case.mask_off()
    ref = np.concatenate([single(ctx, g, np.asarray(ids, np.uint32)) for g, (_, ids) in zip(queries, case.queries)] + [np.empty(0, np.uint64)])
    assert np.array_equal(ref, want)               # the single call agrees with the model: one reference for all four runs
    for explain, tiny in bc.OPTIONS:
        with Options(ctx, explain, tiny):
            got, off, st = explain_batch(ctx, queries, case.all_ids(), case.ids_off(), int(want_off[-1]))
        assert off.tolist() == want_off.tolist(), (explain, tiny)
        assert got.dtype == np.uint64 and np.array_equal(got, want), (explain, tiny)
        assert fields(st) == case.stats(explain, tiny), (explain, tiny)


def test_stats_pinned_by_hand(ctx):
    case = BY_NAME["mixed"]
    queries = build(ctx, case)
    want = case.expect()
    hand = {(1, 1): (1, 3, 2, 3), (1, 0): (0, 4, 2, 3), (0, 1): (0, 0, 6, 3), (0, 0): (0, 0, 6, 3)}
    for (explain, tiny), kinds in hand.items():
        with Options(ctx, explain, tiny):
            got, off, st = explain_batch(ctx, queries, case.all_ids(), case.ids_off(), want.size)
        assert (st.n_tiny, st.n_small, st.n_single, st.n_empty) == kinds
        assert (st.n_rows, st.n_words, st.n_hits) == (1119, 1116, bc.popcount(want)) and np.array_equal(got, want)


def raw(ctx, query_first, group_first, ranges, d_ids, ids_off, d_masks, cap, mask_off=None, stats=None, n_queries=None):
    """the return code of one ii2_explain_batch call: the host arrays as lists or None (NULL), d_ids / d_masks DeviceArrays or None"""
    n = len(ranges)
    arr = lambda a: (C.c_uint64 * len(a))(*a) if a is not None else None
    segs = (C.c_void_p * max(n, 1))(*[s.h if s is not None else None for s, _, _ in ranges])
    first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
    end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
    if n_queries is None:
        n_queries = len(query_first) - 1
    return ctx.lib.ii2_explain_batch(ctx.h, n_queries, arr(query_first), arr(group_first), segs, first, end, d_ids.data_ptr() if d_ids is not None else None,
                                     arr(ids_off), d_masks.data_ptr() if d_masks is not None else None, cap,
                                     mask_off.ctypes.data_as(_lib.u64p) if mask_off is not None else None, C.byref(stats) if stats is not None else None)


def test_protocol(ctx):
    rng = np.random.default_rng(9101)
    lists = [sorted_unique(rng, 100, 20_000) for _ in range(10)]      # (query 0: 13 lists, 1300 postings)
    seg = ctx.encode_lists(lists)
    other = None
    pages = [rng.permutation(sorted_unique(rng, n, 20_000)).astype(np.uint32) for n in (30, 0, 50)]
    ids = np.concatenate(pages)
    d_ids = ctx.empty(ids.size).upload(ids)
    qf, gf, ioff = [0, 2, 3, 5], [0, 1, 3, 4, 5, 6], [0, 30, 30, 80]
    good = [(seg, 0, 4), (seg, 4, 5), (seg, 2, 10), (seg, 0, 1), (seg, 1, 3), (seg, 9, 10)]
    groups = [[lists[0:4], lists[4:5] + lists[2:10]], [lists[0:1]], [lists[1:3], lists[9:10]]]
    want = np.array([w for g, p in zip(groups, pages) for row in bc.rows(g, p) for w in row], np.uint64)
    total = want.size
    assert total == 80
    d_masks = ctx.empty(total, np.uint64)
    stats, mask_off = _lib.ExplainBatchStats(), np.zeros(4, np.uint64)

    def reset():
        d_masks.upload(np.full(total, PATTERN, np.uint64))
        stats.n_rows, stats.n_hits = 77, 78
        mask_off[:] = 99

    def untouched(off_too=True):
        return np.all(d_masks.download() == PATTERN) and (stats.n_rows, stats.n_hits) == (77, 78) and (not off_too or np.all(mask_off == 99))

    assert raw(ctx, qf, gf, good, d_ids, ioff, d_masks, total, mask_off, stats) == OK
    assert np.array_equal(d_masks.download(), want) and mask_off.tolist() == [0, 30, 30, 80]
    assert (stats.n_tiny, stats.n_small, stats.n_single, stats.n_empty, stats.n_rows, stats.n_words, stats.n_hits) == (2, 0, 0, 1, 80, 80, bc.popcount(want))
    reset()
    # one word short: masks and stats keep their fill, mask_off is filled
    assert raw(ctx, qf, gf, good, d_ids, ioff, d_masks, total - 1, mask_off, stats) == ECAPACITY
    assert untouched(off_too=False) and mask_off.tolist() == [0, 30, 30, 80]
    assert ctx.lib.ii2_last_error(ctx.h).decode().startswith(WHO)
    reset()
    # II2_EINVAL: the message names the query, nothing is written
    bad = {
        2: (qf, gf, good[:5] + [(seg, 10, 9)], ioff),                       # a range that ends before it begins
        0: (qf, gf, [(seg, 0, 11)] + good[1:], ioff),                       # ... that ends behind the segment
        1: (qf, gf, good[:3] + [(other, 0, 1)] + good[4:], ioff),           # no segment
    }
    for q, (a, b, ranges, c) in bad.items():
        assert raw(ctx, a, b, ranges, d_ids, c, d_masks, total, mask_off, stats) == EINVAL
        assert ctx.lib.ii2_last_error(ctx.h).decode().startswith(f"{WHO}query {q}: "), ctx.lib.ii2_last_error(ctx.h)
        assert untouched()
    for a, b, c, q in (([0, 2, 1, 5], gf, ioff, 1), ([1, 2, 3, 5], gf, ioff, 0), (qf, [1, 1, 3, 4, 5, 6], ioff, 0), (qf, [0, 1, 3, 2, 5, 6], ioff, 1),
                       (qf, gf, [0, 30, 29, 80], 1), (qf, gf, [1, 30, 30, 80], 0)):
        assert raw(ctx, a, b, good, d_ids, c, d_masks, total, mask_off, stats) == EINVAL, (a, b, c)
        assert ctx.lib.ii2_last_error(ctx.h).decode().startswith(f"{WHO}query {q}: "), ctx.lib.ii2_last_error(ctx.h)
        assert untouched()
    for a, b, c, di, dm in ((None, gf, ioff, d_ids, d_masks), (qf, None, ioff, d_ids, d_masks), (qf, gf, None, d_ids, d_masks)):
        assert raw(ctx, a, b, good, di, c, dm, total, mask_off, stats, n_queries=3) == EINVAL
        assert ctx.lib.ii2_last_error(ctx.h).decode().startswith(WHO) and untouched()
    assert raw(ctx, qf, gf, good, None, ioff, d_masks, total, mask_off, stats) == EINVAL          # ids is NULL
    assert ctx.lib.ii2_last_error(ctx.h).decode().startswith(f"{WHO}query 0: ") and untouched()
    assert raw(ctx, qf, gf, good, d_ids, ioff, None, total, mask_off, stats) == EINVAL            # masks is NULL
    assert untouched()
    # II2_ERANGE: too many queries (the arrays are not read), a query of too many ids (the pointer is not read)
    assert raw(ctx, qf, gf, good, d_ids, ioff, d_masks, total, mask_off, stats, n_queries=(1 << 20) + 1) == ERANGE and untouched()
    assert raw(ctx, qf, gf, good, d_ids, [0, 30, 30, 31 + _lib.II2_EXPLAIN_MAX_IDS], d_masks, 1 << 40, mask_off, stats) == ERANGE
    assert ctx.lib.ii2_last_error(ctx.h).decode().startswith(f"{WHO}query 2: ") and untouched()
    # 2^32 rows in all, none of them with a word to write: 257 queries of 2^24 ids and no group
    n = 257
    assert raw(ctx, [0] * (n + 1), [0], [], None, [q << 24 for q in range(n + 1)], None, 0, None, stats) == ERANGE and untouched()
    # no query: mask_off[0] = 0, everything else may be NULL
    with path_delta(ctx) as d:
        assert raw(ctx, None, None, [], None, None, None, 0, mask_off, None, n_queries=0) == OK and mask_off[0] == 0
        # queries without a word to write: the device pointers may be NULL
        assert raw(ctx, [0, 0, 2], gf[:3], good[:3], None, [0, 5, 5], None, 0, mask_off, stats) == OK
        assert mask_off[:3].tolist() == [0, 0, 0] and (stats.n_empty, stats.n_rows, stats.n_words, stats.n_hits) == (2, 5, 0, 0)
    assert d == {} and np.all(d_masks.download() == PATTERN)
    # mask_off and stats may be NULL; the context goes on working
    assert raw(ctx, qf, gf, good, d_ids, ioff, d_masks, total, None, None) == OK
    assert np.array_equal(d_masks.download(), want)


def test_scratch_stays_clean(ctx):
    rng = np.random.default_rng(9102)
    D = 200_000
    lists = [sorted_unique(rng, int(rng.integers(1, 200)), D) for _ in range(80)]
    seg = ctx.encode_lists(lists)
    queries = [[[(seg, 10 * q + 2 * g, 10 * q + 2 * g + 2)] for g in range(5)] for q in range(8)]
    pages = [rng.permutation(np.union1d(lists[10 * q][:20], sorted_unique(rng, 30, D))).astype(np.uint32) for q in range(8)]
    want = np.array([w for q in range(8) for row in bc.rows([lists[10 * q + 2 * g:10 * q + 2 * g + 2] for g in range(5)], pages[q]) for w in row], np.uint64)
    off = np.cumsum([0] + [p.size for p in pages]).astype(np.uint64)
    got, _, st = explain_batch(ctx, queries, np.concatenate(pages), off, want.size)
    assert np.array_equal(got, want) and st.n_tiny == 8 and st.n_hits == bc.popcount(want) > 0
    # the per-context doc bitmap was not touched: a many-list union and a single explain on the same context are right
    with path_delta(ctx) as d:
        out, n = ctx.union_ranges([(seg, 0, 80)])
    assert d.get("or.many") == 1, d
    assert np.array_equal(out.download(n), np.unique(np.concatenate(lists)))
    assert np.array_equal(single(ctx, queries[3], pages[3]), want[int(off[3]):int(off[4])])
    got, _, _ = explain_batch(ctx, queries, np.concatenate(pages), off, want.size)       # ... and nothing of those two is left either
    assert np.array_equal(got, want)


def test_explains_the_pages_of_topk_batch(ctx):
    rng = np.random.default_rng(9103)
    lists = [sorted_unique(rng, int(n), 6000) for n in rng.integers(50, 600, 24)]
    seg = ctx.encode_lists(lists)
    weights = [[3, 1, 7, 2], [5, 5, 1], [1, 2, 4, 8, 16]]
    groups = [[[(seg, 0, 2)], [(seg, 2, 3)], [(seg, 3, 6)], [(seg, 6, 8)]],
              [[(seg, 8, 9)], [(seg, 9, 12)], [(seg, 12, 13)]],
              [[(seg, 13 + 2 * g, 15 + 2 * g)] for g in range(5)]]
    d_ids, d_scores, off, _ = ctx.topk_batch([(g, w, 40, 1, []) for g, w in zip(groups, weights)])
    assert off.tolist() == [0, 40, 80, 120]
    scores = d_scores.download(120)
    masks, mask_off = ctx.explain_batch(groups, d_ids, off)                   # ids and offsets fed straight in
    assert mask_off.tolist() == [0, 40, 80, 120]
    words = masks.download(120)
    for q in range(3):
        for i in range(int(off[q]), int(off[q + 1])):
            assert sum(w for g, w in enumerate(weights[q]) if (int(words[i]) >> g) & 1) == scores[i], (q, i)
            assert int(words[i]) >> len(weights[q]) == 0
