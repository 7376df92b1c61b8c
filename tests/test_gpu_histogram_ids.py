"""GPU: ii2_histogram_ids - the ids of an ascending device set per bucket of a value axis, minus the removed ones - against numpy
(tests/hist_cases.py).  Without tombstones one thread per bucket bisects the set; with them one wave per 64 ids finds each id's
bucket and a segmented sum leaves one atomic per run of equal buckets.  The two forms agree where the tombstones remove nothing."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import hist_cases as hc
from tests.gpu_util import ctx, sorted_unique  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF
TOP = hc.TOP


def want(ids, edges, removed=()):
    return hc.truth([ids], None, edges, removed)[0]


def both(ctx, ids, edges, removed):
    """the counts without tombstones, with tombstones that remove nothing of the set, and with `removed`"""
    ids = np.asarray(ids, np.uint32)
    d = ctx.empty(max(ids.size, 1)).upload(ids)
    plain = ctx.histogram_ids(d, ids.size, edges)
    miss = np.setdiff1d(np.asarray([3, 77, 100_001, 0xFFFFFFF0], np.uint32), ids)
    same = ctx.histogram_ids(d, ids.size, edges, tomb=ctx.tombstones(miss))
    assert plain.dtype == np.uint64 and plain.shape == (len(edges) - 1,)
    assert np.array_equal(plain, want(ids, edges)), (ids.size, len(edges))
    assert np.array_equal(same, plain), (ids.size, len(edges))
    got = ctx.histogram_ids(d, ids.size, edges, tomb=ctx.tombstones(np.asarray(removed, np.uint32)))
    assert np.array_equal(got, want(ids, edges, removed)), (ids.size, len(edges))
    return plain


def test_set_sizes_and_edge_families(ctx):
    rng = np.random.default_rng(81)
    D = 200_000
    removed = sorted_unique(rng, 20_000, D)
    edge_sets = [[0, TOP], [0, D]] + [hc.uniform(0, D, n) for n in (2, 63, 64, 65, 4096)] + [hc.uniform(30_000, 120_000, 5), [D + 5, D + 9, TOP]]
    for n_set in (0, 1, 63, 64, 65, 4097, 70_000):
        ids = sorted_unique(rng, n_set, D)
        for edges in edge_sets:
            got = both(ctx, ids, edges, removed)
            if edges[0] > D:
                assert not got.any()
    assert both(ctx, ids, edge_sets[-2], removed).sum() < ids.size                   # ids below and above the axis were dropped


def test_runs_across_and_inside_a_wave(ctx):
    ids = np.arange(1000, 1000 + 64 * 5, dtype=np.uint32)                           # five waves of consecutive ids
    removed = ids[::3]
    # a bucket that crosses the 64-id boundaries; runs of 1, 2 and 7 ids inside a wave; an edge exactly at a wave's first and last id
    for edges in ([0, 1030, 1100, 1300, 5000], list(range(1000, 1321)), hc.uniform(1000, 1320, 160), hc.uniform(999, 1322, 46),
                  [1000, 1064, 1127, 1128, 1192, 1320], [1010, 1011, 1200]):
        both(ctx, ids, edges, removed)
    sparse = np.asarray([5, 6, 7, 70, 71, 900, 901, 902, 903, 5000, 70_000, 70_001], np.uint32)
    for edges in ([0, 7, 71, 903, 70_001, TOP], [6, 7, 8, 900], [0, TOP]):
        both(ctx, sparse, edges, [6, 903, 70_001])


def test_top_of_the_id_space(ctx):
    ids = np.asarray([0, 1, 0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    for edges in ([0, TOP], [0, TOP - 1], [1, TOP - 2, TOP - 1, TOP], [TOP - 1, TOP], [TOP - 2, TOP - 1]):
        both(ctx, ids, edges, [0xFFFFFFFF, 1])
    d = ctx.empty(5).upload(ids)
    assert ctx.histogram_ids(d, 5, [0, TOP]).tolist() == [5] and ctx.histogram_ids(d, 5, [0, TOP - 1]).tolist() == [4]
    assert ctx.histogram_ids(d, 3, [0, TOP]).tolist() == [3]                        # n_set counts, not the array's size


def test_errors(ctx):
    ids = np.arange(10, 500, dtype=np.uint32)
    d = ctx.empty(ids.size).upload(ids)
    tomb = ctx.tombstones(np.asarray([11], np.uint32))

    def raw(edges, counts, cap, t=None, n_buckets=None):
        e = np.ascontiguousarray(np.asarray(edges, np.uint64)) if edges is not None else None
        return ctx.lib.ii2_histogram_ids(ctx.h, d.data_ptr(), ids.size, t.h if t else None, n_buckets if n_buckets is not None else len(edges) - 1,
                                         e.ctypes.data_as(_lib.u64p) if e is not None else None,
                                         counts.ctypes.data_as(_lib.u64p) if counts is not None else None, cap)

    buf = np.full(8, SENTINEL, np.uint64)
    edges = [0, 100, 200, 300, 1000]
    for t in (None, tomb):
        assert raw(edges, buf, 3, t) == -4                                          # II2_ECAPACITY
        assert raw(edges, None, 4, t) == -1
        for bad, rc in hc.BAD_EDGES:
            if len(bad) > 1:
                assert raw(bad, buf, 1 << 20, t) == rc, bad
        assert raw(None, buf, 8, t, n_buckets=2) == -1 and raw(edges, buf, 8, t, n_buckets=0) == -1
        assert np.all(buf == SENTINEL)
    assert raw(edges, buf, 4, tomb) == 0
    assert buf[:4].tolist() == [89, 100, 100, 200] and np.all(buf[4:] == SENTINEL)
    # a set that is not ascending: any counts, no fault, and the context goes on working
    shuffled = np.random.default_rng(82).permutation(np.arange(5000, dtype=np.uint32))
    ds = ctx.empty(shuffled.size).upload(shuffled)
    for t in (None, tomb):
        got = ctx.histogram_ids(ds, shuffled.size, hc.uniform(0, 5000, 64), tomb=t)
        assert got.shape == (64,)
    assert ctx.histogram_ids(d, ids.size, edges).tolist() == [90, 100, 100, 200]
