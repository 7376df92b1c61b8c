"""GPU: ii2_histogram_ranges - per list of any number of list ranges and per bucket of a value axis, the ids that lie in a doc set
and are not removed - against numpy: np.searchsorted over the edges of the ids that np.isin keeps (tests/hist_cases.py: truth).
All comparisons are exact.  The sizes are the smallest at which the kernels can go wrong: block and wave edges, edges on ids,
every sink (WHOLE / SPLIT / WIDE) with the blocks that ii2_hist_block sends there, runs of blocks in a wave, windows, the top
of the id space."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib, hist_block
from tests import hist_cases as hc
from tests import segment_kinds as sk
from tests.gpu_util import ctx, sorted_unique  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF
TOP = hc.TOP
ALL = [0, TOP]


def device_set(ctx, ids):
    ids = np.asarray(ids, np.uint32)
    return ctx.empty(max(ids.size, 1)).upload(ids), ids.size


def hist(ctx, ranges, ids, edges, tomb=None):
    if ids is None:
        return ctx.histogram_ranges(ranges, edges, None, tomb=tomb)
    d, n = device_set(ctx, ids)
    return ctx.histogram_ranges(ranges, edges, d, n, tomb=tomb)


def block_bounds(lists):
    """(first doc, bound of the last doc) of every DV1 block of the lists: inside a list the bound is the next block's first doc,
    at its end the list's last doc - what the skip tables say about a block without reading it"""
    lo, hi = [], []
    for l in lists:
        l = np.asarray(l, np.int64)
        if not l.size:
            continue
        first = l[::256]
        lo.append(first)
        hi.append(np.append(first[1:], l[-1]))
    return np.concatenate(lo), np.concatenate(hi)


def kinds(lists, edges, ids=None):
    """(n_whole, n_split, n_wide) of a call that skips no block for the summary's sake: every block whose bounds meet the docs
    that can hit - the lists' span, clipped to the set's (ids) and to the axis - goes where ii2_hist_block says"""
    lo, hi = block_bounds(lists)
    a, z = max(int(lo.min()), edges[0]), min(int(hi.max()), edges[-1] - 1)
    if ids is not None:
        a, z = max(a, int(ids[0])), min(z, int(ids[-1]))
    n = [0, 0, 0, 0]
    for f, u in zip(lo.tolist(), hi.tolist()):
        if a <= z and f <= z and u >= a:
            n[hist_block(edges, f, u)[0]] += 1
    assert n[hc.SKIP] == 0
    return n[hc.WHOLE], n[hc.SPLIT], n[hc.WIDE]


class Option:
    def __init__(self, ctx, name, value, default):
        self.ctx, self.name, self.value, self.default = ctx, name, value, default

    def __enter__(self):
        self.ctx.set_option(self.name, self.value)

    def __exit__(self, *exc):
        self.ctx.set_option(self.name, self.default)


def raw(ctx, ranges, d_set, n_set, edges, counts, cap, stats=None, n_buckets=None):
    """the return code of one ii2_histogram_ranges call into the numpy array `counts` (None: NULL) with capacity `cap`"""
    n = len(ranges)
    segs = (C.c_void_p * max(n, 1))(*[s.h if s is not None else None for s, _, _ in ranges])
    first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
    end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
    e = np.ascontiguousarray(np.asarray(edges, np.uint64)) if edges is not None else None
    cp = counts.ctypes.data_as(_lib.u64p) if counts is not None else None
    nb = n_buckets if n_buckets is not None else len(edges) - 1
    return ctx.lib.ii2_histogram_ranges(ctx.h, n, segs, first, end, d_set.data_ptr() if d_set is not None else None, n_set, None, nb,
                                        e.ctypes.data_as(_lib.u64p) if e is not None else None, cp, cap, C.byref(stats) if stats is not None else None)


def test_hand_case(ctx):
    lists = [np.asarray([1, 5, 9, 300], np.uint32), np.asarray([2, 5, 7], np.uint32), np.asarray([9, 300, 70000], np.uint32)]
    seg = ctx.encode_lists(lists)
    ids = [1, 5, 8, 9, 300, 70000]
    edges = [0, 6, 10, 301, TOP]
    got, st = hist(ctx, [(seg, 0, 3)], ids, edges)
    assert got.dtype == np.uint64 and got.shape == (3, 4)
    assert got.tolist() == [[2, 1, 1, 0], [1, 0, 0, 0], [0, 1, 1, 1]]
    assert (st.n_lists, st.n_blocks, st.n_hits, st.n_windows, st.n_buckets) == (3, 3, 8, 1, 4)
    assert st.n_decoded == st.n_whole + st.n_split + st.n_wide <= 3 and st.n_whole == 0 and st.n_wide == 0
    got, st = hist(ctx, [(seg, 0, 3)], ids, edges, ctx.tombstones(np.asarray([5, 300, 4], np.uint32)))
    assert got.tolist() == [[1, 1, 0, 0], [0, 0, 0, 0], [0, 1, 0, 1]] and st.n_hits == 4
    assert np.array_equal(got, hc.truth(lists, ids, edges, [5, 300, 4]))


def test_block_and_wave_edges_and_set_sizes(ctx):
    rng = np.random.default_rng(61)
    D = 60_000
    lists = [sorted_unique(rng, n, D) for n in (1, 255, 256, 257, 511, 513, 1025)]
    seg = ctx.encode_lists(lists)
    R = [(seg, 0, len(lists))]
    removed = sorted_unique(rng, 3000, D)
    tomb = ctx.tombstones(removed)
    edge_sets = [ALL, [0, D]] + [hc.uniform(0, D, n) for n in (2, 63, 64, 65)] + [hc.uniform(7000, 41_000, 5)]
    sets = {}
    for n_set in (0, 1, 63, 64, 65, 4097):
        ids = sorted_unique(rng, n_set, D)
        if n_set == 1:
            ids = lists[4][100:101]                                      # a single id that does hit
        sets[n_set] = (ids, device_set(ctx, ids))
    for edges in edge_sets:
        for n_set, (ids, (d, n)) in sets.items():
            got, st = ctx.histogram_ranges(R, edges, d, n)
            assert np.array_equal(got, hc.truth(lists, ids, edges)), (n_set, len(edges))
            assert st.n_hits == int(got.sum()) and st.n_lists == len(lists) and st.n_blocks == 15 and st.n_buckets == len(edges) - 1
            assert st.n_decoded == st.n_whole + st.n_split + st.n_wide
            got, _ = ctx.histogram_ranges(R, edges, d, n, tomb=tomb)
            assert np.array_equal(got, hc.truth(lists, ids, edges, removed)), (n_set, len(edges))
    inside = hc.truth(lists, sets[4097][0], edge_sets[-1])
    assert 0 < inside.sum() < hc.truth(lists, sets[4097][0], ALL).sum()       # ids below and above the axis were dropped
    # an axis that misses all lists: zeros, nothing decoded
    for edges in ([D + 10, D + 20, TOP], [TOP - 5, TOP]):
        for ids in (sets[4097][0], None):
            got, st = hist(ctx, R, ids, edges)
            assert not got.any() and got.shape == (len(lists), len(edges) - 1)
            assert (st.n_decoded, st.n_hits, st.n_windows, st.n_blocks, st.n_buckets) == (0, 0, 0, 15, len(edges) - 1)


def test_edges_on_ids(ctx):
    rng = np.random.default_rng(62)
    lists = [sorted_unique(rng, n, 30_000) + 100 for n in (700, 513, 300)]
    seg = ctx.encode_lists(lists)
    ids = np.unique(np.concatenate([l[::2] for l in lists] + [lists[0][255:258], lists[1][510:513]])).astype(np.uint32)
    firsts = [int(l[256 * k]) for l in lists for k in range((len(l) + 255) // 256)]
    lasts = [int(l[min(256 * (k + 1), len(l)) - 1]) for l in lists for k in range((len(l) + 255) // 256)]
    for name, at in (("first id", firsts), ("last id", lasts), ("last id + 1", [x + 1 for x in lasts])):
        edges = sorted(set([0] + at + [TOP]))
        for dset in (ids, None):
            got, st = hist(ctx, [(seg, 0, 3)], dset, edges)
            assert np.array_equal(got, hc.truth(lists, dset, edges)), name
        # a neighbour pair around every edge: each id on its own side
        for e in at[:4]:
            pair = [e - 1, e]
            got, _ = hist(ctx, [(seg, 0, 3)], np.asarray(pair, np.uint32), [0, e, TOP])
            assert np.array_equal(got, hc.truth(lists, pair, [0, e, TOP])), (name, e)


def test_every_sink(ctx):
    rng = np.random.default_rng(63)
    run = np.arange(5000, 5600, dtype=np.uint32)                         # 600 consecutive ids: 3 blocks
    lists = [run, sorted_unique(rng, 2000, 100_000), sorted_unique(rng, 300, 3000) + 5000, np.arange(64, dtype=np.uint32) * 3 + 9000]
    seg = ctx.encode_lists(lists)
    R = [(seg, 0, len(lists))]
    ids = np.unique(np.concatenate([run[::3], lists[1][::2], lists[2], lists[3]])).astype(np.uint32)
    width1 = list(range(5000, 5601))                                     # WIDE for the run's full blocks
    cases = {
        "width 1": width1,
        "64 buckets": hc.uniform(5000, 5000 + 64 * 4, 64),               # the run's first block meets exactly 64: SPLIT
        "65 buckets": hc.uniform(5000, 5000 + 65 * 4 - 4, 64) + [5000 + 65 * 4],
        "coarse": [0, 4000, 9000, 50_000, TOP],
        "uniform 4096": hc.uniform(0, 100_000, 4096),
    }
    seen = np.zeros(3, np.int64)
    for name, edges in cases.items():
        want = hc.truth(lists, ids, edges)
        # every doc: every block that meets the axis is decoded
        got, st = hist(ctx, R, None, edges)
        assert np.array_equal(got, hc.truth(lists, None, edges)), name
        assert (st.n_whole, st.n_split, st.n_wide) == kinds(lists, edges), name
        seen += (st.n_whole, st.n_split, st.n_wide)
        with Option(ctx, "count.summary_skip", 0, 1):
            got, st = hist(ctx, R, ids, edges)
            assert np.array_equal(got, want), name
            assert (st.n_whole, st.n_split, st.n_wide) == kinds(lists, edges, ids), name
            with Option(ctx, "hist.whole", 0, 1):
                got0, st0 = hist(ctx, R, ids, edges)
                assert np.array_equal(got0, want) and st0.n_whole == 0, name
                assert st0.n_split == st.n_whole + st.n_split and st0.n_wide == st.n_wide
        with Option(ctx, "hist.whole", 0, 1):
            got0, st0 = hist(ctx, R, ids, edges)                        # with the summary skip
            assert np.array_equal(got0, want) and st0.n_whole == 0, name
    assert np.all(seen > 0), seen
    assert kinds([run], width1)[2] == 3 and hist_block(cases["64 buckets"], 5000, 5256) == (hc.SPLIT, 0, 63)
    assert hist_block(cases["65 buckets"], 5000, 5256)[0] == hc.WIDE


def test_runs_of_blocks_in_a_wave(ctx):
    # lists of 1 .. 5 blocks, ids 3 apart: block k of a list at `base` starts at base + 768 k
    bases = [0, 1000, 4000, 9000, 15_000, 15_000 + 768 * 2 + 3, 30_000]
    blocks = [1, 2, 3, 4, 5, 2, 1]
    lists = [(np.arange(256 * n - 5, dtype=np.uint32) * 3 + b) for b, n in zip(bases, blocks)]
    seg = ctx.encode_lists(lists)
    R = [(seg, 0, len(lists)), (seg, 2, 4)]
    named = lists + lists[2:4]
    rng = np.random.default_rng(64)
    ids = np.unique(np.concatenate([l[rng.random(l.size) < 0.6] for l in lists])).astype(np.uint32)
    edge_sets = {
        "one": [0, 40_000],                                              # WHOLE -> WHOLE, same bucket; list change inside a bucket
        "per list": [0, 900, 3900, 8900, 14_900, 29_000, 40_000],        # WHOLE -> WHOLE, next bucket, at a list change
        "mid block": [0, 4000 + 768 + 300, 4000 + 768 * 2, 9000 + 768 * 2 + 10, 9000 + 768 * 2 + 20, 15_000 + 768 * 3, 40_000],      # WHOLE -> SPLIT -> WHOLE
        "narrow": hc.uniform(9000, 12_000, 700),                         # WIDE in the middle of a run, the axis inside the docs
    }
    removed = ids[::7]
    tomb = ctx.tombstones(removed)
    for name, edges in edge_sets.items():
        want, want_t, want_all = hc.truth(named, ids, edges), hc.truth(named, ids, edges, removed), hc.truth(named, None, edges, removed)
        seq = [hist_block(edges, f, u)[0] for f, u in zip(*map(np.ndarray.tolist, block_bounds(lists)))]
        if name == "mid block":
            assert any(seq[i:i + 3] == [hc.WHOLE, hc.SPLIT, hc.WHOLE] for i in range(len(seq)))
        if name == "narrow":
            assert hc.WIDE in seq and hc.SKIP in seq
        stats = []
        for per_wave in (0, 1, 2, 3, 16):
            with Option(ctx, "hist.per_wave", per_wave, 0), Option(ctx, "count.summary_skip", 0, 1):
                got, st = hist(ctx, R, ids, edges)
                assert np.array_equal(got, want), (name, per_wave)
                stats.append((st.n_whole, st.n_split, st.n_wide))
                got, _ = hist(ctx, R, ids, edges, tomb)
                assert np.array_equal(got, want_t), (name, per_wave)
                got, _ = hist(ctx, R, None, edges, tomb)
                assert np.array_equal(got, want_all), (name, per_wave)
        assert len(set(stats)) == 1 and stats[0] == kinds(named, edges, ids), (name, stats)


def test_a_counter_that_is_the_sum_of_many_atomics(ctx):
    rng = np.random.default_rng(65)
    long_list = sorted_unique(rng, 40_000, 300_000) + 1000
    seg = ctx.encode_lists([long_list, long_list[::50]])
    ids = long_list[rng.random(long_list.size) < 0.7]
    edges = [0, 1000, 400_000, TOP]
    with Option(ctx, "hist.per_wave", 1, 0):
        got, st = hist(ctx, [(seg, 0, 2)], ids, edges)
        assert np.array_equal(got, hc.truth([long_list, long_list[::50]], ids, edges))
        assert got[0, 1] == ids.size > 25_000 and st.n_whole > 150 and st.n_split == 0
        got, st = hist(ctx, [(seg, 0, 2)], None, edges)
        assert got[0].tolist() == [0, 40_000, 0] and st.n_whole == 157 + 4


def test_windows(ctx):
    rng = np.random.default_rng(66)
    special = np.asarray([2047, 2048, 65535, 65536, 199_999], np.uint32)
    lists = [np.union1d(sorted_unique(rng, int(rng.integers(1, 1500)), 200_000), special[k % 2::2]).astype(np.uint32) for k in range(12)]
    seg = ctx.encode_lists(lists)
    R = [(seg, 0, len(lists))]
    ids = np.union1d(sorted_unique(rng, 30_000, 200_000), special).astype(np.uint32)
    removed = np.union1d(sorted_unique(rng, 5000, 200_000), special[1:2]).astype(np.uint32)
    tomb = ctx.tombstones(removed)
    edge_sets = [ALL, [0, 2048, 65536, 200_000], hc.uniform(1000, 150_000, 100)]
    one = {}
    for k, edges in enumerate(edge_sets):
        one[k], st = hist(ctx, R, ids, edges)
        assert st.n_windows == 1 and np.array_equal(one[k], hc.truth(lists, ids, edges))
    try:
        for log2 in (11, 12):
            ctx.set_option("union.many_window_log2", log2)
            W = 1 << log2
            for k, edges in enumerate(edge_sets):
                got, st = hist(ctx, R, ids, edges)
                assert np.array_equal(got, one[k]), (log2, k)
                lo = max(min(int(l[0]) for l in lists), int(ids[0]), edges[0])
                hi = min(max(int(l[-1]) for l in lists), int(ids[-1]), edges[-1] - 1)
                assert st.n_windows == (hi - (lo & ~2047)) // W + 1, (log2, k)
            got, _ = hist(ctx, R, ids, edge_sets[1], tomb)
            assert np.array_equal(got, hc.truth(lists, ids, edge_sets[1], removed)), log2
    finally:
        ctx.set_option("union.many_window_log2", 30)


def test_top_of_the_id_space(ctx):
    lists = [np.asarray([0, 5, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32), np.asarray([0xFFFFFFFF], np.uint32), np.asarray([7, 0xFFFFFFFE], np.uint32)]
    seg = ctx.encode_lists(lists)
    ids = np.asarray([0, 7, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)
    for last in (TOP, TOP - 1):
        for edges in ([0, last], [0, 6, TOP - 2, last], [TOP - 2, last], [5, TOP - 3, TOP - 2, last]):
            for dset in (ids, None):
                got, st = hist(ctx, [(seg, 0, 3)], dset, edges)
                assert np.array_equal(got, hc.truth(lists, dset, edges)), (last, edges, dset is None)
    got, _ = hist(ctx, [(seg, 0, 3)], None, [TOP - 2, TOP - 1, TOP])
    assert got.tolist() == [[1, 1], [0, 1], [1, 0]]
    got, _ = hist(ctx, [(seg, 0, 3)], ids, [0, TOP])
    assert got[:, 0].tolist() == [3, 1, 2]
    got, _ = hist(ctx, [(seg, 0, 3)], ids, [0, TOP - 1])
    assert got[:, 0].tolist() == [2, 0, 2]                                  # 0xFFFFFFFF lies outside [0, 2^32 - 1)
    got, _ = hist(ctx, [(seg, 0, 3)], ids, [0, TOP], ctx.tombstones(np.asarray([0xFFFFFFFF], np.uint32)))
    assert got[:, 0].tolist() == [2, 0, 2]


def test_ranges(ctx):
    rng = np.random.default_rng(67)
    D = 200_000
    mk = lambda k, lo=1, hi=2000: [sorted_unique(rng, int(rng.integers(lo, hi)), D) for _ in range(k)]
    A, B, S = mk(30), mk(12), mk(8)
    B[3] = np.empty(0, np.uint32)
    B[11] = np.empty(0, np.uint32)
    segA, segB = ctx.encode_lists(A), ctx.encode_lists(B)
    src = [0, -1, 1, 2, -1, -1, 3] + list(range(4, 8)) + [-1]
    base = ctx.encode_lists(S)
    segV = ctx.select(base, src)                                        # a view with empty slots
    V = [S[j] if j >= 0 else np.empty(0, np.uint32) for j in src]
    ranges = [(segA, 0, 20), (segB, 0, 12), (segA, 10, 11),              # two segments; list 10 of A named twice
              (segV, 0, len(src)), (segA, 7, 7), (segV, 4, 6), (segA, 25, 30)]      # an empty range, a range of empty lists
    named = A[0:20] + B + A[10:11] + V + V[4:6] + A[25:30]
    ids = sorted_unique(rng, 40_000, D)
    removed = sorted_unique(rng, 10_000, D)
    for edges in (ALL, hc.uniform(0, D, 24), hc.uniform(30_000, 90_000, 7)):
        got, st = hist(ctx, ranges, ids, edges)
        assert got.shape == (len(named), len(edges) - 1) and np.array_equal(got, hc.truth(named, ids, edges))
        assert np.array_equal(got[10], got[32]) and st.n_lists == len(named)
        got, _ = hist(ctx, ranges, ids, edges, ctx.tombstones(removed))
        assert np.array_equal(got, hc.truth(named, ids, edges, removed))
    got, st = hist(ctx, [(segV, 4, 6), (segB, 3, 4)], ids, [0, 10, 20])      # only empty lists: zeros without a launch
    assert got.shape == (3, 2) and not got.any() and st.n_windows == 0 and st.n_blocks == 0
    got, st = hist(ctx, [], ids, [0, 10, 20])
    assert got.shape == (0, 2) and st.n_lists == 0


@pytest.mark.parametrize("kind", list(sk.KINDS))
def test_segment_kinds(ctx, kind):
    """every way of making a segment (tests/test_gpu_segment_kinds_readers.py has the same call in windows and at the top of the id space)"""
    p = sk.plan(kind, sk.READER_SHAPE)
    q = sk.queries(kind)
    seg, keep = sk.make(ctx, p)
    edges = hc.uniform(3000, sk.SPAN - 5000, 50)
    n = len(p.slots)
    R, named = [(seg, 0, n)], p.slots
    if kind == "big":                                                   # of its 65537 slots the ones around its lists and the last two
        end = max(i for i, l in enumerate(p.slots) if len(l)) + 3
        R, named = [(seg, 0, end), (seg, n - 2, n)], p.slots[:end] + p.slots[n - 2:]
    try:
        got, _ = hist(ctx, R, q.dset, edges, ctx.tombstones(q.removed))
        assert np.array_equal(got, hc.truth(named, q.dset, edges, q.removed))
        got, _ = hist(ctx, R, None, edges)
        assert np.array_equal(got, hc.truth(named, None, edges))
    finally:
        seg.free()
        for s in keep:
            s.free()


def test_equivalences(ctx):
    rng = np.random.default_rng(68)
    D = 500_000
    lists = [sorted_unique(rng, int(n), D) for n in rng.integers(1, 5000, 40)]
    seg = ctx.encode_lists(lists)
    R = [(seg, 0, 40), (seg, 5, 9)]
    ids = sorted_unique(rng, 60_000, D)
    d, n = device_set(ctx, ids)
    tomb = ctx.tombstones(sorted_unique(rng, 20_000, D))
    for t in (None, tomb):
        want, cst = ctx.count_ranges(R, d, n, tomb=t)
        got, st = ctx.histogram_ranges(R, ALL, d, n, tomb=t)
        assert np.array_equal(got[:, 0], want) and st.n_hits == cst.n_hits and st.n_decoded == cst.n_decoded and st.n_windows == cst.n_windows
        # any partition of an axis: the row sums are the count of the set clipped to the axis
        lo, hi = 100_000, 400_000
        clipped = ids[(ids >= lo) & (ids < hi)]
        dc, nc = device_set(ctx, clipped)
        want, _ = ctx.count_ranges(R, dc, nc, tomb=t)
        for edges in ([lo, hi], hc.uniform(lo, hi, 24), sorted(set([lo, hi] + rng.integers(lo, hi, 300).tolist()))):
            got, _ = ctx.histogram_ranges(R, edges, d, n, tomb=t)
            assert np.array_equal(got.sum(axis=1), want), len(edges)


def test_every_doc(ctx):
    rng = np.random.default_rng(69)
    lists = [sorted_unique(rng, n, 300_000) for n in (1, 256, 257, 5000, 0, 70_000, 3)]
    seg = ctx.encode_lists(lists)
    ranges = [(seg, 0, len(lists)), (seg, 3, 4)]
    named = lists + lists[3:4]
    removed = np.union1d(sorted_unique(rng, 50_000, 300_000), lists[6]).astype(np.uint32)
    tomb = ctx.tombstones(removed)
    for edges in (ALL, hc.uniform(0, 300_000, 256), hc.uniform(10_000, 250_000, 13)):
        got, st = hist(ctx, ranges, None, edges)
        assert np.array_equal(got, hc.truth(named, None, edges)) and st.n_windows == 0
        assert (st.n_whole, st.n_split, st.n_wide) == kinds(named, edges)
        got, st = hist(ctx, ranges, None, edges, tomb)
        assert np.array_equal(got, hc.truth(named, None, edges, removed)) and not got[6].any()
    got, st = hist(ctx, ranges, None, ALL)
    assert got[:, 0].tolist() == [len(l) for l in named] and st.n_decoded == st.n_blocks == st.n_whole      # the walk runs


def test_errors_write_nothing(ctx):
    rng = np.random.default_rng(70)
    lists = [sorted_unique(rng, 500, 50_000) for _ in range(10)]
    seg = ctx.encode_lists(lists)
    d, n = device_set(ctx, sorted_unique(rng, 1000, 50_000))
    edges = [0, 100, 20_000, 50_000]
    buf = np.full(40, SENTINEL, np.uint64)
    stats = _lib.HistStats()
    stats.n_lists = 77
    R = [(seg, 0, 10)]
    assert raw(ctx, R, d, n, edges, buf, 29, stats) == -4              # II2_ECAPACITY: one cell short
    assert np.all(buf == SENTINEL) and stats.n_lists == 77
    for bad, rc in hc.BAD_EDGES:
        if len(bad) > 1:
            assert raw(ctx, R, d, n, bad, buf, 40, stats) == rc, bad
    assert raw(ctx, R, d, n, None, buf, 40, stats, n_buckets=3) == -1   # NULL edges
    assert raw(ctx, R, d, n, edges, buf, 40, stats, n_buckets=0) == -1  # no bucket
    for bad in ([(seg, 5, 4)], [(seg, 0, 11)], [(seg, 0, 3), (None, 0, 1)]):      # a bad range, a range past n_lists, no segment
        assert raw(ctx, bad, d, n, edges, buf, 40, stats) == -1
    assert raw(ctx, R, d, n, edges, None, 40, stats) == -1              # counts is NULL
    assert np.all(buf == SENTINEL) and stats.n_lists == 77
    assert raw(ctx, R, d, n, edges, buf, 30, stats) == 0                # exactly enough
    assert np.array_equal(buf[:30].reshape(10, 3), hc.truth(lists, d.download(n), edges)) and np.all(buf[30:] == SENTINEL)
    assert stats.n_lists == 10 and stats.n_buckets == 3
    # the cell limit: 4096 buckets x (2^14 + 1) lists named - a one-id list named over and over - is refused before any launch
    one = ctx.encode_lists([np.asarray([5], np.uint32)])
    many = [(one, 0, 1)] * ((1 << 14) + 1)
    wide = list(range(4097))
    assert raw(ctx, many, d, n, wide, buf, 1 << 40, stats) == -5        # II2_ERANGE
    assert np.all(buf[30:] == SENTINEL) and stats.n_lists == 10
    got, st = hist(ctx, many[:-1], np.asarray([5], np.uint32), wide)    # the limit itself is fine
    assert got.shape == (1 << 14, 4096) and got[:, 5].all() and int(got.sum()) == 1 << 14 == st.n_hits


def test_scratch_stays_clean(ctx):
    rng = np.random.default_rng(71)
    D = 400_000
    lists = [sorted_unique(rng, int(rng.integers(1, 3000)), D) for _ in range(80)]
    seg = ctx.encode_lists(lists)
    ids = sorted_unique(rng, 90_000, D)
    edges = hc.uniform(50_000, 350_000, 24)
    with Option(ctx, "union.many", 1, 0):
        got, _ = hist(ctx, [(seg, 0, 40)], ids, edges)
        assert np.array_equal(got, hc.truth(lists[:40], ids, edges))
        with Option(ctx, "hist.whole", 0, 1):
            got, _ = hist(ctx, [(seg, 0, 40)], ids, hc.uniform(0, D, 4096))
            assert np.array_equal(got, hc.truth(lists[:40], ids, hc.uniform(0, D, 4096)))
        out, n = ctx.union_ranges([(seg, 40, 80)])                     # the same bitmap: nothing of the set may be left in it
        assert np.array_equal(out.download(n), np.unique(np.concatenate(lists[40:80])))
        d, ns = device_set(ctx, ids[:5000])
        cnt, _ = ctx.count_ranges([(seg, 0, 80)], d, ns)               # ... and nothing of the union
        want = hc.truth(lists, ids[:5000], ALL)[:, 0]
        assert np.array_equal(cnt, want)
