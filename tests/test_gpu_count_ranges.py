"""GPU: ii2_count_ranges - per list of any number of list ranges, the ids that lie in a doc set and are not removed (facet
counts) - against numpy: np.isin per list, minus `removed`.  The sizes are the smallest at which the kernels can go wrong: block,
wave, word and chunk edges, more than one window, a list whose counter is the sum of many atomics."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from inverted_index_2_amd import Context, _lib
from tests.gpu_util import ctx, one_block_lists_past_a_wave, sorted_unique  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEFDEADBEEF


def truth(lists, ids, removed=()):
    """one count per list: its ids that lie in `ids` (None: every doc) and not in `removed`"""
    out = np.zeros(len(lists), np.uint64)
    for k, l in enumerate(lists):
        l = np.asarray(l, np.uint32)
        hit = np.ones(l.size, bool) if ids is None else np.isin(l, np.asarray(ids, np.uint32))
        out[k] = int(np.count_nonzero(hit & ~np.isin(l, np.asarray(removed, np.uint32))))
    return out


def device_set(ctx, ids):
    ids = np.asarray(ids, np.uint32)
    return ctx.empty(max(ids.size, 1)).upload(ids), ids.size


def count(ctx, ranges, ids, tomb=None):
    if ids is None:
        return ctx.count_ranges(ranges, None, tomb=tomb)
    d, n = device_set(ctx, ids)
    return ctx.count_ranges(ranges, d, n, tomb=tomb)


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


class Option:
    def __init__(self, ctx, name, value, default):
        self.ctx, self.name, self.value, self.default = ctx, name, value, default

    def __enter__(self):
        self.ctx.set_option(self.name, self.value)

    def __exit__(self, *exc):
        self.ctx.set_option(self.name, self.default)


def raw(ctx, ranges, d_set, n_set, counts, cap, stats=None):
    """the return code of one ii2_count_ranges call into the numpy array `counts` (None: NULL) with capacity `cap`"""
    n = len(ranges)
    segs = (C.c_void_p * max(n, 1))(*[s.h if s is not None else None for s, _, _ in ranges])
    first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
    end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
    cp = counts.ctypes.data_as(C.POINTER(C.c_uint64)) if counts is not None else None
    return ctx.lib.ii2_count_ranges(ctx.h, n, segs, first, end, d_set.data_ptr() if d_set is not None else None, n_set, None, cp, cap,
                                    C.byref(stats) if stats is not None else None)


def test_hand_case(ctx):
    lists = [np.asarray([1, 5, 9, 300], np.uint32), np.asarray([2, 5, 7], np.uint32), np.asarray([9, 300, 70000], np.uint32)]
    seg = ctx.encode_lists(lists)
    ids = [1, 5, 8, 9, 300, 70000]
    got, st = count(ctx, [(seg, 0, 3)], ids)
    assert got.dtype == np.uint64 and got.tolist() == [4, 1, 3]
    assert (st.n_lists, st.n_blocks, st.n_hits, st.n_windows) == (3, 3, 8, 1) and st.n_decoded <= 3
    got, st = count(ctx, [(seg, 0, 3)], ids, ctx.tombstones(np.asarray([5, 300, 4], np.uint32)))
    assert got.tolist() == [2, 0, 2] and st.n_hits == 4


def test_block_and_wave_edges_and_set_sizes(ctx):
    rng = np.random.default_rng(41)
    D = 60_000
    lists = [sorted_unique(rng, n, D) for n in (1, 255, 256, 257, 511, 513, 1025)]
    seg = ctx.encode_lists(lists)
    removed = sorted_unique(rng, 3000, D)
    tomb = ctx.tombstones(removed)
    for n_set in (0, 1, 63, 64, 65, 4097):
        ids = sorted_unique(rng, n_set, D)
        if n_set == 1:
            ids = lists[4][100:101]                                      # a single id that does hit
        got, st = count(ctx, [(seg, 0, len(lists))], ids)
        assert np.array_equal(got, truth(lists, ids)), n_set
        assert st.n_hits == int(got.sum()) and st.n_lists == len(lists) and st.n_blocks == 15
        assert st.n_windows == (1 if n_set else 0)
        got, _ = count(ctx, [(seg, 0, len(lists))], ids, tomb)
        assert np.array_equal(got, truth(lists, ids, removed)), n_set


def test_word_and_chunk_edges(ctx):
    edges = np.asarray([31, 32, 63, 64, 2047, 2048, 65535, 65536, 131071, 131072], np.uint32)
    near = np.asarray([30, 33, 62, 65, 2046, 2049, 65534, 65537, 131070, 131073], np.uint32)
    lists = [edges, edges[::2], edges[1::2], near, np.union1d(edges, near)]
    seg = ctx.encode_lists(lists)
    for skip in (1, 0):
        with Option(ctx, "count.summary_skip", skip, 1):
            # every edge id in the set only, in a list only, and in both, across the pairs of (set, list)
            for ids in (edges, edges[::2], edges[1::2], near, np.union1d(edges, near), edges[3:8]):
                got, _ = count(ctx, [(seg, 0, len(lists))], ids)
                assert np.array_equal(got, truth(lists, ids)), (skip, ids)
                rem = np.asarray([32, 2047, 65536, 131071], np.uint32)
                got, _ = count(ctx, [(seg, 0, len(lists))], ids, ctx.tombstones(rem))
                assert np.array_equal(got, truth(lists, ids, rem)), (skip, ids)


def test_one_long_list_among_many_short_ones(ctx):
    rng = np.random.default_rng(43)
    D = 1_000_000
    short = [np.asarray([int(x)], np.uint32) for x in rng.integers(0, D, 3000)]
    lists = short[:1500] + [sorted_unique(rng, 100_000, D)] + short[1500:]       # the long one in the middle of the range
    seg = ctx.encode_lists(lists)
    ids = sorted_unique(rng, 300_000, D)
    want = truth(lists, ids)
    for skip in (1, 0):
        with Option(ctx, "count.summary_skip", skip, 1):
            got, st = count(ctx, [(seg, 0, len(lists))], ids)
            assert np.array_equal(got, want), skip
            assert st.n_blocks == 3000 + 391 and st.n_hits == int(want.sum())
    assert want[1500] > 20_000 and 0 < np.count_nonzero(want[:1500]) < 1500       # many atomics into one counter, one into others


def test_ranges(ctx):
    rng = np.random.default_rng(44)
    D = 200_000
    mk = lambda k, lo=1, hi=2000: [sorted_unique(rng, int(rng.integers(lo, hi)), D) for _ in range(k)]
    A, B, S = mk(50), mk(20), mk(12)
    B[3] = np.empty(0, np.uint32)
    B[19] = np.empty(0, np.uint32)
    segA, segB = ctx.encode_lists(A), ctx.encode_lists(B)
    src = [0, -1, 1, 2, -1, -1, 3] + list(range(4, 12)) + [-1]
    base = ctx.encode_lists(S)
    segV = ctx.select(base, src)                                        # a view with empty slots
    V = [S[j] if j >= 0 else np.empty(0, np.uint32) for j in src]
    ranges = [(segA, 0, 30), (segB, 0, 20), (segA, 10, 11),              # two segments; list 10 of A named twice
              (segV, 0, len(src)), (segA, 7, 7), (segV, 4, 6), (segA, 40, 50)]      # an empty range, a range of empty lists
    named = A[0:30] + B + A[10:11] + V + V[4:6] + A[40:50]
    ids = sorted_unique(rng, 40_000, D)
    removed = sorted_unique(rng, 10_000, D)
    got, st = count(ctx, ranges, ids)
    assert got.size == len(named) and np.array_equal(got, truth(named, ids))
    assert got[10] == got[50] and st.n_lists == len(named)
    got, _ = count(ctx, ranges, ids, ctx.tombstones(removed))
    assert np.array_equal(got, truth(named, ids, removed))
    # capacity: exactly enough works (above); one too few is II2_ECAPACITY and writes nothing
    d, n = device_set(ctx, ids)
    buf = np.full(len(named), SENTINEL, np.uint64)
    stats = _lib.CountStats()
    stats.n_lists = 77
    assert raw(ctx, ranges, d, n, buf, len(named) - 1, stats) == -4
    assert np.all(buf == SENTINEL) and stats.n_lists == 77
    assert raw(ctx, ranges, d, n, buf, len(named), stats) == 0
    assert np.array_equal(buf, truth(named, ids)) and stats.n_lists == len(named)
    # no range, only empty ranges: nothing to write, counts may be NULL
    assert raw(ctx, [], d, n, None, 0) == 0
    assert raw(ctx, [(segA, 7, 7)], d, n, None, 0) == 0
    got, st = count(ctx, [(segV, 4, 6), (segB, 3, 4)], ids)               # only empty lists: zeros without a launch
    assert got.tolist() == [0, 0, 0] and st.n_windows == 0 and st.n_blocks == 0


def test_windows(ctx):
    rng = np.random.default_rng(45)
    lists = [sorted_unique(rng, int(rng.integers(1, 1500)), 10_000) + 777 for _ in range(40)]
    seg = ctx.encode_lists(lists)
    ids = sorted_unique(rng, 3000, 10_500) + 500
    removed = sorted_unique(rng, 800, 11_000)
    tomb = ctx.tombstones(removed)
    one, st1 = count(ctx, [(seg, 0, 40)], ids)
    assert st1.n_windows == 1 and np.array_equal(one, truth(lists, ids))
    for skip in (1, 0):
        with Option(ctx, "union.many_window_log2", 11, 30), Option(ctx, "count.summary_skip", skip, 1):
            got, st = count(ctx, [(seg, 0, 40)], ids)
            assert 4 <= st.n_windows <= 6 and np.array_equal(got, one), skip
            got, _ = count(ctx, [(seg, 0, 40)], ids, tomb)
            assert np.array_equal(got, truth(lists, ids, removed)), skip
    # the default window, ids 0 and 2^32 - 1 in the set and in a list: a doc span of 2^32, four windows of 2^30
    edge = [np.asarray([0, 5, 0xFFFFFFFF], np.uint32), np.asarray([0xFFFFFFFE, 0xFFFFFFFF], np.uint32), np.asarray([0, 7], np.uint32)] + lists[:5]
    seg2 = ctx.encode_lists(edge)
    ids2 = np.union1d(ids, np.asarray([0, 0xFFFFFFFF], np.uint32)).astype(np.uint32)
    got, st = count(ctx, [(seg2, 0, len(edge))], ids2)
    assert st.n_windows == 4 and np.array_equal(got, truth(edge, ids2))
    assert got[:3].tolist() == [2, 1, 1]
    rem2 = np.asarray([0xFFFFFFFF, 5], np.uint32)
    got, _ = count(ctx, [(seg2, 0, len(edge))], ids2, ctx.tombstones(rem2))
    assert np.array_equal(got, truth(edge, ids2, rem2))


def test_span_clipping(ctx):
    rng = np.random.default_rng(46)
    lists = [sorted_unique(rng, int(n), 1_000_000) for n in (60_000, 30_000, 5000, 900, 300, 20)]
    seg = ctx.encode_lists(lists)
    ids = (sorted_unique(rng, 40, 101) + 400_000).astype(np.uint32)
    lo, hi = block_bounds(lists)
    meet = int(np.count_nonzero((lo <= int(ids[-1])) & (hi >= int(ids[0]))))      # blocks whose doc bounds meet the set's span
    assert 0 < meet <= 2 * len(lists) and lo.size > 370
    for skip in (0, 1):
        with Option(ctx, "count.summary_skip", skip, 1):
            got, st = count(ctx, [(seg, 0, len(lists))], ids)
            assert np.array_equal(got, truth(lists, ids)), skip
            assert st.n_blocks == lo.size and st.n_decoded <= meet, (skip, st.n_decoded, meet)
    assert got.sum() > 0


def test_summary_skip(ctx):
    rng = np.random.default_rng(47)
    D = 20_000_000
    long_list = np.cumsum(rng.integers(50, 148, 200_000)).astype(np.uint32)        # gaps of about 100
    assert long_list[-1] < D - 1
    seg = ctx.encode_lists([long_list])
    a = int(np.searchsorted(long_list, 7_000_000))
    stretch = np.union1d(long_list[a:a + 10:2], sorted_unique(rng, 45, 1000) + 7_000_000)[:50]      # hits and misses in one 1000-doc stretch
    ids = np.union1d(stretch, np.asarray([0, D - 1], np.uint32)).astype(np.uint32)                 # ... and the span kept wide
    want = truth([long_list], ids)
    lo, hi = block_bounds([long_list])
    n_blocks = lo.size
    holds_hit = np.unique(np.flatnonzero(np.isin(long_list, ids)) // 256).size
    chunks = np.unique(ids.astype(np.int64) >> 11)                                  # the 2048-doc chunks that hold a set id
    meets = int(sum(np.any((chunks >= l >> 11) & (chunks <= h >> 11)) for l, h in zip(lo, hi)))
    assert n_blocks == 782 and 1 <= holds_hit <= meets < 40
    with Option(ctx, "count.summary_skip", 0, 1):
        got, st = count(ctx, [(seg, 0, 1)], ids)
        assert np.array_equal(got, want) and st.n_decoded == n_blocks == st.n_blocks
    got, st = count(ctx, [(seg, 0, 1)], ids)
    assert np.array_equal(got, want) and want[0] >= 5
    assert holds_hit <= st.n_decoded <= meets, (holds_hit, st.n_decoded, meets)


def test_every_doc(ctx):
    rng = np.random.default_rng(48)
    lists = [sorted_unique(rng, n, 300_000) for n in (1, 256, 257, 5000, 0, 70_000, 3)]
    seg = ctx.encode_lists(lists)
    ranges = [(seg, 0, len(lists)), (seg, 3, 4)]
    named = lists + lists[3:4]
    got, st = count(ctx, ranges, None)
    assert np.array_equal(got, [len(l) for l in named]) and st.n_windows == 0 and st.n_hits == sum(len(l) for l in named)
    removed = np.union1d(sorted_unique(rng, 50_000, 300_000), lists[6]).astype(np.uint32)
    got, st = count(ctx, ranges, None, ctx.tombstones(removed))
    assert np.array_equal(got, truth(named, None, removed)) and got[6] == 0
    assert st.n_windows == 0 and st.n_decoded == st.n_blocks


def test_a_wave_walks_several_blocks_across_range_ends(ctx):
    """More blocks than 2 x 32 waves per CU: every wave of k_cr_count walks three blocks, and range ends fall inside its run."""
    rng = np.random.default_rng(52)
    D = 1 << 22
    segments, ranges, per_wave = one_block_lists_past_a_wave(rng, D)
    segs = [ctx.encode_lists(lists) for lists in segments]
    named = [segments[s][j] for s, a, b in ranges for j in range(a, b)]
    flat, owner = np.concatenate(named), np.repeat(np.arange(len(named)), [l.size for l in named])
    lo, hi = block_bounds(named)                                         # (one block per list)
    assert lo.size == len(named) > 2 * 32 * torch.cuda.get_device_properties(0).multi_processor_count and per_wave >= 3

    def want(ids, removed=()):
        hit = (np.ones(flat.size, bool) if ids is None else np.isin(flat, ids)) & ~np.isin(flat, np.asarray(removed, np.uint32))
        return np.bincount(owner[hit], minlength=len(named)).astype(np.uint64)

    # the set: 300 ids of the middle half of the universe, a third of them out of the lists
    mid = flat[(flat >= D // 4) & (flat < 3 * D // 4)]
    ids = np.union1d(rng.choice(mid, 100, replace=False), sorted_unique(rng, 200, D // 2) + D // 4).astype(np.uint32)
    doc_lo, doc_hi = max(int(lo.min()), int(ids[0])), min(int(hi.max()), int(ids[-1]))
    meet = (lo <= doc_hi) & (hi >= doc_lo)                               # the bound test
    base = doc_lo & ~2047
    ca, cc = (np.maximum(lo, doc_lo) - base) >> 11, (np.minimum(hi, doc_hi) - base) >> 11
    inside = ids[(ids >= doc_lo) & (ids <= doc_hi)].astype(np.int64)
    marked = np.unique((inside - base) >> 11)                            # the summary: the 2048-doc chunks that hold a marked id
    near = np.searchsorted(marked, ca) < np.searchsorted(marked, cc, side="right")
    read = {0: int(meet.sum()), 1: int((meet & ((cc - ca >= 64) | near)).sum())}
    assert 0 < read[1] < read[0] < lo.size and int((meet & (cc - ca >= 64)).sum()) > 50
    R = [(segs[s], a, b) for s, a, b in ranges]
    for skip in (0, 1):
        with Option(ctx, "count.summary_skip", skip, 1):
            got, st = count(ctx, R, ids)
            assert np.array_equal(got, want(ids)), skip
            assert (st.n_lists, st.n_blocks, st.n_windows, st.n_hits) == (len(named), lo.size, 1, int(got.sum()))
            assert st.n_decoded == read[skip], (skip, st.n_decoded, read)
    assert got.sum() >= 100
    removed = np.union1d(rng.choice(flat, 5000, replace=False), ids[::3]).astype(np.uint32)
    got, st = count(ctx, R, None, ctx.tombstones(removed))               # every doc: no bound test, every block is read
    assert np.array_equal(got, want(None, removed)) and 0 < got.sum() < flat.size
    assert st.n_windows == 0 and st.n_decoded == st.n_blocks == lo.size


def test_scratch_stays_clean(ctx):
    rng = np.random.default_rng(49)
    D = 400_000
    lists = [sorted_unique(rng, int(rng.integers(1, 3000)), D) for _ in range(80)]
    seg = ctx.encode_lists(lists)
    ids = sorted_unique(rng, 90_000, D)
    with Option(ctx, "union.many", 1, 0):
        got, _ = count(ctx, [(seg, 0, 40)], ids)
        assert np.array_equal(got, truth(lists[:40], ids))
        out, n = ctx.union_ranges([(seg, 40, 80)])                     # the same bitmap: nothing of the set may be left in it
        assert np.array_equal(out.download(n), np.unique(np.concatenate(lists[40:80])))
        got, _ = count(ctx, [(seg, 0, 80)], ids[:5000])                # ... and nothing of the union
        assert np.array_equal(got, truth(lists, ids[:5000]))


def test_set_from_a_query(ctx):
    rng = np.random.default_rng(50)
    D = 100_000
    lists = [sorted_unique(rng, int(n), D) for n in rng.integers(200, 6000, 30)]
    seg = ctx.encode_lists(lists)
    groups, exclude = [[(seg, 0, 2)], [(seg, 2, 5)]], [[(seg, 5, 6)]]
    dset, n = ctx.andnot_ranges(groups, exclude, out=ctx.empty(20_000))
    assert n > 0
    got, st = ctx.count_ranges([(seg, 6, 30)], dset, n)
    _, off = ctx.query_batch_groups([(groups + [[(seg, k, k + 1)]], exclude) for k in range(6, 30)], out=ctx.empty(24 * 20_000))
    assert np.array_equal(got, np.diff(off)) and st.n_hits == int(off[-1])
    assert np.array_equal(got, truth(lists[6:], dset.download(n)))


def test_two_contexts_on_two_threads(ctx):
    workers = [Context(0), Context(0)]
    inputs = []
    for i in range(2):
        rng = np.random.default_rng(200 + i)
        lists = [sorted_unique(rng, int(rng.integers(1, 4000)), 500_000) for _ in range(120 + 7 * i)]
        ids = sorted_unique(rng, 70_000 + 999 * i, 500_000)
        inputs.append((lists, ids, truth(lists, ids)))
    errors, barrier = [], threading.Barrier(2)

    def run(i):
        try:
            c = workers[i]
            lists, ids, want = inputs[i]
            seg = c.encode_lists(lists)
            d, n = device_set(c, ids)
            barrier.wait()
            for rep in range(5):
                got, st = c.count_ranges([(seg, 0, len(lists))], d, n)
                assert np.array_equal(got, want) and st.n_hits == int(want.sum()), (i, rep)
        except BaseException as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for c in workers:
        c.close()


def test_errors_leave_nothing_behind(ctx):
    rng = np.random.default_rng(51)
    lists = [sorted_unique(rng, 500, 50_000) for _ in range(10)]
    seg = ctx.encode_lists(lists)
    d, n = device_set(ctx, sorted_unique(rng, 1000, 50_000))
    buf = np.full(16, SENTINEL, np.uint64)
    assert raw(ctx, [(seg, 0, 10)], d, n, buf, 16) == 0                 # (the call's buffers are grown: the errors below allocate nothing)
    live = (C.c_uint64(), C.c_uint64())
    ctx.lib.ii2_devmem_stats(C.byref(live[0]), C.byref(live[1]))
    before = live[0].value
    buf[:] = SENTINEL
    for bad in ([(seg, 5, 4)], [(seg, 0, 11)], [(seg, 0, 3), (None, 0, 1)]):      # a bad range, a range past n_lists, no segment
        assert raw(ctx, bad, d, n, buf, 16) == -1
    assert raw(ctx, [(seg, 0, 10)], d, n, None, 16) == -1               # counts is NULL
    assert np.all(buf == SENTINEL)
    ctx.lib.ii2_devmem_stats(C.byref(live[0]), C.byref(live[1]))
    assert live[0].value == before
    got, _ = ctx.count_ranges([(seg, 0, 10)], d, n)                     # the context goes on working
    assert np.array_equal(got, truth(lists, d.download(n)))
