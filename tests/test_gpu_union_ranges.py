"""GPU: ii2_union_ranges - the union of every list of any number of list ranges (PrefixSearch's union), against numpy:
np.setdiff1d(np.unique(np.concatenate(lists)), removed)."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import II2Error
from tests.gpu_util import ctx, path_delta, sorted_unique  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF


def truth(lists, removed=()):
    arrs = [np.asarray(l, np.uint32) for l in lists if len(l)]
    if not arrs:
        return np.empty(0, np.uint32)
    return np.setdiff1d(np.unique(np.concatenate(arrs)), np.asarray(removed, np.uint32)).astype(np.uint32)


def union(ctx, ranges, tomb=None):
    out, n = ctx.union_ranges(ranges, tomb=tomb)
    return out.download(n)


def raw(ctx, ranges, out, cap):
    """(return code, count) of one ii2_union_ranges call into `out` with capacity `cap`."""
    n = len(ranges)
    segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
    first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
    end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
    cnt = C.c_uint64(12345)
    rc = ctx.lib.ii2_union_ranges(ctx.h, n, segs, first, end, None, out.data_ptr(), cap, C.byref(cnt))
    return rc, cnt.value


class Option:
    def __init__(self, ctx, name, value, default):
        self.ctx, self.name, self.value, self.default = ctx, name, value, default

    def __enter__(self):
        self.ctx.set_option(self.name, self.value)

    def __exit__(self, *exc):
        self.ctx.set_option(self.name, self.default)


@pytest.fixture(scope="module")
def zipf(ctx):
    """One segment of 5000 Zipf-sized lists over 2M docs, then 300 lists of one posting each."""
    rng = np.random.default_rng(7)
    D = 2_000_000
    lists = [sorted_unique(rng, max(1, D // (4 * r)), D) for r in range(1, 5001)]
    lists += [np.asarray([int(x)], np.uint32) for x in rng.integers(0, D, 300)]
    return ctx.encode_lists(lists), lists


def test_many_lists_one_segment(ctx, zipf):
    seg, lists = zipf
    n = len(lists)
    for a, b in [(0, n), (100, 170), (5000, 5300), (4000, 5300), (0, 1)]:
        assert np.array_equal(union(ctx, [(seg, a, b)]), truth(lists[a:b])), (a, b)
    rng = np.random.default_rng(3)
    removed = np.unique(rng.integers(0, 2_000_000, 50_000)).astype(np.uint32)
    removed = np.union1d(removed, lists[5100]).astype(np.uint32)       # a single-posting list removed entirely
    tomb = ctx.tombstones(removed)
    for a, b in [(0, n), (100, 170), (5000, 5300)]:
        assert np.array_equal(union(ctx, [(seg, a, b)], tomb), truth(lists[a:b], removed)), (a, b)


def test_eight_kinds_of_segments(ctx):
    rng = np.random.default_rng(11)
    D = 300_000
    mk = lambda k, lo=1, hi=3000: [sorted_unique(rng, int(rng.integers(lo, hi)), D) for _ in range(k)]
    A = mk(120)
    segA = ctx.encode_lists(A)
    B = mk(40)
    B[3] = np.empty(0, np.uint32)
    B[17] = np.empty(0, np.uint32)
    segB = ctx.encode_lists(B)
    X1, X2 = mk(90), mk(90)
    segM, _ = ctx.merge_to_segment([ctx.encode_lists(X1), ctx.encode_lists(X2)])
    M = [np.union1d(x, y) for x, y in zip(X1, X2)]
    S = mk(30)
    base = ctx.encode_lists(S)
    src = [0, -1, 1, 2, -1, -1, 3] + list(range(4, 30)) + [-1]
    segV = ctx.select(base, src)                                        # a view with empty slots
    V = [S[j] if j >= 0 else np.empty(0, np.uint32) for j in src]
    d0, d1 = [b"a", b"c", b"e"], [b"b", b"c", b"d", b"e"]
    L1 = mk(4)
    al = ctx.align_terms([d0, d1])
    segAl = ctx.select_aligned(ctx.encode_lists(L1), al, 1)           # union terms a b c d e: slot 0 empty
    Al = [np.empty(0, np.uint32)] + L1
    C6, C7, C8 = mk(70, 1, 5), mk(10, 5000, 20000), mk(3)
    seg6, seg7, seg8 = ctx.encode_lists(C6), ctx.encode_lists(C7), ctx.encode_lists(C8)
    ranges = [(segA, 0, 100), (segA, 50, 120),          # the same segment twice, overlapping
              (segB, 0, 40), (segM, 10, 80), (segV, 0, len(src)), (segAl, 0, 5),
              (seg6, 0, 70), (seg7, 2, 9), (seg8, 1, 1),          # an empty range
              (segV, 1, 2), (segV, 4, 6)]                          # ranges made only of empty lists
    want = truth(A[0:120] + B + M[10:80] + V + Al + C6 + C7[2:9])
    assert np.array_equal(union(ctx, ranges), want)
    removed = np.unique(rng.integers(0, D, 20_000)).astype(np.uint32)
    assert np.array_equal(union(ctx, ranges, ctx.tombstones(removed)), truth(A + B + M[10:80] + V + Al + C6 + C7[2:9], removed))
    # empty queries: no range, only empty ranges / empty lists - count 0, no output buffer needed
    assert raw(ctx, [], ctx.empty(1), 0) == (0, 0)
    assert raw(ctx, [(seg8, 1, 1), (segV, 1, 2), (segAl, 0, 1)], ctx.empty(1), 0) == (0, 0)
    # bad ranges
    for bad in [[(segA, 5, 4)], [(segA, 0, 121)]]:
        rc, _ = raw(ctx, bad, ctx.empty(16), 16)
        assert rc == -1


def test_doc_id_edges_and_windows(ctx):
    rng = np.random.default_rng(5)
    lists = [sorted_unique(rng, int(rng.integers(1, 4000)), 500_000) + 1_000_003 for _ in range(100)]
    lists[0] = np.asarray([1_000_003, 1_000_004, 1_000_040], np.uint32)           # lo = 1000003: not a multiple of 32
    seg = ctx.encode_lists(lists)
    want = truth(lists)
    assert np.array_equal(union(ctx, [(seg, 0, 100)]), want)
    removed = np.unique(rng.integers(1_000_000, 1_600_000, 30_000)).astype(np.uint32)
    tomb = ctx.tombstones(removed)
    for log2 in (11, 13, 17):                 # several windows: 2048, 8192, 131072 docs each
        with Option(ctx, "union.many_window_log2", log2, 30):
            assert np.array_equal(union(ctx, [(seg, 0, 100)]), want), log2
            assert np.array_equal(union(ctx, [(seg, 0, 100)], tomb), truth(lists, removed)), log2
    # ids at 0 and at the largest id the encoder takes: a doc range of 2^32, four windows of 2^30
    edge = [np.asarray([0, 5, 0xFFFFFFFF], np.uint32), np.asarray([0xFFFFFFFE, 0xFFFFFFFF], np.uint32)] + lists[:80]
    seg2 = ctx.encode_lists(edge)
    assert np.array_equal(union(ctx, [(seg2, 0, len(edge))]), truth(edge))
    rem2 = np.asarray([0, 0xFFFFFFFF, 1_000_003], np.uint32)
    assert np.array_equal(union(ctx, [(seg2, 0, len(edge))], ctx.tombstones(rem2)), truth(edge, rem2))


def _paths_lists(rng):
    small = [sorted_unique(rng, n, 1_000_000) for n in (300, 900, 2000)]
    rank = [sorted_unique(rng, 60_000, 8_000_000) for _ in range(4)]
    stream = [sorted_unique(rng, 800_000, 1_200_000), sorted_unique(rng, 400_000, 1_200_000)]
    tile = [sorted_unique(rng, 150_000, 2_000_000) for _ in range(10)]
    return {"or.small": small, "or.rank": rank, "or.stream2": stream, "or.tiles": tile}       # (the key: the path ii2_union takes)


def test_many_path_matches_union_on_few_lists(ctx):
    rng = np.random.default_rng(9)
    removed = np.unique(rng.integers(0, 2_000_000, 10_000)).astype(np.uint32)
    tomb = ctx.tombstones(removed)
    for name, lists in _paths_lists(rng).items():
        seg = ctx.encode_lists(lists)
        pairs = [(seg, i) for i in range(len(lists))]
        for t in (None, tomb):
            with path_delta(ctx) as took:
                out, n = ctx.union(pairs, tomb=t)
            assert took == {name: 1}, (name, took)
            want = out.download(n)
            assert np.array_equal(want, truth(lists, removed if t else ())), name
            with path_delta(ctx) as took:
                got = union(ctx, [(seg, 0, len(lists))], t)              # <= 64 lists: ii2_union's own path
            assert took == {name: 1}, (name, took)
            assert np.array_equal(got, want), name
            with Option(ctx, "union.many", 1, 0), path_delta(ctx) as took:
                got = union(ctx, [(seg, 0, len(lists))], t)
            assert took == {"or.many": 1, "or.many_window": 1}, (name, took)       # one window of 2^30 docs
            assert np.array_equal(got, want), name


def _capacity_case(ctx, ranges, want):
    out = ctx.empty(want.size + 64).upload(np.full(want.size + 64, SENTINEL, np.uint32))
    rc, cnt = raw(ctx, ranges, out, want.size - 1)
    assert rc == -4 and cnt == want.size                                  # II2_ECAPACITY, the size needed
    assert np.all(out.download() == SENTINEL)                             # nothing written
    rc, cnt = raw(ctx, ranges, out, want.size)                            # the next call: exact (the scratch is clean)
    assert rc == 0 and cnt == want.size
    assert np.array_equal(out.download(cnt), want)
    assert np.all(out.download()[cnt:] == SENTINEL)


def test_capacity_all_or_nothing(ctx, zipf):
    seg, lists = zipf
    _capacity_case(ctx, [(seg, 100, 400)], truth(lists[100:400]))       # many lists
    _capacity_case(ctx, [(seg, 3, 6)], truth(lists[3:6]))                # few lists, default options
    with Option(ctx, "union.many", 1, 0):
        _capacity_case(ctx, [(seg, 3, 6)], truth(lists[3:6]))
    with Option(ctx, "union.many_window_log2", 14, 30):                  # a result over many windows
        _capacity_case(ctx, [(seg, 200, 800)], truth(lists[200:800]))
    assert np.array_equal(union(ctx, [(seg, 0, 5)]), truth(lists[0:5]))
    with pytest.raises(II2Error):
        ctx.union_ranges([(seg, 0, 10)], out=ctx.empty(4))


def test_user_size_20000_of_100k_lists(ctx):
    rng = np.random.default_rng(21)
    D = 100_000_000
    T = 100_000
    sizes = np.maximum(1, (2_000_000 / np.arange(1, T + 1))).astype(np.int64)
    key = np.repeat(np.arange(T, dtype=np.uint64), sizes) << np.uint64(32) | rng.integers(0, D, int(sizes.sum())).astype(np.uint64)
    key = np.unique(key)
    term = (key >> np.uint64(32)).astype(np.int64)
    vals = (key & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    off = np.zeros(T + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(term, minlength=T))
    seg = ctx.encode(off, vals)
    a, b = 1000, 21000
    want = np.unique(vals[int(off[a]):int(off[b])])
    assert np.array_equal(union(ctx, [(seg, a, b)]), want)
