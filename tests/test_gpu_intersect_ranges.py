"""GPU: ii2_intersect_ranges - the AND of ORs over list ranges (a term spread over the segments of an unmerged shard, a
prefix) - against numpy: reduce(np.intersect1d, [np.unique(np.concatenate(group))]) minus the removed ids."""
import ctypes as C
import threading
from functools import reduce

import numpy as np
import pytest

from inverted_index_2_amd import Context, II2Error, synth
from tests.gpu_util import ctx, path_delta, sorted_unique  # noqa: F401
from tests.test_config1_cpu import c1_segments

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
ALWAYS_MARK = 1 << 40


def truth(groups, removed=()):
    """groups: [[list of ids, ...], ...]"""
    if not groups:
        return np.empty(0, np.uint32)
    sets = [np.unique(np.concatenate([np.asarray(l, np.uint32) for l in g] + [np.empty(0, np.uint32)])) for g in groups]
    return np.setdiff1d(reduce(np.intersect1d, sets), np.asarray(removed, np.uint32)).astype(np.uint32)


def isect(ctx, groups, tomb=None):
    out, n = ctx.intersect_ranges(groups, tomb=tomb)
    return out.download(n)


def raw(ctx, groups, out, cap):
    """(return code, count) of one ii2_intersect_ranges call into `out` (a DeviceArray or None) with capacity `cap`."""
    ranges = [r for g in groups for r in g]
    n = len(ranges)
    gf = [0]
    for g in groups:
        gf.append(gf[-1] + len(g))
    group_first = (C.c_uint64 * len(gf))(*gf)
    segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
    first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
    end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
    cnt = C.c_uint64(12345)
    rc = ctx.lib.ii2_intersect_ranges(ctx.h, len(groups), group_first, segs, first, end, None,
                                      out.data_ptr() if out is not None else None, cap, C.byref(cnt))
    return rc, cnt.value


class Options:
    DEFAULTS = {"intersect.ranges": 0, "intersect.ranges_mark": 64, "union.many_window_log2": 30, "union.many": 0}

    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, {k.replace("__", "."): v for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set_option(k, self.DEFAULTS[k])


# every path of the call: the default choice, the group path with its own filter choice, forced probe, forced mark
MODES = [{}, {"intersect__ranges": 1}, {"intersect__ranges": 1, "intersect__ranges_mark": 0},
         {"intersect__ranges": 1, "intersect__ranges_mark": ALWAYS_MARK}]


def check_all_modes(ctx, groups, want, tomb=None):
    for m in MODES:
        with Options(ctx, **m), path_delta(ctx) as took:
            got = isect(ctx, groups, tomb)
        assert np.array_equal(got, want), m
        # the mode took the paths it names: a non-empty result of two or more groups means every filter pass ran
        forced = m.get("intersect__ranges") == 1
        assert not (forced and "ir.handoff" in took), (m, took)
        assert took.get("ir.handoff", 0) + took.get("ir.groups", 0) <= 1, (m, took)
        if forced and len(groups) > 1 and want.size:
            assert took.get("ir.groups") == 1, (m, took)
            passes = len(groups) - 1
            if m.get("intersect__ranges_mark") == 0:
                assert took.get("ir.probe") == passes and "ir.mark" not in took, (m, took)
            elif m.get("intersect__ranges_mark") == ALWAYS_MARK:
                assert took.get("ir.mark") == passes and "ir.probe" not in took, (m, took)
            else:
                assert took.get("ir.probe", 0) + took.get("ir.mark", 0) == passes, (m, took)


def test_c1_as_configured(ctx):
    # BASELINE configs[0]: 2 unmerged segments x 10k docs, the two most frequent terms - no merge before the AND
    terms, offs, vals, (s1, s2), (rank, doc) = c1_segments(1_000_000, 10_000)
    segs = [ctx.encode(o, v) for o, v in zip(offs, vals)]
    groups = [[(s, int(s1), int(s1) + 1) for s in segs], [(s, int(s2), int(s2) + 1) for s in segs]]
    want = np.intersect1d(doc[rank == 0], doc[rank == 1]).astype(np.uint32)
    assert 5000 < want.size < 12000
    check_all_modes(ctx, groups, want)


def test_handoff_matches_group_path(ctx):
    rng = np.random.default_rng(1)
    D = 4_000_000
    dense = [synth.zipf_list(2, D), synth.zipf_list(3, D)]                      # C2-shaped, reduced
    skewed = [sorted_unique(rng, 150, D), sorted_unique(rng, 900_000, D)]
    eight = [sorted_unique(rng, int(D / (2 + r)), D) for r in range(8)]
    for lists in (dense, skewed, eight):
        seg = ctx.encode_lists(lists)
        groups = [[(seg, i, i + 1)] for i in range(len(lists))]
        want = truth([[l] for l in lists])
        out, n = ctx.intersect([(seg, i) for i in range(len(lists))])
        assert np.array_equal(out.download(n), want)
        check_all_modes(ctx, groups, want)


def _split(lists, k, how, rng):
    """The lists cut over k segments: by doc range, or at random with 10 % of the postings also in a second segment."""
    parts = [[None] * len(lists) for _ in range(k)]
    for t, l in enumerate(lists):
        if how == "range":
            hi = int(l.max()) + 1 if l.size else 1
            cut = np.searchsorted(l, np.linspace(0, hi, k + 1).astype(np.int64))
            for s in range(k):
                parts[s][t] = l[cut[s]:cut[s + 1]]
        else:
            home = rng.integers(0, k, l.size)
            dup = rng.random(l.size) < 0.1
            second = (home + 1 + rng.integers(0, max(k - 1, 1), l.size)) % k
            for s in range(k):
                parts[s][t] = l[(home == s) | (dup & (second == s))]
    return parts


@pytest.mark.parametrize("k", [2, 5, 16])
def test_terms_split_over_segments(ctx, k):
    rng = np.random.default_rng(k)
    D = 3_000_000
    lists = [synth.zipf_list(r, D) for r in (1, 2, 5)] + [sorted_unique(rng, 4000, D)]
    want = truth([[l] for l in lists])
    for how in ("range", "random"):
        parts = _split(lists, k, how, rng)
        segs = [ctx.encode_lists(p) for p in parts]
        for terms in ([0, 1], [1, 2, 0], [3, 0, 1, 2]):
            groups = [[(segs[s], t, t + 1) for s in range(k)] for t in terms]
            check_all_modes(ctx, groups, truth([[lists[t]] for t in terms]))
        groups = [[(segs[s], t, t + 1) for s in range(k)] for t in range(len(lists))]
        check_all_modes(ctx, groups, want)


@pytest.fixture(scope="module")
def prefix_seg(ctx):
    """One segment: 3000 small lists (a dictionary's prefix runs) over 2M docs, then three long terms."""
    rng = np.random.default_rng(7)
    D = 2_000_000
    lists = [sorted_unique(rng, int(rng.integers(1, 400)), D) for _ in range(3000)]
    lists += [sorted_unique(rng, 600_000, D), sorted_unique(rng, 40_000, D), sorted_unique(rng, 300, D)]
    return ctx.encode_lists(lists), lists


def test_prefix_groups(ctx, prefix_seg):
    seg, lists = prefix_seg
    for t in (3000, 3001, 3002):
        groups = [[(seg, 500, 2500)], [(seg, t, t + 1)]]
        want = truth([lists[500:2500], [lists[t]]])
        assert want.size > 0
        check_all_modes(ctx, groups, want)
    groups = [[(seg, 0, 1500)], [(seg, 1200, 3000)]]                         # two prefixes
    check_all_modes(ctx, groups, truth([lists[0:1500], lists[1200:3000]]))
    groups = [[(seg, 0, 1000), (seg, 2000, 2100)], [(seg, 900, 2900)], [(seg, 3000, 3002)]]
    check_all_modes(ctx, groups, truth([lists[0:1000] + lists[2000:2100], lists[900:2900], lists[3000:3002]]))


def test_views_overlaps_and_shared_segments(ctx):
    rng = np.random.default_rng(11)
    D = 300_000
    mk = lambda k, lo=1, hi=30000: [sorted_unique(rng, int(rng.integers(lo, hi)), D) for _ in range(k)]
    A = mk(20)
    segA = ctx.encode_lists(A)
    X1, X2 = mk(10), mk(10)
    segM, _ = ctx.merge_to_segment([ctx.encode_lists(X1), ctx.encode_lists(X2)])
    M = [np.union1d(x, y) for x, y in zip(X1, X2)]
    S = mk(8)
    src = [0, -1, 1, 2, -1, 3, 4, 5, 6, 7]
    segV = ctx.select(ctx.encode_lists(S), src)
    V = [S[j] if j >= 0 else np.empty(0, np.uint32) for j in src]
    L1 = mk(4)
    segAl = ctx.select_aligned(ctx.encode_lists(L1), ctx.align_terms([[b"a", b"c", b"e"], [b"b", b"c", b"d", b"e"]]), 1)
    Al = [np.empty(0, np.uint32)] + L1
    groups = [[(segA, 0, 5), (segA, 3, 8), (segM, 2, 4)],       # overlapping ranges of one segment
              [(segA, 4, 6), (segV, 0, 10)],                     # the same segment in another group, a view with empty slots
              [(segAl, 0, 5), (segM, 0, 10), (segA, 0, 20)]]
    want = truth([A[0:8] + M[2:4], A[4:6] + V, Al + M + A])
    assert want.size > 0
    check_all_modes(ctx, groups, want)
    removed = np.unique(rng.integers(0, D, 20_000)).astype(np.uint32)
    tomb = ctx.tombstones(removed)
    check_all_modes(ctx, groups, truth([A[0:8] + M[2:4], A[4:6] + V, Al + M + A], removed), tomb)


def test_empty_and_trivial_calls(ctx, prefix_seg):
    seg, lists = prefix_seg
    segV = ctx.select(seg, [-1, 5, -1])                                       # slots 0 and 2 are empty lists
    out = ctx.empty(64).upload(np.full(64, SENTINEL, np.uint32))
    assert raw(ctx, [], None, 0) == (0, 0)                                   # no group
    for m in MODES:
        with Options(ctx, **m):
            assert raw(ctx, [[(seg, 0, 10)], [(seg, 4, 4)]], None, 0) == (0, 0)               # an empty range
            assert raw(ctx, [[(seg, 0, 10)], [(segV, 0, 1), (segV, 2, 3)]], out, 64) == (0, 0)   # only empty lists
            assert raw(ctx, [[(seg, 0, 10)], []], out, 64) == (0, 0)                           # a group without ranges
    assert np.all(out.download() == SENTINEL)
    # disjoint doc spans: nothing in common
    lo = ctx.encode_lists([np.arange(0, 5000, 3, dtype=np.uint32), np.arange(10_000, 20_000, 7, dtype=np.uint32)])
    for m in MODES:
        with Options(ctx, **m):
            assert raw(ctx, [[(lo, 0, 1)], [(lo, 1, 2)]], out, 64) == (0, 0)
    assert np.all(out.download() == SENTINEL)
    # one group: the union of its ranges
    u, n = ctx.union_ranges([(seg, 100, 900), (segV, 0, 3)])
    assert np.array_equal(isect(ctx, [[(seg, 100, 900), (segV, 0, 3)]]), u.download(n))
    # bad ranges
    for bad in [[[(seg, 5, 4)], [(seg, 0, 1)]], [[(seg, 0, 1)], [(seg, 0, len(lists) + 1)]]]:
        rc, _ = raw(ctx, bad, ctx.empty(16), 16)
        assert rc == -1


def test_hundred_groups_and_id_edges(ctx):
    rng = np.random.default_rng(3)
    D = 1 << 32
    core = np.asarray([0, 1, 77, 1 << 20, (1 << 31) + 5, D - 2, D - 1], np.uint32)
    lists = [np.union1d(core, sorted_unique(rng, int(rng.integers(10, 20000)), D)).astype(np.uint32) for _ in range(100)]
    seg = ctx.encode_lists(lists)
    groups = [[(seg, i, i + 1)] for i in range(100)]
    want = truth([[l] for l in lists])
    assert np.array_equal(want, core) or set(core) <= set(want.tolist())
    check_all_modes(ctx, groups, want)
    removed = np.asarray([0, D - 1, 77], np.uint32)
    check_all_modes(ctx, groups, truth([[l] for l in lists], removed), ctx.tombstones(removed))


@pytest.mark.parametrize("n_blocks", [2, 10, 63, 64, 65, 100])
def test_probe_walks_to_the_largest_id(ctx, n_blocks):
    # the probe reaches 2^32 - 1 in a list's last block from an earlier block of the same list: fewer than 64 blocks ahead
    # (the one-load walk), exactly 64, and more (the search behind it)
    D = 1 << 32
    a = np.append(np.arange(0, 256 * (n_blocks - 1) + 45, dtype=np.uint32), np.uint32(D - 1))
    cand = np.asarray([5, 200, D - 1], np.uint32)                          # the last two from block 0 on
    seg = ctx.encode_lists([a, cand, np.asarray([5, D - 2], np.uint32)])
    assert seg.range_blocks(0, 1, ctx) == n_blocks
    for groups, want in ([[[(seg, 0, 1)], [(seg, 1, 2)]], cand], [[[(seg, 0, 1)], [(seg, 2, 3)]], np.asarray([5], np.uint32)]):
        for m in ({"intersect__ranges": 1, "intersect__ranges_mark": 0}, {"intersect__ranges": 1}, {}):
            with Options(ctx, **m):
                assert np.array_equal(isect(ctx, groups), want), (n_blocks, m)


def test_mark_over_several_windows(ctx, prefix_seg):
    seg, lists = prefix_seg
    groups = [[(seg, 0, 600)], [(seg, 300, 2000)], [(seg, 3000, 3001)]]
    want = truth([lists[0:600], lists[300:2000], [lists[3000]]])
    removed = np.unique(np.random.default_rng(2).integers(0, 2_000_000, 50_000)).astype(np.uint32)
    for log2 in (11, 14, 17):
        with Options(ctx, intersect__ranges_mark=ALWAYS_MARK, union__many_window_log2=log2):
            assert np.array_equal(isect(ctx, groups), want), log2
            assert np.array_equal(isect(ctx, groups, ctx.tombstones(removed)),
                                  truth([lists[0:600], lists[300:2000], [lists[3000]]], removed)), log2


def test_tombstones(ctx, prefix_seg):
    seg, lists = prefix_seg
    groups = [[(seg, 3000, 3001)], [(seg, 3001, 3002)], [(seg, 0, 3000)]]
    want = truth([[lists[3000]], [lists[3001]], lists[0:3000]])
    assert want.size > 100
    part = want[::3]
    check_all_modes(ctx, groups, np.setdiff1d(want, part), ctx.tombstones(part))
    check_all_modes(ctx, groups, np.empty(0, np.uint32), ctx.tombstones(want))          # every id of the result removed
    pair = [[(seg, 3000, 3001)], [(seg, 3001, 3002)]]
    w2 = truth([[lists[3000]], [lists[3001]]])
    check_all_modes(ctx, pair, np.empty(0, np.uint32), ctx.tombstones(w2))


def _capacity_case(ctx, groups, want):
    out = ctx.empty(want.size + 64).upload(np.full(want.size + 64, SENTINEL, np.uint32))
    rc, cnt = raw(ctx, groups, out, want.size - 1)
    assert rc == -4 and cnt == want.size                                   # II2_ECAPACITY, the size needed
    assert np.all(out.download() == SENTINEL)                              # nothing written
    rc, cnt = raw(ctx, groups, out, want.size)
    assert rc == 0 and cnt == want.size
    assert np.array_equal(out.download(cnt), want)
    assert np.all(out.download()[cnt:] == SENTINEL)


def test_capacity_all_or_nothing(ctx, prefix_seg):
    seg, lists = prefix_seg
    rng = np.random.default_rng(4)
    big = sorted_unique(rng, 200_000, 1_000_000)
    sub = big[::7]                                                         # the result is the whole shorter list
    s2 = ctx.encode_lists([big, sub])
    # cap = exact: the hand-off (cap >= the shorter list); exact - 1: the group path
    _capacity_case(ctx, [[(s2, 0, 1)], [(s2, 1, 2)]], sub)
    for m in MODES[1:]:
        with Options(ctx, **m):
            _capacity_case(ctx, [[(s2, 0, 1)], [(s2, 1, 2)]], sub)
            _capacity_case(ctx, [[(seg, 3000, 3001)], [(seg, 0, 3000)], [(seg, 3001, 3003)]],
                           truth([[lists[3000]], lists[0:3000], lists[3001:3003]]))
    with pytest.raises(II2Error):
        ctx.intersect_ranges([[(s2, 0, 1)], [(s2, 1, 2)]], out=ctx.empty(4))


def test_two_contexts_at_once(ctx, prefix_seg):
    seg, lists = prefix_seg
    groups = [[(seg, 0, 2000)], [(seg, 1000, 3000)], [(seg, 3000, 3002)]]
    want = truth([lists[0:2000], lists[1000:3000], lists[3000:3002]])
    u_want = np.unique(np.concatenate(lists[0:3000]))
    errors = []

    def work(mark):
        try:
            c = Context(0)
            c.set_option("intersect.ranges_mark", mark)
            for _ in range(6):
                out, n = c.intersect_ranges(groups)
                assert np.array_equal(out.download(n), want)
            c.set_option("union.many", 1)
            out, n = c.union_ranges([(seg, 0, 3000)])                      # the scratch was left zero
            assert np.array_equal(out.download(n), u_want)
            c.close()
        except Exception as e:                                             # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=(m,)) for m in (ALWAYS_MARK, ALWAYS_MARK)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
