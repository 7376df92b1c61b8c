"""GPU: ii2_query_batch_groups - many AND-of-ORs / NOT queries in one call (csrc/setop_groups_batch.hip + setop.cpp) - against
numpy AND against the single-query entry point (ctx.andnot_ranges) on the same queries, under (batch.groups, batch.tiny) =
(1, 1) (both forms of the batch kernel), (1, 0) (its 1024-thread form for all) and (0, 1) (every query through the single-query
path).  All comparisons are exact.  The pools, queries and expectations are tests/group_batch_cases.py (pure numpy)."""
import ctypes as C
import threading

import numpy as np
import pytest

from inverted_index_2_amd import Context, II2Error, _lib, pack_group_batch
from tests import group_batch_cases as cases
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
MODES = ((1, 1), (1, 0), (0, 1))


def _encode(c, lists):
    """pool of numpy lists -> [(Segment, lists)]: three segments and the view of the first one"""
    pool = [(c.encode_lists(ls), ls) for ls in lists[:3]]
    pool.append((c.select(pool[0][0], cases.VIEW_SRC), lists[3]))
    return pool


def _bind(pool, queries):
    """ranges over pool entries -> ranges over Segments"""
    return [([[(pool[s][0], a, b) for s, a, b in g] for g in groups], [[(pool[s][0], a, b) for s, a, b in g] for g in exclude])
            for groups, exclude in queries]


def _modes(c, modes):
    for groups, tiny in modes:
        c.set_option("batch.groups", groups)
        c.set_option("batch.tiny", tiny)
        try:
            yield groups, tiny
        finally:
            c.set_option("batch.groups", 1)
            c.set_option("batch.tiny", 1)


def _check_batch(c, pool, queries, removed=None, tomb=None, modes=MODES, singles=True):
    """queries over pool entries: numpy, every mode (identical bytes), then ctx.andnot_ranges per query"""
    lists = [ls for _, ls in pool]
    want = [cases.want(lists, g, x, removed) for g, x in queries]
    bound = _bind(pool, queries)
    got_bytes = []
    for mode in _modes(c, modes):
        out, off = c.query_batch_groups(bound, tomb=tomb)
        assert off.dtype == np.uint64 and off.size == len(queries) + 1 and off[0] == 0, mode
        assert np.all(np.diff(off.astype(np.int64)) >= 0), mode
        ids = out.download(int(off[-1]))
        out.free()
        for q, w in enumerate(want):
            g = ids[int(off[q]):int(off[q + 1])]
            assert g.size == w.size and np.array_equal(g, w), (mode, q, cases.query_class(lists, *queries[q]), g[:8], w[:8])
        got_bytes.append(ids.tobytes())
    assert all(b == got_bytes[0] for b in got_bytes)
    if singles:
        big = c.empty(max(max((w.size for w in want), default=0), 1) + 8)
        for q, (groups, exclude) in enumerate(bound):
            if not groups:
                continue                                                     # (ii2_andnot_ranges: no required group is an error)
            smallest = min(sum(l.size for l in cases.lists_of(lists, g)) for g in queries[q][0])
            if smallest + 8 > big.count:
                big.free()
                big = c.empty(smallest + 8)
            _, n = c.andnot_ranges(groups, exclude, tomb=tomb, out=big)
            assert np.array_equal(big.download(n), want[q]), ("andnot_ranges", q)
        big.free()
    return want


@pytest.mark.parametrize("universe,with_tomb,seed", cases.RANDOM_BATCHES)
def test_random_batches(ctx, universe, with_tomb, seed):
    lists, queries, removed, wants = cases.random_batch(universe, with_tomb, seed)
    n, nonempty, removed_some = cases.check_mix(lists, queries, wants, removed)      # >= 30 tiny, 30 small, 10 large, 10 empty ...
    print("classes", n, "non-empty", nonempty, "an exclusion removed something in", removed_some)
    pool = _encode(ctx, lists)
    tomb = ctx.tombstones(removed) if with_tomb else None
    got = _check_batch(ctx, pool, queries, removed, tomb)
    assert all(np.array_equal(a, b) for a, b in zip(got, wants))


def test_agrees_with_the_flat_batch(ctx):
    rng = np.random.default_rng(77)
    core = cases.core_of(rng, 100_000)
    lists = cases.make_lists(rng, 100_000, core=core)
    pool = _encode(ctx, lists)
    flat, grouped = [], []
    for _ in range(200):
        s = int(rng.integers(0, len(pool)))
        k = int(rng.choice([1, 2, 3, 5, 12]))
        a = int(rng.integers(0, len(lists[s]) - k + 1))
        if rng.random() < 0.5:
            flat.append(("or", [(pool[s][0], a, a + k), (pool[0][0], 5, 7)]))
            grouped.append(([[(pool[s][0], a, a + k), (pool[0][0], 5, 7)]], []))             # an OR: one required group
        else:
            flat.append(("and", [(pool[s][0], a, a + k)]))
            grouped.append(([[(pool[s][0], j, j + 1)] for j in range(a, a + k)], []))         # an AND of lists: one group per list
    removed = np.unique(rng.integers(0, 100_000, 400, dtype=np.uint64)).astype(np.uint32)
    for tomb in (None, ctx.tombstones(removed)):
        o1, f1 = ctx.query_batch(flat, tomb=tomb)
        for mode in _modes(ctx, MODES):
            o2, f2 = ctx.query_batch_groups(grouped, tomb=tomb)
            assert np.array_equal(f1, f2), mode
            assert o1.download(int(f1[-1])).tobytes() == o2.download(int(f2[-1])).tobytes(), mode
            o2.free()
        assert int(f1[-1]) > 1000
        o1.free()


def test_capacity_of_the_batch_kernel_and_one_past_it(ctx):
    full = [np.arange(i, 256 * 64 + i, 64, dtype=np.uint32) for i in range(33)]   # 33 lists of 256 postings: one full block each
    l64 = [np.arange(i, 64 * 100 + i, 100, dtype=np.uint32) for i in range(33)]   # 33 lists of 64 postings
    one = [np.array([77], np.uint32), np.array([64], np.uint32)]
    many = [np.arange(i % 7, 2000, 17 + i % 5, dtype=np.uint32) for i in range(80)]
    lists = [full, l64, one, many]
    pool = [(ctx.encode_lists(ls), ls) for ls in lists]
    queries = [
        # the excluded lists are counted in: 20 + 12 lists, 2048 postings in 32 blocks - exactly the 256-thread form's capacity
        ([[(1, 0, 10)], [(1, 10, 20)]], [[(1, 20, 32)]]),
        ([[(1, 0, 10)], [(1, 10, 20)]], [[(1, 20, 33)]]),           # 33 blocks: one past it -> the 1024-thread form
        ([[(1, 0, 32)]], []),                                       # 32 blocks in one group
        ([[(1, 0, 33)]], []),
        ([[(0, 0, 4)], [(0, 2, 6)]], []),                           # 2048 postings in 8 full blocks
        ([[(0, 0, 4)], [(0, 2, 6)]], [[(2, 0, 1)]]),                # 2049 postings
        ([[(0, 0, 16)], [(0, 8, 16)]], [[(0, 16, 24)]]),            # 8192 postings in 32 blocks: exactly the 1024-thread form's capacity
        ([[(0, 0, 16)], [(0, 8, 16)]], [[(0, 16, 24)], [(2, 1, 2)]]),   # 8193 postings: a large query
        ([[(0, 0, 16)], [(0, 8, 16), (2, 1, 2)]], [[(0, 16, 24)]]),     # ... with the extra posting on the required side
        ([[(0, 0, 33)]], []),
        ([[(3, 0, 30)], [(3, 30, 50)]], [[(3, 50, 64)]]),           # 64 lists
        ([[(3, 0, 30)], [(3, 30, 50)]], [[(3, 50, 65)]]),           # 65 lists: a large query
        ([[(3, 0, 30), (3, 64, 65)], [(3, 30, 50)]], [[(3, 50, 64)]]),
        ([[(3, 0, 64)]], []),
        ([[(3, 0, 65)]], []),
        ([[(3, 0, 40), (3, 20, 80), (1, 0, 33)]], [[(3, 1, 2)]]),
    ]
    klass = [cases.query_class(lists, g, x) for g, x in queries]
    assert klass == ["tiny", "small", "tiny", "small", "tiny", "small", "small", "large", "large", "large", "small", "large", "large",
                     "small", "large", "large"]
    want = _check_batch(ctx, pool, queries)
    assert want[2].size == 2048 and want[9].size == 33 * 256 and want[6].size > 0 and want[10].size > 0 and want[13].size > 64


def test_ids_zero_and_all_ones_survive_without_tombstones(ctx):
    a = np.array([0, 5, 9, 0xFFFFFFFF], np.uint32)
    b = np.array([0, 6, 9, 0xFFFFFFFF], np.uint32)
    x = np.array([9], np.uint32)
    pool = [(ctx.encode_lists([a, b, x]), [a, b, x])]
    want = _check_batch(ctx, pool, [([[(0, 0, 1)], [(0, 1, 2)]], [[(0, 2, 3)]]), ([[(0, 0, 2)]], []), ([[(0, 1, 2)]], [[(0, 2, 3)]])])
    assert want[0].tolist() == [0, 0xFFFFFFFF] and want[1].tolist() == [0, 5, 6, 9, 0xFFFFFFFF] and want[2].tolist() == [0, 6, 0xFFFFFFFF]


def test_edges_zero_queries_all_empty_and_large_only(ctx):
    rng = np.random.default_rng(5)
    a = np.arange(0, 3000, 3, dtype=np.uint32)
    b = np.arange(1, 3000, 3, dtype=np.uint32)
    e = np.empty(0, np.uint32)
    far = np.arange(900_000, 900_100, dtype=np.uint32)
    big1 = np.unique(rng.integers(0, 400_000, 60_000, dtype=np.uint64)).astype(np.uint32)
    big2 = np.unique(rng.integers(0, 400_000, 90_000, dtype=np.uint64)).astype(np.uint32)
    ls = [a, b, e, big1, big2, far]
    pool = [(ctx.encode_lists(ls), ls)]
    for _ in _modes(ctx, ((1, 1), (0, 1))):                                      # zero queries: offsets [0], no output needed
        out, off = ctx.query_batch_groups([])
        assert off.tolist() == [0]
    off = np.full(1, 77, np.uint64)
    rc = ctx.lib.ii2_query_batch_groups(ctx.h, 0, None, None, None, None, None, None, None, None, 0, off.ctypes.data_as(_lib.u64p))
    assert rc == 0 and off[0] == 0                                               # ... and every array may be NULL
    _check_batch(ctx, pool, [([[(0, 0, 1)]], [])])                               # one query
    # no group; a required group without postings; disjoint ids; spans that do not overlap; an excluded group without postings
    want = _check_batch(ctx, pool, [([], []), ([[(0, 0, 1)], [(0, 2, 3)]], []), ([[(0, 0, 1)], [(0, 1, 2)]], []),
                                    ([[(0, 0, 2)], [(0, 5, 6)]], [[(0, 0, 1)]]), ([[(0, 2, 2)]], [])])
    assert all(w.size == 0 for w in want)
    want = _check_batch(ctx, pool, [([[(0, 0, 1)]], [[(0, 2, 3)], []])])
    assert want[0].size == a.size
    want = _check_batch(ctx, pool, [([[(0, 3, 4)], [(0, 4, 5)]], []), ([[(0, 3, 5)]], [[(0, 0, 2)]]), ([[(0, 3, 4)]], [[(0, 4, 5)]]),
                                    ([[(0, 3, 4)], [(0, 4, 5)], [(0, 0, 2)]], [])])
    assert want[0].size > 1000 and want[2].size > 1000                           # large queries only, a two-list AND among them
    # large and short ones side by side, the large ones not last
    _check_batch(ctx, pool, [([[(0, 0, 2)]], []), ([[(0, 3, 4)], [(0, 4, 5)]], [[(0, 0, 1)]]), ([[(0, 0, 1)], [(0, 0, 1)]], [[(0, 1, 2)]]),
                             ([[(0, 3, 5)]], []), ([[(0, 1, 2)]], [[(0, 1, 2)]])])


def _raw(c, qf, gf, gn, segs, first, end, out, cap, tomb=None):
    qf, gf, first, end = (np.asarray(x, np.uint64) for x in (qf, gf, first, end))
    gn = None if gn is None else np.asarray(gn, np.uint8)
    hs = (C.c_void_p * max(len(segs), 1))(*[s.h for s in segs])
    off = np.full(qf.size, 0xDEAD, np.uint64)
    rc = c.lib.ii2_query_batch_groups(c.h, qf.size - 1, qf.ctypes.data_as(_lib.u64p), gf.ctypes.data_as(_lib.u64p),
                                      gn.ctypes.data_as(_lib.u8p) if gn is not None else None, hs, first.ctypes.data_as(_lib.u64p),
                                      end.ctypes.data_as(_lib.u64p), tomb.h if tomb else None, C.c_void_p(out.data_ptr()), cap,
                                      off.ctypes.data_as(_lib.u64p))
    return rc, off, (c.lib.ii2_last_error(c.h) or b"").decode()


def test_capacity_is_all_or_nothing(ctx):
    rng = np.random.default_rng(11)
    ls = [np.unique(rng.integers(0, 50_000, n, dtype=np.uint64)).astype(np.uint32) for n in (40, 500, 3000, 20_000, 9, 700, 30_000)]
    seg = ctx.encode_lists(ls)
    pool = [(seg, ls)]
    queries = [([[(0, 0, 2)]], []), ([[(0, 1, 2)], [(0, 2, 3)]], [[(0, 0, 1)]]), ([[(0, 2, 4)]], [[(0, 5, 6)]]), ([], []),
               ([[(0, 4, 6)]], []), ([[(0, 3, 4)], [(0, 6, 7)]], [[(0, 2, 3)]])]
    want = [cases.want([ls], g, x) for g, x in queries]
    sizes = [w.size for w in want]
    total = sum(sizes)
    assert total > 20_000 and sizes[5] > 1000
    qf, gf, gn, segs, first, end = pack_group_batch(_bind(pool, queries))
    for _ in _modes(ctx, ((1, 1), (0, 1))):
        out = ctx.empty(total + 64).upload(np.full(total + 64, SENTINEL, np.uint32))
        rc, off, msg = _raw(ctx, qf, gf, gn, segs, first, end, out, total - 1)
        assert rc == -4, (rc, msg)                                               # II2_ECAPACITY
        assert np.all(out.download() == SENTINEL)                                # byte for byte unchanged
        assert np.diff(off.astype(np.int64)).tolist() == sizes and off[0] == 0   # ... and the true sizes
        rc, off, msg = _raw(ctx, qf, gf, gn, segs, first, end, out, total)
        assert rc == 0, msg
        got = out.download()
        assert np.array_equal(got[:total], np.concatenate(want)) and np.all(got[total:] == SENTINEL)
        # sizes only: no buffer, capacity 0
        rc, off2, msg = _raw(ctx, qf, gf, gn, segs, first, end, type("N", (), {"data_ptr": lambda self: 0})(), 0)
        assert rc == -4 and np.array_equal(off2, off)
        out.free()


def test_invalid_queries_are_rejected_before_anything_runs(ctx):
    ls = [np.arange(i, 500, 7, dtype=np.uint32) for i in range(70)]
    seg = ctx.encode_lists(ls)
    out = ctx.empty(4096).upload(np.full(4096, SENTINEL, np.uint32))
    good = [((0, 3), 0), ((5, 6), 1)]            # groups as ((first, end) of ONE range, flag): lists 0 .. 2 minus list 5

    def run(queries, group_first=None, flags=True):
        groups = [g for q in queries for g in q]
        qf = np.cumsum([0] + [len(q) for q in queries])
        gf = np.arange(len(groups) + 1) if group_first is None else group_first
        gn = [f for _, f in groups] if flags else None
        return _raw(ctx, qf, gf, gn, [seg] * len(groups), [r[0] for r, _ in groups], [r[1] for r, _ in groups], out, 4096)

    cases_ = {
        "no required group": ([good, good, [((0, 3), 1), ((4, 5), 1)]], None),
        "flag 2": ([good, good, [((0, 3), 0), ((4, 5), 2)]], None),
        "list index out of range": ([good, good, [((60, 71), 0)]], None),
        "list index out of range in an excluded group": ([good, good, [((0, 1), 0), ((60, 71), 1)]], None),
        "first > end": ([good, good, [((9, 4), 0)]], None),
        "group_first descending": ([good, good, [((0, 3), 0), ((4, 5), 1)], good], np.array([0, 1, 2, 3, 4, 6, 5, 7, 8])),
    }
    for _ in _modes(ctx, ((1, 1), (0, 1))):
        for what, (queries, gf) in cases_.items():
            rc, off, msg = run(queries, gf)
            assert rc == -1, (what, rc)                                          # II2_EINVAL
            assert "query 2" in msg and "ii2_query_batch_groups" in msg, (what, msg)
            assert np.all(off == 0xDEAD), what                                   # nothing written
            assert np.all(out.download() == SENTINEL), what
        rc, off, msg = run([good, good, [((0, 64), 0)]])                         # fine
        assert rc == 0, msg
        out.upload(np.full(4096, SENTINEL, np.uint32))
        rc, off, msg = _raw(ctx, [0, 1, 1], [0, 1], [0], [seg], [0], [1], out, 4096)      # query_first: fine, a query without groups
        assert rc == 0 and off.tolist() == [0, ls[0].size, ls[0].size], msg
        out.upload(np.full(4096, SENTINEL, np.uint32))
        rc, off, msg = _raw(ctx, [0, 2, 1], [0, 1, 2], [0, 0], [seg, seg], [0, 1], [1, 2], out, 4096)   # query_first descending
        assert rc == -1 and "query 1" in msg and np.all(off == 0xDEAD) and np.all(out.download() == SENTINEL), msg
    with pytest.raises(II2Error) as e:
        ctx.query_batch_groups([([[(seg, 0, 1)]], []), ([], [[(seg, 0, 1)]])])
    assert e.value.code == -1 and "query 1" in str(e.value)


def test_launches_do_not_grow_with_the_batch(ctx):
    rng = np.random.default_rng(21)
    ls = [np.unique(rng.integers(0, 100_000, int(rng.integers(5, 120)), dtype=np.uint64)).astype(np.uint32) for _ in range(200)]
    seg = ctx.encode_lists(ls)

    def batch(nq):
        qs = []
        for q in range(nq):
            a, b, x = (int(v) for v in rng.integers(0, 190, 3))
            qs.append(([[(seg, a, a + int(rng.integers(1, 6)))], [(seg, b, b + 3)]], [[(seg, x, x + 2)]] if q % 2 else []))
        return qs

    b8, b512 = batch(8), batch(512)
    ctx.query_batch_groups(b512)                                                 # (buffers grown, counts mirrored)
    ctx.set_option("profile.events", 1)
    try:
        ctx.profile_read()
        passes = {}
        for groups, _ in _modes(ctx, ((1, 1), (0, 1))):
            for qs in (b8, b512):
                ctx.query_batch_groups(qs)
                _, n = ctx.profile_read()
                passes[(groups, len(qs))] = n
    finally:
        ctx.set_option("profile.events", 0)
    print("bracketed passes (batch.groups, queries):", passes)
    assert passes[(1, 8)] == passes[(1, 512)] and 1 <= passes[(1, 8)] <= 4       # the same for any number of queries
    assert passes[(0, 8)] >= 8 and passes[(0, 512)] >= 512                       # one by one: at least one pass per query


def test_same_batch_twice_and_two_contexts_on_two_threads(ctx):
    rng = np.random.default_rng(31)
    core = cases.core_of(rng, 200_000)
    lists = cases.make_lists(rng, 200_000, n_lists=60, core=core)
    pool = _encode(ctx, lists)
    removed = np.unique(rng.integers(0, 200_000, 500, dtype=np.uint64)).astype(np.uint32)
    tomb = ctx.tombstones(removed)
    queries = cases.random_queries(rng, lists, 200)
    want = [cases.want(lists, g, x, removed) for g, x in queries]
    bound = _bind(pool, queries)
    out1, off1 = ctx.query_batch_groups(bound, tomb=tomb)
    out2, off2 = ctx.query_batch_groups(bound, tomb=tomb)
    b1, b2 = out1.download(int(off1[-1])), out2.download(int(off2[-1]))
    assert np.array_equal(off1, off2) and b1.tobytes() == b2.tobytes()
    assert np.array_equal(b1, np.concatenate(want))
    workers = [Context(0), Context(0)]
    errors, barrier = [], threading.Barrier(2)

    def run(i):
        try:
            c = workers[i]
            mine = bound if i == 0 else bound[::-1]                              # segments and tombstones made by `ctx`, used by `c`
            w = want if i == 0 else want[::-1]
            barrier.wait()
            for _ in range(3):
                out, off = c.query_batch_groups(mine, tomb=tomb)
                ids = out.download(int(off[-1]))
                assert np.array_equal(ids, np.concatenate(w)), i
                assert np.diff(off.astype(np.int64)).tolist() == [x.size for x in w], i
                out.free()
        except BaseException as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for w in workers:
        w.close()
    assert not errors, errors
