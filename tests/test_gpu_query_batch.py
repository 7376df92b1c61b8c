"""GPU: ii2_query_batch - many AND / OR queries in one call (csrc/setop_batch.hip + setop.cpp) - against numpy AND against the
single-query entry points (ctx.intersect / ctx.union / ctx.union_ranges) on the same queries, with option batch.small = 1 (the
batch kernel; with batch.tiny = 1 and 0: its 256-thread form for the tiniest queries, or the 1024-thread form for all) and 0
(every query through the single-query paths).  All comparisons are exact."""
import ctypes as C
import threading

import numpy as np
import pytest

from inverted_index_2_amd import Context, II2Error, _lib
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5


# ---- expectations -----------------------------------------------------------------------------------
def _lists_of(pool, ranges):
    """the numpy lists of ranges [(segment number, first, end), ...] over pool = [(Segment, [arrays])]"""
    return [pool[s][1][j] for s, a, b in ranges for j in range(a, b)]


def _want(pool, name, ranges, removed):
    ls = _lists_of(pool, ranges)
    if name == "or":
        w = np.unique(np.concatenate(ls)) if ls else np.empty(0, np.uint32)
    else:
        w = ls[0]
        for x in ls[1:]:
            w = np.intersect1d(w, x, assume_unique=True)
    if removed is not None:
        w = np.setdiff1d(w, removed, assume_unique=True)
    return w.astype(np.uint32)


def _queries(pool, spec):
    return [(name, [(pool[s][0], a, b) for s, a, b in ranges]) for name, ranges in spec]


def _check_batch(c, pool, spec, removed=None, tomb=None, modes=((1, 1), (1, 0), (0, 1)), singles=True):
    """spec = [("and" | "or", [(segment number, first, end), ...]), ...]: numpy, both modes, the single-query entry points"""
    want = [_want(pool, name, ranges, removed) for name, ranges in spec]
    queries = _queries(pool, spec)
    got_bytes = []
    for small in modes:                               # (batch.small, batch.tiny): both workgroup sizes, then one by one
        c.set_option("batch.small", small[0])
        c.set_option("batch.tiny", small[1])
        try:
            out, off = c.query_batch(queries, tomb=tomb)
        finally:
            c.set_option("batch.small", 1)
            c.set_option("batch.tiny", 1)
        assert off.dtype == np.uint64 and off.size == len(spec) + 1 and off[0] == 0, small
        assert np.all(np.diff(off.astype(np.int64)) >= 0), small
        ids = out.download(int(off[-1]))
        out.free()
        for q, w in enumerate(want):
            g = ids[int(off[q]):int(off[q + 1])]
            assert g.size == w.size and np.array_equal(g, w), (small, q, spec[q][0], len(_lists_of(pool, spec[q][1])), g[:8], w[:8])
        got_bytes.append(ids.tobytes())
    assert all(b == got_bytes[0] for b in got_bytes)
    if singles:
        big = c.empty(max(max((sum(l.size for l in _lists_of(pool, r)) for _, r in spec), default=0), 1) + 8)
        for q, (name, ranges) in enumerate(spec):
            rs = [(pool[s][0], a, b) for s, a, b in ranges]
            ls = [(pool[s][0], j) for s, a, b in ranges for j in range(a, b)]
            if name == "and":
                _, n = c.intersect(ls, tomb=tomb, out=big)
                assert np.array_equal(big.download(n), want[q]), ("intersect", q)
            else:
                _, n = c.union_ranges(rs, tomb=tomb, out=big)
                assert np.array_equal(big.download(n), want[q]), ("union_ranges", q)
                if 1 <= len(ls) <= 64:
                    _, n = c.union(ls, tomb=tomb, out=big)
                    assert np.array_equal(big.download(n), want[q]), ("union", q)
        big.free()
    return want


# ---- pools of lists: several segments and a view -----------------------------------------------------
def _make_pool(c, rng, universe, n_lists=90, core=None, big=True):
    def one():
        kind = rng.random()
        if kind < 0.06:
            n = 0
        elif kind < 0.55:
            n = int(rng.integers(1, 60))
        elif kind < 0.85:
            n = int(rng.integers(60, 600))
        elif kind < 0.96 or not big:
            n = int(rng.integers(600, 3000))
        else:
            n = int(rng.integers(8193, 20000))                                   # past the batch kernel's capacity on its own
        n = min(n, universe)
        l = np.unique(rng.integers(0, universe, n, dtype=np.uint64)).astype(np.uint32) if n else np.empty(0, np.uint32)
        if core is not None and n and rng.random() < 0.6:
            l = np.union1d(l, core).astype(np.uint32)
        return l

    pool = []
    for k in (n_lists, n_lists // 2, n_lists // 3):
        ls = [one() for _ in range(k)]
        pool.append((c.encode_lists(ls), ls))
    # a view (ii2_seg_select) of a run of the first segment's lists with empty slots around and between them
    seg0, ls0 = pool[0]
    run = list(range(10, 30))
    src = [-1] + run[:7] + [-1, -1] + run[7:] + [-1]
    view = c.select(seg0, src)
    pool.append((view, [ls0[j] if j >= 0 else np.empty(0, np.uint32) for j in src]))
    return pool


def _random_spec(rng, pool, n_queries):
    spec = []
    for _ in range(n_queries):
        name = "and" if rng.random() < 0.5 else "or"
        k = int(rng.choice([1, 1, 2, 2, 3, 5, 12, 33, 64]))
        ranges, have = [], 0
        while have < k:
            s = int(rng.integers(0, len(pool)))
            n = len(pool[s][1])
            ln = min(int(rng.choice([1, 1, 1, 2, 4])), k - have)
            a = int(rng.integers(0, n - ln + 1))
            ranges.append((s, a, a + ln))
            have += ln
            if rng.random() < 0.15 and have < k:                                 # the same list twice in a query
                ranges.append((s, a, a + 1))
                have += 1
        if name == "or" and rng.random() < 0.1:
            ranges.append((0, 3, 3))                                             # an empty range
        spec.append((name, ranges))
    return spec


@pytest.mark.parametrize("universe,with_tomb", [(50, False), (5_000, True), (1_000_000, False), ((1 << 32) - 1, True)])
def test_random_batches(ctx, universe, with_tomb):
    rng = np.random.default_rng(4200 + universe % 977)
    if universe > 1_000_000:
        core = np.array([0, 7, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)       # ids 0 and 0xFFFFFFFF present
    else:
        core = np.unique(rng.integers(0, universe, 12, dtype=np.uint64)).astype(np.uint32)
    pool = _make_pool(ctx, rng, universe, core=core)
    removed = tomb = None
    if with_tomb:
        removed = np.unique(np.concatenate([rng.integers(0, universe, 300, dtype=np.uint64).astype(np.uint32), core[:2]]))
        tomb = ctx.tombstones(removed)
    spec = _random_spec(rng, pool, 300)
    want = _check_batch(ctx, pool, spec, removed, tomb)
    assert sum(w.size > 0 for w in want) > 30


def test_ids_zero_and_all_ones_survive_without_tombstones(ctx):
    a = np.array([0, 5, 0xFFFFFFFF], np.uint32)
    b = np.array([0, 6, 0xFFFFFFFF], np.uint32)
    pool = [(ctx.encode_lists([a, b]), [a, b])]
    want = _check_batch(ctx, pool, [("and", [(0, 0, 2)]), ("or", [(0, 0, 2)]), ("and", [(0, 1, 2)])])
    assert want[0].tolist() == [0, 0xFFFFFFFF] and want[1].tolist() == [0, 5, 6, 0xFFFFFFFF]


def test_edges_zero_one_all_empty_and_large_only(ctx):
    rng = np.random.default_rng(5)
    a = np.arange(0, 3000, 3, dtype=np.uint32)
    b = np.arange(1, 3000, 3, dtype=np.uint32)
    e = np.empty(0, np.uint32)
    big1 = np.unique(rng.integers(0, 400_000, 60_000, dtype=np.uint64)).astype(np.uint32)
    big2 = np.unique(rng.integers(0, 400_000, 90_000, dtype=np.uint64)).astype(np.uint32)
    ls = [a, b, e, big1, big2]
    pool = [(ctx.encode_lists(ls), ls)]
    for small in (1, 0):                                                         # zero queries: offsets [0], no output needed
        ctx.set_option("batch.small", small)
        out, off = ctx.query_batch([])
        assert off.tolist() == [0]
    ctx.set_option("batch.small", 1)
    off = np.full(1, 77, np.uint64)
    rc = ctx.lib.ii2_query_batch(ctx.h, 0, None, None, None, None, None, None, None, 0, off.ctypes.data_as(_lib.u64p))
    assert rc == 0 and off[0] == 0                                               # ... and d_out may be NULL
    _check_batch(ctx, pool, [("and", [(0, 0, 1)])])                              # one query
    _check_batch(ctx, pool, [("or", [(0, 0, 2)])])
    want = _check_batch(ctx, pool, [("and", [(0, 0, 2)]), ("or", [(0, 2, 3)]), ("or", []), ("and", [(0, 1, 3)]), ("or", [(0, 2, 2)])])
    assert all(w.size == 0 for w in want)                                        # every result empty
    want = _check_batch(ctx, pool, [("and", [(0, 3, 5)]), ("or", [(0, 3, 5)]), ("and", [(0, 3, 5), (0, 0, 1)]), ("or", [(0, 0, 5)])])
    assert want[0].size > 1000                                                   # large queries only
    # large and small ones side by side, the large ones not last
    _check_batch(ctx, pool, [("or", [(0, 0, 2)]), ("and", [(0, 3, 5)]), ("and", [(0, 0, 1), (0, 0, 1)]), ("or", [(0, 3, 5)]), ("or", [(0, 1, 2)])])


def test_capacity_of_the_batch_kernel_and_one_past_it(ctx):
    full = [np.arange(i, 256 * 64 + i, 64, dtype=np.uint32) for i in range(33)]   # 33 lists of 256 postings: one full block each
    l64 = [np.arange(i, 64 * 100 + i, 100, dtype=np.uint32) for i in range(33)]   # 33 lists of 64 postings
    one = [np.array([77], np.uint32), np.array([64], np.uint32)]
    many = [np.arange(i % 7, 2000, 17 + i % 5, dtype=np.uint32) for i in range(80)]
    pool = [(ctx.encode_lists(full), full), (ctx.encode_lists(l64), l64), (ctx.encode_lists(one), one), (ctx.encode_lists(many), many)]
    spec = []
    for name in ("and", "or"):
        spec += [
            (name, [(1, 0, 32)]),                       # 2048 postings in 32 blocks: exactly the 256-thread form's capacity
            (name, [(1, 0, 33)]),                       # 33 blocks: one past it -> the 1024-thread form
            (name, [(0, 0, 8)]),                        # 2048 postings in 8 full blocks
            (name, [(0, 0, 8), (2, 0, 1)]),             # 2049 postings
            (name, [(0, 0, 32)]),                       # 8192 postings in 32 blocks: exactly the 1024-thread form's capacity
            (name, [(0, 0, 32), (2, 1, 2)]),            # 8193 postings: a large query
            (name, [(0, 0, 33)]),
            (name, [(3, 0, 64)]),                       # 64 lists
        ]
    spec += [("or", [(3, 0, 65)]), ("or", [(3, 0, 80)]), ("or", [(3, 0, 40), (3, 20, 80), (1, 0, 33)])]     # > 64 lists: by their ranges
    want = _check_batch(ctx, pool, spec)
    assert want[0].size == 0 and want[8].size == 2048 and want[12].size == 8192 and want[13].size == 8192 and want[2 * 8 + 1].size > 64


def _raw(c, op, qf, segs, first, end, out, cap, tomb=None):
    op = np.asarray(op, np.uint8)
    qf, first, end = (np.asarray(x, np.uint64) for x in (qf, first, end))
    hs = (C.c_void_p * max(len(segs), 1))(*[s.h for s in segs])
    off = np.full(op.size + 1, 0xDEAD, np.uint64)
    rc = c.lib.ii2_query_batch(c.h, op.size, op.ctypes.data_as(_lib.u8p), qf.ctypes.data_as(_lib.u64p), hs, first.ctypes.data_as(_lib.u64p),
                               end.ctypes.data_as(_lib.u64p), tomb.h if tomb else None, C.c_void_p(out.data_ptr()), cap,
                               off.ctypes.data_as(_lib.u64p))
    return rc, off, (c.lib.ii2_last_error(c.h) or b"").decode()


def test_capacity_is_all_or_nothing(ctx):
    rng = np.random.default_rng(11)
    ls = [np.unique(rng.integers(0, 50_000, n, dtype=np.uint64)).astype(np.uint32) for n in (40, 500, 3000, 20_000, 9, 700)]
    seg = ctx.encode_lists(ls)
    pool = [(seg, ls)]
    spec = [("or", [(0, 0, 2)]), ("and", [(0, 1, 3)]), ("or", [(0, 2, 4)]), ("or", []), ("or", [(0, 4, 6)]), ("and", [(0, 3, 4), (0, 2, 3)])]
    want = [_want(pool, n, r, None) for n, r in spec]
    sizes = [w.size for w in want]
    total = sum(sizes)
    assert total > 20_000
    op = [0 if n == "and" else 1 for n, _ in spec]
    rr = [r for _, rs in spec for r in rs]
    qf = np.cumsum([0] + [len(rs) for _, rs in spec])
    segs, first, end = [seg] * len(rr), [a for _, a, _ in rr], [b for _, _, b in rr]
    for small in (1, 0):
        ctx.set_option("batch.small", small)
        out = ctx.empty(total + 64).upload(np.full(total + 64, SENTINEL, np.uint32))
        rc, off, msg = _raw(ctx, op, qf, segs, first, end, out, total - 1)
        assert rc == -4, (rc, msg)                                               # II2_ECAPACITY
        assert np.all(out.download() == SENTINEL)                                # byte for byte unchanged
        assert np.diff(off.astype(np.int64)).tolist() == sizes and off[0] == 0   # ... and the true sizes
        rc, off, msg = _raw(ctx, op, qf, segs, first, end, out, total)
        assert rc == 0, msg
        got = out.download()
        assert np.array_equal(got[:total], np.concatenate(want)) and np.all(got[total:] == SENTINEL)
        # sizes only: no buffer, capacity 0
        rc, off2, msg = _raw(ctx, op, qf, segs, first, end, type("N", (), {"data_ptr": lambda self: 0})(), 0)
        assert rc == -4 and np.array_equal(off2, off)
        out.free()
    ctx.set_option("batch.small", 1)


def test_invalid_queries_are_rejected_before_anything_runs(ctx):
    ls = [np.arange(i, 500, 7, dtype=np.uint32) for i in range(70)]
    seg = ctx.encode_lists(ls)
    out = ctx.empty(4096).upload(np.full(4096, SENTINEL, np.uint32))
    good = (1, [(0, 3)])            # an OR of lists 0 .. 2

    def run(queries):
        op = [o for o, _ in queries]
        rr = [r for _, rs in queries for r in rs]
        qf = np.cumsum([0] + [len(rs) for _, rs in queries])
        return _raw(ctx, op, qf, [seg] * len(rr), [a for a, _ in rr], [b for _, b in rr], out, 4096)

    cases = {
        "an AND with no list": [good, good, (0, [])],
        "an AND with an empty range only": [good, good, (0, [(5, 5)])],
        "an AND with 65 lists": [good, good, (0, [(0, 65)])],
        "an AND with 65 lists in two ranges": [good, good, (0, [(0, 40), (40, 65)])],
        "list index out of range": [good, good, (1, [(60, 71)])],
        "first > end": [good, good, (1, [(9, 4)])],
        "unknown op": [good, good, (2, [(0, 1)])],
    }
    for small in (1, 0):
        ctx.set_option("batch.small", small)
        for what, queries in cases.items():
            rc, off, msg = run(queries)
            assert rc == -1, (what, rc)                                          # II2_EINVAL
            assert "query 2" in msg, (what, msg)                                 # the message names the query
            assert np.all(off == 0xDEAD), what                                   # nothing written
            assert np.all(out.download() == SENTINEL), what
        rc, off, msg = run([(0, [(0, 64)]), good])                               # 64 lists are fine
        assert rc == 0, msg
        out.upload(np.full(4096, SENTINEL, np.uint32))
    ctx.set_option("batch.small", 1)
    with pytest.raises(II2Error) as e:
        ctx.query_batch([("or", [(seg, 0, 1)]), ("and", [(seg, 0, 65)])])
    assert e.value.code == -1 and "query 1" in str(e.value)


def test_launches_do_not_grow_with_the_batch(ctx):
    rng = np.random.default_rng(21)
    ls = [np.unique(rng.integers(0, 100_000, int(rng.integers(5, 120)), dtype=np.uint64)).astype(np.uint32) for _ in range(200)]
    seg = ctx.encode_lists(ls)

    def batch(nq):
        qs = []
        for q in range(nq):
            a = int(rng.integers(0, 190))
            qs.append(("and", [(seg, a, a + 2)]) if q % 2 else ("or", [(seg, a, a + int(rng.integers(1, 9)))]))
        return qs

    b8, b512 = batch(8), batch(512)
    ctx.query_batch(b512)                                                        # (buffers grown, counts mirrored)
    ctx.set_option("profile.events", 1)
    try:
        ctx.profile_read()
        passes = {}
        for small in (1, 0):
            ctx.set_option("batch.small", small)
            for qs in (b8, b512):
                ctx.query_batch(qs)
                _, n = ctx.profile_read()
                passes[(small, len(qs))] = n
    finally:
        ctx.set_option("profile.events", 0)
        ctx.set_option("batch.small", 1)
    print("bracketed passes (batch.small, queries):", passes)
    assert passes[(1, 8)] == passes[(1, 512)] and 1 <= passes[(1, 8)] <= 4       # the same for any number of queries
    assert passes[(0, 8)] >= 8 and passes[(0, 512)] >= 512                       # one by one: at least one pass per query


def test_same_batch_twice_and_two_contexts_on_two_threads(ctx):
    rng = np.random.default_rng(31)
    core = np.unique(rng.integers(0, 200_000, 15, dtype=np.uint64)).astype(np.uint32)
    pool = _make_pool(ctx, rng, 200_000, n_lists=60, core=core)
    removed = np.unique(rng.integers(0, 200_000, 500, dtype=np.uint64)).astype(np.uint32)
    tomb = ctx.tombstones(removed)
    spec = _random_spec(rng, pool, 200)
    want = [_want(pool, n, r, removed) for n, r in spec]
    queries = _queries(pool, spec)
    out1, off1 = ctx.query_batch(queries, tomb=tomb)
    out2, off2 = ctx.query_batch(queries, tomb=tomb)
    b1, b2 = out1.download(int(off1[-1])), out2.download(int(off2[-1]))
    assert np.array_equal(off1, off2) and b1.tobytes() == b2.tobytes()
    assert np.array_equal(b1, np.concatenate(want))
    workers = [Context(0), Context(0)]
    errors, barrier = [], threading.Barrier(2)

    def run(i):
        try:
            c = workers[i]
            mine = queries if i == 0 else queries[::-1]                          # segments and tombstones made by `ctx`, used by `c`
            w = want if i == 0 else want[::-1]
            barrier.wait()
            for _ in range(3):
                out, off = c.query_batch(mine, tomb=tomb)
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
