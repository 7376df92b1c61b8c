"""GPU: ii2_query_batch_groups - many AND-of-ORs / NOT queries in one call (csrc/setop_groups_batch.hip + setop.cpp) - against
numpy AND against the single-query entry point (ctx.andnot_ranges) on the same queries, under (batch.groups, batch.tiny) =
(1, 1) (both forms of the batch kernel), (1, 0) (its 1024-thread form for all) and (0, 1) (every query through the single-query
path).  All comparisons are exact.  The pools, queries and expectations are tests/group_batch_cases.py (pure numpy)."""
import ctypes as C
import threading

import numpy as np
import pytest
import torch

from inverted_index_2_amd import Context, II2Error, _lib, pack_group_batch
from tests import group_batch_cases as cases
from tests.gpu_util import ctx, path_delta  # noqa: F401

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
    lists, queries = cases.CAPACITY_LISTS, cases.CAPACITY_QUERIES[:16]            # (the table: tests/group_batch_cases.py)
    pool = [(ctx.encode_lists(ls), ls) for ls in lists]
    klass = [cases.query_class(lists, g, x) for g, x in queries]
    assert klass == ["tiny", "small", "tiny", "small", "tiny", "small", "small", "large", "large", "large", "small", "large", "large",
                     "small", "large", "large"]
    want = _check_batch(ctx, pool, queries)
    assert want[2].size == 2048 and want[9].size == 33 * 256 and want[6].size > 0 and want[10].size > 0 and want[13].size > 64


def test_batch_and_single_call_admit_the_same_queries(ctx):
    """Every query of the capacity table through the batch and, where it has an excluded group, through ii2_andnot_ranges with
    andnot.small = 2 (its one-launch form up to the kernel's capacity): the two take their one-workgroup kernel for exactly the
    queries that tests/group_batch_cases.py: query_class calls tiny or small, and return the same ids."""
    lists, queries = cases.CAPACITY_LISTS, cases.CAPACITY_QUERIES
    klass = [cases.query_class(lists, g, x) for g, x in queries]
    assert klass == cases.CAPACITY_CLASSES
    pool = [(ctx.encode_lists(ls), ls) for ls in lists]
    bound = _bind(pool, queries)
    with path_delta(ctx) as d:
        out, off = ctx.query_batch_groups(bound)
    print("batch", d)
    assert d.get("gbatch.single", 0) == klass.count("large")
    ids = out.download(int(off[-1]))
    out.free()
    got = [ids[int(off[q]):int(off[q + 1])] for q in range(len(queries))]
    for q, (g, x) in enumerate(queries):
        assert np.array_equal(got[q], cases.want(lists, g, x)), q
    big = ctx.empty(max(min(sum(l.size for l in cases.lists_of(lists, g)) for g in groups) for groups, _ in queries) + 8)
    seen = set()
    ctx.set_option("andnot.small", 2)
    try:
        for q, (groups, exclude) in enumerate(bound):
            if not exclude:
                continue
            with path_delta(ctx) as d:
                _, n = ctx.andnot_ranges(groups, exclude, out=big)
            print("query", q, klass[q], d)
            if klass[q] in ("tiny", "small"):
                assert d == {"andnot.small": 1}, (q, d)
            elif klass[q] == "large":
                assert "andnot.general" in d and "andnot.small" not in d, (q, d)
            else:
                assert d == {}, (q, d)                                           # an empty query launches nothing
            assert np.array_equal(big.download(n), got[q]), q
            seen.add(klass[q] if klass[q] in ("large", "empty") else "fits")
    finally:
        ctx.set_option("andnot.small", 1)
        big.free()
    assert seen == {"fits", "large", "empty"}


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


# Malformed queries as groups of ONE range each, ((first, end), flag), and how group_first runs ("descending": its last two
# entries swapped); PINNED holds what the library before the shared planner returned for each: (code, ii2_last_error) of
# ii2_andnot_ranges on the query alone, and of ii2_query_batch_groups with it as query 2 of three.
MALFORMED = {
    "flag 2": ([((0, 3), 0), ((4, 5), 2)], None),
    "every group excluded": ([((0, 3), 1), ((4, 5), 1)], None),
    "first > end": ([((0, 3), 0), ((9, 4), 1)], None),
    "past the segment's lists": ([((60, 71), 0)], None),
    "group_first descending": ([((0, 3), 0), ((4, 5), 1)], "descending"),
    "flag 2 behind a bad range": ([((9, 4), 0), ((4, 5), 2)], None),             # the flags are checked before any range
}
_A, _B = "ii2_andnot_ranges: ", "ii2_query_batch_groups: query 2: "
PINNED = {
    "flag 2": ((-1, _A + "a group_not flag is neither 0 nor 1"), (-1, _B + "a group_not flag is neither 0 nor 1")),
    "every group excluded": ((-1, _A + "no required group (the library has no doc universe to complement)"),
                             (-1, _B + "no required group (the library has no doc universe to complement)")),
    "first > end": ((-1, _A + "bad range"), (-1, _B + "bad range")),
    "past the segment's lists": ((-1, _A + "bad range"), (-1, _B + "bad range")),
    "group_first descending": ((-1, _A + "group_first does not ascend"), (-1, _B + "group_first does not ascend")),
    "flag 2 behind a bad range": ((-1, _A + "a group_not flag is neither 0 nor 1"), (-1, _B + "a group_not flag is neither 0 nor 1")),
}
# (a segment of another device fails the same test of the range check as a bad range does: this literal is read off
# collect_ranges, NOT recorded from a run - no machine with two devices was at hand, and on one device the case is left out)
PINNED_FOREIGN = ((-1, _A + "bad range"), (-1, _B + "bad range"))


def _single_and_batch_errors(c, seg, groups, group_first, out, last_seg=None):
    """((code, message) of ii2_andnot_ranges, (code, message) of ii2_query_batch_groups with the query as number 2 of three);
    last_seg: the segment of the query's last group in place of seg"""
    good = [((0, 3), 0), ((5, 6), 1)]
    res = []
    for queries in ([groups], [good, good, groups]):
        flat = [g for q in queries for g in q]
        gf = np.arange(len(flat) + 1, dtype=np.uint64)
        if group_first == "descending":
            gf[-2:] = gf[-2:][::-1].copy()
        gn = np.array([f for _, f in flat], np.uint8)
        first, end = (np.array([r[i] for r, _ in flat], np.uint64) for i in (0, 1))
        hs = (C.c_void_p * len(flat))(*[seg.h] * (len(flat) - 1), (last_seg or seg).h)
        if len(queries) == 1:
            cnt = C.c_uint64(0xDEAD)
            rc = c.lib.ii2_andnot_ranges(c.h, len(flat), gf.ctypes.data_as(_lib.u64p), gn.ctypes.data_as(_lib.u8p), hs,
                                         first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p), None, C.c_void_p(out.data_ptr()),
                                         4096, C.byref(cnt))
            assert cnt.value == 0xDEAD
        else:
            qf = np.cumsum([0] + [len(q) for q in queries]).astype(np.uint64)
            off = np.full(qf.size, 0xDEAD, np.uint64)
            rc = c.lib.ii2_query_batch_groups(c.h, 3, qf.ctypes.data_as(_lib.u64p), gf.ctypes.data_as(_lib.u64p), gn.ctypes.data_as(_lib.u8p),
                                              hs, first.ctypes.data_as(_lib.u64p), end.ctypes.data_as(_lib.u64p), None,
                                              C.c_void_p(out.data_ptr()), 4096, off.ctypes.data_as(_lib.u64p))
            assert np.all(off == 0xDEAD)
        res.append((rc, (c.lib.ii2_last_error(c.h) or b"").decode()))
    return tuple(res)


def test_codes_and_messages_of_malformed_queries_are_pinned(ctx):
    ls = [np.arange(i, 500, 7, dtype=np.uint32) for i in range(70)]
    seg = ctx.encode_lists(ls)
    out = ctx.empty(4096).upload(np.full(4096, SENTINEL, np.uint32))
    got = {what: _single_and_batch_errors(ctx, seg, groups, gf, out) for what, (groups, gf) in MALFORMED.items()}
    print(got)
    assert got == PINNED
    # a segment of another context's device: only where a second device is there to make one (else this case is left out)
    if torch.cuda.device_count() > 1:
        other = Context(1)
        foreign = other.encode_lists(ls[:8])
        got = _single_and_batch_errors(ctx, seg, [((0, 3), 0), ((4, 5), 1)], None, out, last_seg=foreign)
        print(got)
        assert got == PINNED_FOREIGN
        foreign.free()
        other.close()
    assert np.all(out.download() == SENTINEL)
    seg.free()
    out.free()


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
