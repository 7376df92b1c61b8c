"""GPU: ii2_topk_batch - many ranked queries in one launch - against numpy (tests/topkw_cases.reference) and against the single call
(Context.topk_weighted_ranges) in the same context, bit-identical: every (case, weights, k, min_score) of tests/topkw_cases.py as
ONE batch, the lists in one segment and in two, then a batch per case with its tombstones; the cases written for the kernel's seams
(tests/topk_batch_cases.py); 16 448 queries in one call; call hygiene; the error table; the options; the scratch left zero."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from inverted_index_2_amd.engine import pack_topk_batch
from tests import atleast_cases as ac
from tests import topk_batch_cases as bc
from tests import topk_cases as tc
from tests import topkw_cases as wc
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
OK, EINVAL, ECAPACITY, ERANGE = 0, -1, -4, -5
DEFAULTS = {"batch.topk": 1, "batch.tiny": 1, "atleast.small": 1, "atleast.handoff": 1, "union.many_window_log2": 30, "union.many": 0}
WHO = "ii2_topk_batch: "
FIELDS = [f[0] for f in _lib.TopkBatchStats._fields_]


class Options:
    def __init__(self, ctx, kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set_option(k, DEFAULTS[k])


@pytest.fixture(scope="module")
def laid(ctx):
    cache = {}

    def get(case, n_segs=1):
        if (case.name, n_segs) not in cache:
            cache[case.name, n_segs] = bc.Laid(ctx, case, n_segs)
        return cache[case.name, n_segs]
    return get


_REF = {}


def ref(t, k, m, tomb):
    """(ids, scores, eligible) of the reference, computed once per (case, weights, k, min_score, tomb) and shared"""
    key = (t.name, k, m, tomb)
    if key not in _REF:
        ids, scores, hist = wc.reference(t.case, t.weights, k, m, tomb)
        _REF[key] = (ids, scores, int(hist.sum()))
    return _REF[key]


def fields(st):
    return [getattr(st, f) for f in FIELDS]


def query(L, t, k, m):
    return (L.groups, t.weights, k, m, L.exclude)


def want_stats(ctx, items, topk=1, tiny=1):
    """[n_tiny, n_small, n_single, n_empty, n_staged] of a batch of (WCase, k, min_score), by the plan export"""
    n = dict.fromkeys(bc.FORMS, 0)
    staged = 0
    for t, k, m in items:
        form, bound = bc.form_of(ctx.lib, t, k, m, topk, tiny)
        n[form] += 1
        staged += bound
    return [n["tiny"], n["small"], n["single"], n["empty"], staged]


def check_batch(ctx, queries, items, tomb_h, tomb, what, stats=None):
    """one call; every result against the reference"""
    with path_delta(ctx) as took:
        ids, scores, off, eligible, st = ctx.topk_batch(queries, tomb=tomb_h, stats=True)
    assert took == {}, what                                         # the ranked family counts no kernel path
    got_ids, got_scores = ids.download(int(off[-1])), scores.download(int(off[-1]))
    assert off[0] == 0
    for q, (t, k, m) in enumerate(items):
        want_ids, want_scores, want_eligible = ref(t, k, m, tomb)
        a, b = int(off[q]), int(off[q + 1])
        w = (what, q, t.name, k, m)
        assert b - a == want_ids.size, w
        assert np.array_equal(got_ids[a:b], want_ids), w
        assert np.array_equal(got_scores[a:b], want_scores), w
        assert int(eligible[q]) == want_eligible, w
    if stats is not None:
        assert fields(st) == stats, what
    return st


# ---- 1. the existing table as one batch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_segs", [1, 2])
def test_the_weighted_table_as_one_batch(ctx, laid, n_segs):
    items = [(t, k, m) for t in wc.CASES for m in t.min_scores for k in t.ks]
    queries = [query(laid(t.case, n_segs), t, k, m) for t, k, m in items]
    stats = want_stats(ctx, items)
    print(len(items), "queries", dict(zip(FIELDS, stats)))
    assert len(items) > 1000 and all(stats[:3])                     # every form runs
    check_batch(ctx, queries, items, None, False, ("table", n_segs), stats)


@pytest.mark.parametrize("n_segs", [1, 2])
def test_a_batch_per_case_with_its_tombstones(ctx, laid, n_segs):
    n = 0
    for t in wc.CASES:
        L = laid(t.case, n_segs)
        if L.tomb is None:
            continue
        items = [(t, k, m) for m in t.min_scores for k in t.ks]
        check_batch(ctx, [query(L, t, k, m) for _, k, m in items], items, L.tomb, True, (t.name, n_segs), want_stats(ctx, items))
        n += 1
    assert n > 20


# ---- 2. the kernel's seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", bc.CASES, ids=lambda b: b.name)
def test_seams(ctx, laid, b):
    t = b.w
    for n_segs in (1, 2):
        L = laid(t.case, n_segs)
        items = [(t, k, m) for m in t.min_scores for k in t.ks]
        queries = [query(L, t, k, m) for _, k, m in items]
        for tomb in (False, True):
            stats = want_stats(ctx, items)
            assert stats[FIELDS.index("n_" + b.form)] == len(items)
            check_batch(ctx, queries, items, L.tomb if tomb else None, tomb, (b.name, n_segs, tomb), stats)
        if n_segs == 2:
            continue
        # the single call in the same context says the same
        for tomb in (False, True):
            for _, k, m in items:
                ids, scores, n, hist, st = ctx.topk_weighted_ranges(L.groups, t.weights, k, m, L.exclude, tomb=L.tomb if tomb else None, stats=True)
                want_ids, want_scores, want_eligible = ref(t, k, m, tomb)
                assert n == want_ids.size and st.n_eligible == want_eligible, (b.name, tomb, k, m)
                assert np.array_equal(ids.download(n), want_ids) and np.array_equal(scores.download(n), want_scores), (b.name, tomb, k, m)


# ---- 3. scale ----------------------------------------------------------------------------------------------------------------------------
def test_many_queries_in_one_call(ctx, laid):
    tiny = [(bc.BY_NAME["shared_ids"].w, 5, 1), (bc.BY_NAME["required_and_excluded"].w, 2, 7), (bc.BY_NAME["highest_id"].w, 4, 1),
            (wc.BY_NAME["tie_mixed_sets-mixed"], 6, 5)]
    small = (bc.BY_NAME["binary_padded"].w, 100, 1)
    items = []
    for i in range(4096):
        items += tiny
        if i % 64 == 0:
            items.append(small)
    assert len(items) == 4 * 4096 + 64
    queries = [query(laid(t.case, 1), t, k, m) for t, k, m in items]
    stats = want_stats(ctx, items)
    assert stats[:4] == [4 * 4096, 64, 0, 0]
    ids, scores, off, eligible, st = ctx.topk_batch(queries, stats=True)
    assert fields(st) == stats
    want_ids = np.concatenate([ref(t, k, m, False)[0] for t, k, m in items])
    want_scores = np.concatenate([ref(t, k, m, False)[1] for t, k, m in items])
    sizes = [ref(t, k, m, False)[0].size for t, k, m in items]
    assert min(sizes) > 0
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64))
    assert np.array_equal(ids.download(int(off[-1])), want_ids) and np.array_equal(scores.download(int(off[-1])), want_scores)
    assert np.array_equal(eligible, np.asarray([ref(t, k, m, False)[2] for t, k, m in items], np.uint64))


# ---- raw calls ---------------------------------------------------------------------------------------------------------------------------
def sentinel_buffer(ctx, n):
    return ctx.empty(n).upload(np.full(n, SENTINEL, np.uint32))


def raw(ctx, queries, ids, scores, cap, tomb=None, off=None, eligible=None, stats=None, flags=None, group_first=None, n_queries=None):
    """the return code of one ii2_topk_batch call over pack_topk_batch(queries); flags / group_first replace the packed arrays"""
    query_first, gf, group_not, qsegs, first, end, weight, min_score, k = pack_topk_batch(queries)
    if flags is not None:
        group_not = np.asarray(flags, np.uint8)
    if group_first is not None:
        gf = np.asarray(group_first, np.uint64)
    segs = (C.c_void_p * max(len(qsegs), 1))(*[s.h for s in qsegs])
    return ctx.lib.ii2_topk_batch(ctx.h, len(queries) if n_queries is None else n_queries, query_first.ctypes.data_as(_lib.u64p), gf.ctypes.data_as(_lib.u64p),
                                  group_not.ctypes.data_as(_lib.u8p), None if weight is None else weight.ctypes.data_as(_lib.u32p),
                                  min_score.ctypes.data_as(_lib.u32p), k.ctypes.data_as(_lib.u32p), segs, first.ctypes.data_as(_lib.u64p),
                                  end.ctypes.data_as(_lib.u64p), tomb.h if tomb else None, ids.data_ptr() if ids is not None else None,
                                  scores.data_ptr() if scores is not None else None, cap, off.ctypes.data_as(_lib.u64p) if off is not None else None,
                                  eligible.ctypes.data_as(_lib.u64p) if eligible is not None else None, C.byref(stats) if stats is not None else None)


def hygiene_batch(laid):
    items = [(bc.BY_NAME["shared_ids"].w, 5, 1), (wc.BY_NAME["dense_classes-odd"], 1000, 1), (bc.BY_NAME["shared_ids"].w, 0, 1),
             (wc.BY_NAME["many_lists-pow2"], 7, 1), (wc.BY_NAME["every_score_binary-binary"], 300, 1), (bc.BY_NAME["highest_id"].w, 2, 100)]
    return items, [query(laid(t.case, 2), t, k, m) for t, k, m in items]


def test_call_hygiene(ctx, laid):
    items, queries = hygiene_batch(laid)
    want = [ref(t, k, m, False) for t, k, m in items]
    want_ids, want_scores = np.concatenate([w[0] for w in want]), np.concatenate([w[1] for w in want])
    want_off = np.concatenate([[0], np.cumsum([w[0].size for w in want])]).astype(np.uint64)
    want_eligible = np.asarray([w[2] for w in want], np.uint64)
    total = int(want_off[-1])
    assert want[2][0].size == 0 and want[2][2] > 0 and want[5][2] == 0          # k = 0 with eligible docs; min_score above W'
    stats = want_stats(ctx, items)
    assert stats[:4] == [3, 1, 1, 1]
    # nothing is written behind out_off[n], in either buffer
    ids, scores = sentinel_buffer(ctx, total + 16), sentinel_buffer(ctx, total + 16)
    off, eligible, st = np.full(len(items) + 1, 7, np.uint64), np.full(len(items), 7, np.uint64), _lib.TopkBatchStats()
    with path_delta(ctx) as took:
        assert raw(ctx, queries, ids, scores, total + 16, off=off, eligible=eligible, stats=st) == OK
    assert took == {} and fields(st) == stats
    assert np.array_equal(off, want_off) and np.array_equal(eligible, want_eligible)
    got_ids, got_scores = ids.download(), scores.download()
    assert np.array_equal(got_ids[:total], want_ids) and np.all(got_ids[total:] == SENTINEL)
    assert np.array_equal(got_scores[:total], want_scores) and np.all(got_scores[total:] == SENTINEL)
    # d_scores, eligible and stats may be NULL
    ids = sentinel_buffer(ctx, total + 16)
    off[:] = 7
    assert raw(ctx, queries, ids, None, total + 16, off=off) == OK
    got_ids = ids.download()
    assert np.array_equal(off, want_off) and np.array_equal(got_ids[:total], want_ids) and np.all(got_ids[total:] == SENTINEL)
    # cap one short: nothing written, out_off filled, eligible and stats written; then cap = out_off[n] succeeds
    ids, scores = sentinel_buffer(ctx, total + 16), sentinel_buffer(ctx, total + 16)
    off[:], eligible[:], st = 7, 7, _lib.TopkBatchStats()
    assert raw(ctx, queries, ids, scores, total - 1, off=off, eligible=eligible, stats=st) == ECAPACITY
    assert ctx.lib.ii2_last_error(ctx.h).decode().startswith(WHO)
    assert np.all(ids.download() == SENTINEL) and np.all(scores.download() == SENTINEL)
    assert np.array_equal(off, want_off) and np.array_equal(eligible, want_eligible) and fields(st) == stats
    assert raw(ctx, queries, ids, scores, int(off[-1]), off=off, eligible=eligible) == OK
    got_ids, got_scores = ids.download(), scores.download()
    assert np.array_equal(got_ids[:total], want_ids) and np.all(got_ids[total:] == SENTINEL)
    assert np.array_equal(got_scores[:total], want_scores) and np.all(got_scores[total:] == SENTINEL)
    # n_queries == 0
    off = np.full(1, 7, np.uint64)
    assert raw(ctx, [], None, None, 0, off=off) == OK and off[0] == 0
    st = _lib.TopkBatchStats(*([7] * 5))
    assert raw(ctx, [], None, None, 0, off=off, stats=st) == OK and fields(st) == [0] * 5
    assert raw(ctx, [], None, None, 0, off=None) == EINVAL


def test_empty_queries_launch_nothing(ctx, laid):
    t = wc.BY_NAME["empty_groups-odd"]                                   # n' = 3, W' = 21
    L = laid(t.case, 1)
    queries = [(L.groups, t.weights, 10, 22, L.exclude),                 # min_score above W'
               ([], None, 10, 1, []),                                    # no group
               ([[], []], [4, 9], 10, 1, []),                            # groups without ranges
               ([[(L.segs[0], 6, 7)]], [9], 10, 1, [])]                  # a group over an empty list
    off, eligible, st = np.full(5, 7, np.uint64), np.full(4, 7, np.uint64), _lib.TopkBatchStats(*([7] * 5))
    with path_delta(ctx) as took:
        assert raw(ctx, queries, None, None, 0, off=off, eligible=eligible, stats=st) == OK      # the buffers may be NULL
    assert took == {} and not off.any() and not eligible.any()
    assert fields(st) == [0, 0, 0, 4, 0]
    # an excluded group without postings is ignored, whatever its weight says
    ids, scores, off, eligible = ctx.topk_batch([(L.groups, t.weights, 16, 1, [[(L.segs[0], 6, 7)], []])])
    assert np.array_equal(ids.download(int(off[1])), wc.reference(L.case, t.weights, 16, 1)[0])


# ---- 5. the error table ----------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(ctx, laid):
    L = laid(tc.BY_NAME["basic_m2"].case, 1)
    seg = L.segs[0]
    G = L.groups
    other = [[(seg, 0, 1)], [(seg, 1, 2)]]
    wide = ctx.encode_lists([ac.A(5, 1000 + g) for g in range(256)])
    many = [[(wide, g, g + 1)] for g in range(256)]
    good = (G, [1, 2, 3], 4, 1, [])
    # (the middle query, code, what the message says, replacement flags of the batch or None)
    table = [
        ("min_score 0", (G, [1, 2, 3], 4, 0, []), EINVAL, "min_score is 0", None),
        ("weight 0", (G, [1, 0, 3], 4, 1, []), EINVAL, "group 1 has weight 0 (drop the group instead)", None),
        ("weight 256", (G, [1, 2, 256], 4, 1, []), ERANGE, "group 2", None),
        ("W' = 256", (other, [128, 128], 4, 1, []), ERANGE, "255", None),
        ("256 groups with postings", (many, None, 4, 1, []), ERANGE, "255", None),
        ("k above II2_TOPK_MAX", (G, [1, 2, 3], _lib.II2_TOPK_MAX + 1, 1, []), ERANGE, "II2_TOPK_MAX", None),
        ("no required group", ([], None, 4, 1, other), EINVAL, "no required group", None),
        ("a flag of 2", (other, [1, 1], 4, 1, []), EINVAL, "group_not", [0, 0, 0, 0, 2, 0, 0, 0]),
        ("a range that ends before it begins", ([[(seg, 2, 1)]], [1], 4, 1, []), EINVAL, "", None),
        ("a range past the segment's lists", ([[(seg, 0, 1)]], [1], 4, 1, [[(seg, 5, 7)]]), EINVAL, "", None),
    ]
    for what, middle, code, says, flags in table:
        ids, scores = sentinel_buffer(ctx, 64), sentinel_buffer(ctx, 64)
        off, eligible, st = np.full(4, 7, np.uint64), np.full(3, 7, np.uint64), _lib.TopkBatchStats(*([7] * 5))
        with path_delta(ctx) as took:
            rc = raw(ctx, [good, middle, good], ids, scores, 64, off=off, eligible=eligible, stats=st, flags=flags)
        msg = ctx.lib.ii2_last_error(ctx.h).decode()
        assert rc == code, (what, rc, msg)
        assert msg.startswith(WHO + "query 1: ") and says in msg, (what, msg)
        assert np.all(ids.download() == SENTINEL) and np.all(scores.download() == SENTINEL) and took == {}, what
        assert np.all(off == 7) and np.all(eligible == 7) and fields(st) == [7] * 5, what
    # a group_first that does not ascend inside the middle query
    ids = sentinel_buffer(ctx, 64)
    off = np.full(4, 7, np.uint64)
    assert raw(ctx, [good, (other, [1, 1], 4, 1, []), good], ids, None, 64, off=off, group_first=[0, 1, 2, 3, 5, 4, 6, 7, 8]) == EINVAL
    assert ctx.lib.ii2_last_error(ctx.h).decode().startswith(WHO + "query 1: ") and np.all(off == 7) and np.all(ids.download() == SENTINEL)
    # more than 2^20 queries; a result to write and nowhere to write it
    one = np.zeros(2, np.uint64)
    assert raw(ctx, [good], ids, None, 64, off=one, n_queries=(1 << 20) + 1) == ERANGE
    assert raw(ctx, [good], None, None, 64, off=one) == EINVAL
    assert ctx.lib.ii2_last_error(ctx.h).decode() == WHO + "output buffer is NULL"
    # the same three queries without the error
    ids, scores, off, eligible = ctx.topk_batch([good, good, good])
    want = wc.reference(L.case, [1, 2, 3], 4, 1)[0]
    assert np.array_equal(ids.download(int(off[-1])), np.concatenate([want] * 3))


# ---- 6. the options, the scratch ----------------------------------------------------------------------------------------------------------
def test_options_change_where_a_query_runs_not_what_it_returns(ctx, laid):
    items, queries = hygiene_batch(laid)
    got = {}
    for topk, tiny in ((1, 1), (1, 0), (0, 1), (0, 0)):
        with Options(ctx, {"batch.topk": topk, "batch.tiny": tiny}):
            ids, scores, off, eligible, st = ctx.topk_batch(queries, stats=True)
        assert fields(st) == want_stats(ctx, items, topk, tiny), (topk, tiny)
        got[topk, tiny] = (off, ids.download(int(off[-1])), scores.download(int(off[-1])), eligible, fields(st))
    assert got[1, 1][4][:4] == [3, 1, 1, 1] and got[1, 0][4][:4] == [0, 4, 1, 1] and got[0, 1][4][:4] == got[0, 0][4][:4] == [0, 0, 5, 1]
    for key in got:
        for a, b in zip(got[key][:4], got[1, 1][:4]):
            assert np.array_equal(a, b), key
    assert np.array_equal(got[1, 1][1], np.concatenate([ref(t, k, m, False)[0] for t, k, m in items]))


@pytest.fixture(scope="module")
def probe(ctx):
    """lists over the cases' id range that share no id with any case"""
    used = np.unique(np.concatenate([l for t in wc.CASES for l in t.case.lists] + [l for b in bc.CASES for l in b.w.case.lists]))
    near = np.asarray([2046, 2049, 4094, 4097, 65534, 65537, 99999, 100001, 131070, 131073, 199999, 200001], np.uint32)
    a = np.setdiff1d(np.union1d(np.arange(2, 1 << 18, 4099, dtype=np.uint32), near), used).astype(np.uint32)
    b = np.setdiff1d(np.arange(11, 30000, 13, dtype=np.uint32), used).astype(np.uint32)
    return ctx.encode_lists([a, b]), np.union1d(a, b).astype(np.uint32)


@pytest.mark.parametrize("wlog2", [30, 11])
def test_scratch_is_left_zero(ctx, laid, probe, wlog2):
    """the probes of test_gpu_topk_weighted.py::test_scratch_is_left_zero behind a batch that runs every form"""
    items, queries = hygiene_batch(laid)
    seg, probe_union = probe
    with Options(ctx, {"union.many_window_log2": wlog2}):
        ctx.topk_batch(queries)
    with Options(ctx, {"union.many": 1, "union.many_window_log2": wlog2}):
        u, n = ctx.union_ranges([(seg, 0, 2)])
    assert np.array_equal(u.download(n), probe_union)
    case = wc.BY_NAME["dense_classes-odd"].case
    L = laid(case, 2)
    with Options(ctx, {"atleast.handoff": 0, "atleast.small": 0, "union.many_window_log2": wlog2}):
        out, n, ast = ctx.atleast_ranges(L.groups, 2, L.exclude, stats=True)
    assert ast.form == ac.COUNT
    assert np.array_equal(out.download(n), ac.reference(case, m=2))
