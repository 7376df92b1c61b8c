"""GPU: ii2_andnot_ranges - the AND of ORs over list ranges minus excluded (NOT) groups - against numpy:
setdiff1d(reduce(intersect1d, [unique(concatenate(g)) for g in required]), concatenate(all excluded lists + removed)),
bit-identical, in the one-launch form and the general form, the latter on every path of the required part and with both filters."""
import ctypes as C
import threading
from functools import reduce

import numpy as np
import pytest

from inverted_index_2_amd import Context, II2Error, synth
from tests.gpu_util import ctx, path_delta, sorted_unique  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
ALWAYS_MARK = 1 << 40
U32 = (1 << 32) - 1
EMPTY = np.empty(0, np.uint32)


def truth(required, excluded=(), removed=()):
    """required: [[ids of a list, ...], ...] per group; excluded: the same for the excluded groups"""
    if not required:
        return EMPTY
    sets = [np.unique(np.concatenate([np.asarray(l, np.uint32) for l in g] + [EMPTY])) for g in required]
    drop = np.concatenate([np.asarray(l, np.uint32) for g in excluded for l in g] + [np.asarray(removed, np.uint32), EMPTY])
    return np.setdiff1d(reduce(np.intersect1d, sets), drop).astype(np.uint32)


class Options:
    DEFAULTS = {"intersect.ranges": 0, "intersect.ranges_mark": 64, "union.many_window_log2": 30, "union.many": 0, "andnot.small": 1,
                "profile.events": 0}

    def __init__(self, ctx, **kv):
        self.ctx, self.kv = ctx, {k.replace("__", "."): v for k, v in kv.items()}

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set_option(k, self.DEFAULTS[k])


# the four MODES of tests/test_gpu_intersect_ranges.py: the default choice, the group path with its own filter choice, forced probe,
# forced mark - each with the one-launch form on (up to its default limit) and off - once with the one-launch form up to the
# kernel's capacity (andnot.small = 2), and once more a mark over many windows (with the one-launch form up to its capacity: the
# queries over the whole id space all fit it, and a mark over 2048-doc windows would walk 2^21 windows for them)
MODES = [{}, {"intersect__ranges": 1}, {"intersect__ranges": 1, "intersect__ranges_mark": 0},
         {"intersect__ranges": 1, "intersect__ranges_mark": ALWAYS_MARK}]
ALL_MODES = [dict(m, andnot__small=s) for s in (1, 0) for m in MODES] + [{"andnot__small": 2}] + \
    [{"intersect__ranges_mark": ALWAYS_MARK, "union__many_window_log2": 11, "andnot__small": 2}]


def andnot(ctx, groups, exclude, tomb=None):
    out, n = ctx.andnot_ranges(groups, exclude, tomb=tomb)
    return out.download(n)


def check_all_modes(ctx, groups, exclude, want, tomb=None, modes=ALL_MODES):
    for m in modes:
        with Options(ctx, **m), path_delta(ctx) as took:
            got = andnot(ctx, groups, exclude, tomb)
        assert np.array_equal(got, want), m
        # one launch or the general form, never both; the one-launch form is the whole call; the forced filter is the one that ran
        small, general = took.get("andnot.small", 0), took.get("andnot.general", 0)
        assert small + general <= 1 and (small + general == 1 or not want.size), (m, took)
        assert not small or (took == {"andnot.small": 1} and m.get("andnot__small") != 0), (m, took)
        if m.get("intersect__ranges_mark") == 0:
            assert "ir.mark" not in took and "ir.mark_drop" not in took, (m, took)
        elif m.get("intersect__ranges_mark") == ALWAYS_MARK:
            assert "ir.probe" not in took and "ir.probe_drop" not in took, (m, took)


def raw(ctx, groups, flags, out, cap, tomb=None):
    """(return code, count) of one ii2_andnot_ranges call: flags = None (group_not == NULL) or one byte per group."""
    ranges = [r for g in groups for r in g]
    n = len(ranges)
    gf = [0]
    for g in groups:
        gf.append(gf[-1] + len(g))
    group_first = (C.c_uint64 * len(gf))(*gf)
    group_not = (C.c_uint8 * max(len(groups), 1))(*flags) if flags is not None else None
    segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
    first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
    end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
    cnt = C.c_uint64(12345)
    rc = ctx.lib.ii2_andnot_ranges(ctx.h, len(groups), group_first, group_not, segs, first, end, tomb.h if tomb else None,
                                   out.data_ptr() if out is not None else None, cap, C.byref(cnt))
    return rc, cnt.value


# ---- by hand ---------------------------------------------------------------------------------------
def test_by_hand(ctx):
    seg = ctx.encode_lists([np.asarray(l, np.uint32) for l in ([1, 2, 3, 5], [2, 3, 5, 9], [3])])
    check_all_modes(ctx, [[(seg, 0, 1)], [(seg, 1, 2)]], [[(seg, 2, 3)]], np.asarray([2, 5], np.uint32))
    # one required group: (a OR b) NOT c; a list both required and excluded removes its ids
    check_all_modes(ctx, [[(seg, 0, 2)]], [[(seg, 2, 3)]], np.asarray([1, 2, 5, 9], np.uint32))
    check_all_modes(ctx, [[(seg, 0, 2)]], [[(seg, 2, 3)], [(seg, 0, 1)]], np.asarray([9], np.uint32))
    check_all_modes(ctx, [[(seg, 0, 1)], [(seg, 1, 2)]], [], np.asarray([2, 3, 5], np.uint32))


def test_id_edges(ctx):
    a = np.asarray([0, 7, 1 << 31, U32 - 1, U32], np.uint32)
    b = np.asarray([0, 1, 7, 9, 1 << 31, U32], np.uint32)
    lists = [a, b, np.asarray([0], np.uint32), np.asarray([U32], np.uint32), np.asarray([0, U32], np.uint32), np.asarray([7], np.uint32)]
    seg = ctx.encode_lists(lists)
    req = [[(seg, 0, 1)], [(seg, 1, 2)]]
    for ex in ([5], [2], [3], [4], [2, 3], [5, 4]):                     # 0 and 2^32 - 1 as survivors and as excluded ids
        want = truth([[a], [b]], [[lists[i] for i in ex]])
        check_all_modes(ctx, req, [[(seg, i, i + 1)] for i in ex], want)
        check_all_modes(ctx, req, [[(seg, i, i + 1) for i in ex]], want)
    check_all_modes(ctx, req, [[(seg, 5, 6)]], truth([[a], [b]], [[lists[5]]], [U32]), ctx.tombstones(np.asarray([U32], np.uint32)))
    check_all_modes(ctx, req, [[(seg, 3, 4)]], truth([[a], [b]], [[lists[3]]], [0]), ctx.tombstones(np.asarray([0], np.uint32)))


# ---- 200 random short queries --------------------------------------------------------------------------
N_QUERIES = 200
UNIVERSES = [50, 3000, 400_000, 2_000_000, U32]


@pytest.fixture(scope="module")
def pools(ctx):
    """Per universe: three segments of 12 lists of 0 - 600 postings - the first eight mostly short (600 u^3, u uniform, at least 1), the last
    four long (400 - 600); over the whole id space 0 - 150, so that those queries always fit the one-launch form's capacity (see
    _random_queries) - and a view of the first segment with empty slots; every entry is (segment, list index, ids)."""
    rng = np.random.default_rng(2024)
    out = []
    for u in UNIVERSES:
        entries = []
        top = 150 if u == U32 else 600
        for s in range(3):
            sizes = [max(1, int(top * rng.random() ** 3)) for _ in range(8)] + [int(rng.integers(2 * top // 3, top + 1)) for _ in range(4)]
            lists = [sorted_unique(rng, min(n, u), u) for n in sizes]
            if s == 0:
                lists[3] = EMPTY
            seg = ctx.encode_lists(lists)
            entries += [(seg, j, l) for j, l in enumerate(lists)]
            if s == 0:
                src = [0, -1, 1, 2, -1, 3, 4, 5]
                view = ctx.select(seg, src)
                entries += [(view, i, lists[j] if j >= 0 else EMPTY) for i, j in enumerate(src)]
        out.append(entries)
    return out


def _random_queries(pools):
    """[(required groups, excluded groups) of pool entries]: 1 - 4 required and 0 - 3 excluded groups of 1 - 6 lists; every fifth
    one has 4 + 3 groups of 6 of the long lists - too large for the one-launch kernel - and is drawn from the universes up to 2M
    docs (a mark over 2048-doc windows walks the whole doc span); the others draw from the mostly short lists and the view."""
    rng = np.random.default_rng(99)
    qs = []
    for q in range(N_QUERIES):
        big = q % 5 == 4
        pool = pools[int(rng.integers(1, 4))] if big else pools[int(rng.integers(0, len(pools)))]
        long_ones = [e for e in pool if e[1] >= 8]
        short_ones = [e for e in pool if e[1] < 8]
        n_req, n_ex = (4, 3) if big else (int(rng.integers(1, 5)), int(rng.integers(0, 4)))
        if big:
            pick = lambda: [long_ones[int(i)] for i in rng.integers(0, len(long_ones), 6)]
        else:
            pick = lambda: [short_ones[int(i)] for i in rng.integers(0, len(short_ones), int(rng.integers(1, 7)))]
        req = [pick() for _ in range(n_req)]
        ex = [pick() for _ in range(n_ex)]
        if rng.random() < 0.3:
            req[0].append(req[0][0])                                    # the same list twice in a group
        if n_req > 1 and rng.random() < 0.3:
            req[1].append(req[0][-1])                                   # ... and in two groups
        if n_ex and rng.random() < 0.3:
            ex[0].append(req[-1][0])                                    # ... and both required and excluded
        if not big and rng.random() < 0.3:                              # a run of lists of one segment: one range (see _ranges)
            k = int(rng.integers(0, 9))
            (ex[0] if n_ex and rng.random() < 0.5 else req[-1]).extend(pool[k:k + 3])
        qs.append((req, ex))
    return qs


def _ranges(entries):
    """one range per entry; neighbours that continue a run of lists of one segment are one range"""
    out = []
    for s, j, _ in entries:
        if out and out[-1][0] is s and out[-1][2] == j:
            out[-1] = (s, out[-1][1], j + 1)
        else:
            out.append((s, j, j + 1))
    return out


WORK_LIMIT = 32768          # postings x lists up to which the one-launch form is the default (include/ii2.h, conventions)


def _one_launch(req, ex):
    """The documented limits, on the host: the non-empty lists of the query - the excluded ones only when their doc span meets
    the required groups' common span - are at most 64 and hold at most 8192 postings in at most 128 blocks: "capacity"; with
    postings x lists <= WORK_LIMIT as well: "default"; else "general".  None: no launch."""
    spans = []
    for g in req:
        ls = [l for _, _, l in g if l.size]
        if not ls:
            return None
        spans.append((min(int(l[0]) for l in ls), max(int(l[-1]) for l in ls)))
    clo, chi = max(s[0] for s in spans), min(s[1] for s in spans)
    if clo > chi:
        return None
    lists = [l for g in req for _, _, l in g if l.size]
    lists += [l for g in ex for _, _, l in g if l.size and int(l[0]) <= chi and int(l[-1]) >= clo]
    post = sum(l.size for l in lists)
    if not (len(lists) <= 64 and post <= 8192 and sum((l.size + 255) // 256 for l in lists) <= 128):
        return "general"
    return "default" if post * len(lists) <= WORK_LIMIT else "capacity"


def test_random_queries_cover_both_forms(pools):
    forms = [_one_launch(req, ex) for req, ex in _random_queries(pools)]
    print("forms of the random queries:", {f: forms.count(f) for f in ("default", "capacity", "general", None)})
    assert forms.count("default") >= 100               # the one-launch form as a caller gets it
    assert forms.count("capacity") >= 10               # ... and up to the kernel's capacity (andnot.small = 2)
    assert forms.count("general") >= 20                # too large for the kernel


@pytest.mark.parametrize("with_tomb", [False, True])
def test_random_queries(ctx, pools, with_tomb):
    rng = np.random.default_rng(5)
    nonempty = 0
    for q, (req, ex) in enumerate(_random_queries(pools)):
        removed, tomb = (), None
        if with_tomb:
            base = truth([[l for _, _, l in g] for g in req])
            removed = np.concatenate([base[::3], sorted_unique(rng, 40, max(int(base[-1]) if base.size else 50, 50))]).astype(np.uint32)
            tomb = ctx.tombstones(removed)
        want = truth([[l for _, _, l in g] for g in req], [[l for _, _, l in g] for g in ex], removed)
        nonempty += want.size > 0
        groups, exclude = [_ranges(g) for g in req], [_ranges(g) for g in ex]
        for m in ALL_MODES:
            with Options(ctx, **m):
                got = andnot(ctx, groups, exclude, tomb)
            assert np.array_equal(got, want), (m, q)
    assert nonempty > 20


def test_null_and_all_zero_flags_are_intersect_ranges(ctx, pools):
    for m in ({}, {"andnot__small": 2}, {"andnot__small": 0}, {"intersect__ranges": 1}):
        with Options(ctx, **m):
            for q, (req, ex) in enumerate(_random_queries(pools)):
                groups = [_ranges(g) for g in req + ex]                 # all of them required
                out, n = ctx.intersect_ranges(groups)
                want = out.download(n)
                cap = max(out.count, 1)
                for flags in (None, [0] * len(groups)):
                    buf = ctx.empty(cap)
                    rc, cnt = raw(ctx, groups, flags, buf, cap)
                    assert rc == 0 and cnt == want.size, (m, q, flags)
                    assert np.array_equal(buf.download(cnt), want), (m, q, flags)


# ---- large, reduced C2 shape --------------------------------------------------------------------------
D_LARGE = 4_000_000


def _cut(l, k):
    hi = int(l.max()) + 1
    cut = np.searchsorted(l, np.linspace(0, hi, k + 1).astype(np.int64))
    return [l[cut[s]:cut[s + 1]] for s in range(k)]


@pytest.fixture(scope="module")
def large(ctx):
    r2, r3, r5 = (synth.zipf_list(r, D_LARGE) for r in (2, 3, 5))
    whole = ctx.encode_lists([r2, r3, r5])
    p2, p3 = _cut(r2, 4), _cut(r3, 4)
    parts = [ctx.encode_lists([p2[s], p3[s]]) for s in range(4)]
    return dict(r2=r2, r3=r3, r5=r5, whole=whole, parts=parts)


def test_large_two_dense_lists(ctx, large):
    w = large["whole"]
    check_all_modes(ctx, [[(w, 0, 1)]], [[(w, 1, 2)]], truth([[large["r2"]]], [[large["r3"]]]))


def test_large_terms_cut_over_segments(ctx, large):
    w, parts = large["whole"], large["parts"]
    groups = [[(p, 0, 1) for p in parts], [(w, 2, 3)]]
    exclude = [[(p, 1, 2) for p in parts]]
    want = truth([[large["r2"]], [large["r5"]]], [[large["r3"]]])
    assert want.size > 1000
    check_all_modes(ctx, groups, exclude, want)
    removed = want[::5]
    check_all_modes(ctx, groups, exclude, np.setdiff1d(want, removed), ctx.tombstones(removed))


def test_large_dense_list_not_2000_short_lists(ctx, large):
    rng = np.random.default_rng(8)
    short = [sorted_unique(rng, int(rng.integers(1, 300)), D_LARGE) for _ in range(2000)]
    seg = ctx.encode_lists(short)
    w = large["whole"]
    want = truth([[large["r2"]]], [short])
    assert 0 < want.size < large["r2"].size
    check_all_modes(ctx, [[(w, 0, 1)]], [[(seg, 0, 2000)]], want)
    check_all_modes(ctx, [[(w, 0, 1)]], [[(seg, 0, 700)], [(seg, 700, 2000)]], want)     # the excluded groups are one logical group


def test_large_excluded_superset_leaves_the_buffer_alone(ctx, large):
    w = large["whole"]
    sup = ctx.encode_lists([np.union1d(large["r2"], large["r5"]).astype(np.uint32)])
    cap = large["r2"].size + 16
    out = ctx.empty(cap).upload(np.full(cap, SENTINEL, np.uint32))
    for m in ALL_MODES:
        with Options(ctx, **m):
            assert raw(ctx, [[(w, 0, 1)], [(sup, 0, 1)]], [0, 1], out, cap) == (0, 0), m
            assert raw(ctx, [[(w, 0, 1)], [(w, 2, 3)], [(sup, 0, 1)]], [0, 0, 1], out, cap) == (0, 0), m
    assert np.all(out.download() == SENTINEL)


def test_large_exclusions_that_remove_nothing(ctx, large):
    w, parts = large["whole"], large["parts"]
    far = ctx.encode_lists([np.arange(D_LARGE + 10, D_LARGE + 50_000, 3, dtype=np.uint32), EMPTY, EMPTY])   # beyond every required doc
    groups = [[(p, 0, 1) for p in parts], [(w, 2, 3)]]
    out, n = ctx.intersect_ranges(groups)
    want = out.download(n)
    assert np.array_equal(want, truth([[large["r2"]], [large["r5"]]]))
    check_all_modes(ctx, groups, [[(far, 0, 1)]], want)                                  # a span disjoint from the required one
    check_all_modes(ctx, groups, [[(far, 1, 3)], [], [(far, 2, 2)]], want)              # excluded groups that are all empty
    # the excluded span must not narrow the required one: a short excluded list in the middle
    mid = ctx.encode_lists([want[want.size // 2: want.size // 2 + 3]])
    check_all_modes(ctx, groups, [[(mid, 0, 1)]], np.delete(want, np.arange(want.size // 2, want.size // 2 + 3)))


# ---- errors and capacity --------------------------------------------------------------------------------
def test_errors_leave_the_buffer_alone(ctx, pools):
    seg = pools[2][0][0]
    out = ctx.empty(4096).upload(np.full(4096, SENTINEL, np.uint32))
    assert raw(ctx, [], [], None, 0) == (0, 0)                                           # no group
    for m in ({}, {"andnot__small": 2}, {"andnot__small": 0}):
        with Options(ctx, **m):
            assert raw(ctx, [[(seg, 0, 1)], [(seg, 1, 2)]], [1, 1], out, 4096)[0] == -1     # every group excluded
            assert "no required group" in ctx.lib.ii2_last_error(ctx.h).decode()
            assert raw(ctx, [[(seg, 0, 1)], [(seg, 1, 2)]], [0, 2], out, 4096)[0] == -1     # a flag of 2
            assert raw(ctx, [[(seg, 0, 1)], [(seg, 5, 4)]], [0, 1], out, 4096)[0] == -1     # a bad range
            assert "ii2_andnot_ranges" in ctx.lib.ii2_last_error(ctx.h).decode()
            assert raw(ctx, [[(seg, 0, 1)], [(seg, 0, 13)]], [0, 1], out, 4096)[0] == -1    # past the segment's lists
            assert raw(ctx, [[(seg, 0, 13)], [(seg, 0, 1)]], None, out, 4096)[0] == -1      # group_not == NULL: ii2_intersect_ranges' error
            assert "ii2_intersect_ranges" in ctx.lib.ii2_last_error(ctx.h).decode()
            # a required group without postings: count 0, d_out may be NULL
            assert raw(ctx, [[(seg, 3, 4)], [(seg, 1, 2)]], [0, 1], None, 0) == (0, 0)
            assert raw(ctx, [[(seg, 1, 2)], [(seg, 3, 4)], [(seg, 2, 3)]], [0, 0, 1], None, 0) == (0, 0)
    import torch
    if torch.cuda.device_count() > 1:                                                    # a segment of another context's device
        other = Context(1)
        foreign = other.encode_lists([np.arange(10, dtype=np.uint32)])
        assert raw(ctx, [[(seg, 0, 1)], [(foreign, 0, 1)]], [0, 1], out, 4096)[0] == -1
        assert raw(ctx, [[(foreign, 0, 1)], [(seg, 0, 1)]], [0, 1], out, 4096)[0] == -1
        foreign.free()
        other.close()
    assert np.all(out.download() == SENTINEL)
    with pytest.raises(II2Error):
        ctx.andnot_ranges([], [[(seg, 0, 1)]])


def _capacity_case(ctx, groups, flags, want):
    assert want.size > 1
    out = ctx.empty(want.size + 64).upload(np.full(want.size + 64, SENTINEL, np.uint32))
    rc, cnt = raw(ctx, groups, flags, out, want.size - 1)
    assert rc == -4 and cnt == want.size                                   # II2_ECAPACITY, the size needed
    assert np.all(out.download() == SENTINEL)                              # nothing written
    rc, cnt = raw(ctx, groups, flags, out, want.size)
    assert rc == 0 and cnt == want.size
    assert np.array_equal(out.download(cnt), want)
    assert np.all(out.download()[cnt:] == SENTINEL)


def test_capacity_all_or_nothing(ctx, large):
    rng = np.random.default_rng(4)
    # short queries: the result is the shorter required list minus the excluded ids; with an excluded list that hits nothing the
    # result is the whole shorter list (cap = count is then enough for the one-launch form, cap = count - 1 is not)
    a = sorted_unique(rng, 500, 100_000)
    lists = [a, np.union1d(a, sorted_unique(rng, 300, 100_000)).astype(np.uint32), a[::9], np.setdiff1d(np.arange(100, 900, dtype=np.uint32), a)]
    seg = ctx.encode_lists(lists)
    two = [[(seg, 0, 1)], [(seg, 1, 2)]]
    # long queries: a dense list, a subset of it, a few excluded ids - and an exclusion that does not reach it (the copy)
    big = large["r2"]
    sub = big[::7]
    s2 = ctx.encode_lists([big, sub, sub[::11], np.asarray([D_LARGE + 5], np.uint32)])
    long2 = [[(s2, 0, 1)], [(s2, 1, 2)]]
    cases = [(two + [[(seg, 2, 3)]], [0, 0, 1], truth([[lists[0]], [lists[1]]], [[lists[2]]])),
             (two + [[(seg, 3, 4)]], [0, 0, 1], a),
             (two, [0, 0], a),
             (long2 + [[(s2, 2, 3)]], [0, 0, 1], truth([[big], [sub]], [[sub[::11]]])),
             (long2 + [[(s2, 3, 4)]], [0, 0, 1], sub),
             (long2, [0, 0], sub)]
    for m in ({}, {"andnot__small": 2}, {"andnot__small": 0}, {"andnot__small": 0, "intersect__ranges_mark": 0}, {"andnot__small": 0, "intersect__ranges_mark": ALWAYS_MARK},
              {"intersect__ranges": 1, "intersect__ranges_mark": 0}, {"intersect__ranges": 1, "intersect__ranges_mark": ALWAYS_MARK}):
        with Options(ctx, **m):
            for groups, flags, want in cases:
                _capacity_case(ctx, groups, flags, want)
    with pytest.raises(II2Error):
        ctx.andnot_ranges(long2, [[(s2, 2, 3)]], out=ctx.empty(4))


# ---- launches, scratch, threads ----------------------------------------------------------------------------
def test_one_launch_form_is_one_pass(ctx, pools):
    e = [x for x in pools[2] if x[2].size > 50]
    groups = [_ranges(e[0:2]), _ranges(e[2:4])]
    exclude = [_ranges(e[4:6])]
    assert _one_launch([e[0:2], e[2:4]], [e[4:6]]) == "default"
    passes = {}
    with Options(ctx, profile__events=1):
        ctx.profile_read()
        for small in (1, 0):
            with Options(ctx, andnot__small=small), path_delta(ctx) as took:
                andnot(ctx, groups, exclude)
                _, passes[small] = ctx.profile_read()
            assert (took == {"andnot.small": 1}) if small else (took.get("andnot.general") == 1 and "andnot.small" not in took), took
    print("bracketed passes (andnot.small):", passes)
    assert passes[1] == 1
    assert passes[0] >= 2


def test_scratch_is_clean_after_a_mark(ctx, large):
    rng = np.random.default_rng(12)
    short = [sorted_unique(rng, int(rng.integers(1, 300)), D_LARGE) for _ in range(300)]
    seg = ctx.encode_lists(short)
    w = large["whole"]
    want = truth([[large["r5"]]], [short])
    for log2 in (30, 14):
        with Options(ctx, andnot__small=0, intersect__ranges_mark=ALWAYS_MARK, union__many_window_log2=log2):
            assert np.array_equal(andnot(ctx, [[(w, 2, 3)]], [[(seg, 0, 300)]]), want)
            with Options(ctx, union__many=1):
                u, n = ctx.union_ranges([(seg, 0, 300)])
                assert np.array_equal(u.download(n), np.unique(np.concatenate(short)))
                u, n = ctx.union_ranges([(w, 2, 3), (seg, 0, 300)])
                assert np.array_equal(u.download(n), np.unique(np.concatenate(short + [large["r5"]])))


def test_two_contexts_on_two_threads(ctx, pools):
    queries = _random_queries(pools)
    wants = [truth([[l for _, _, l in g] for g in req], [[l for _, _, l in g] for g in ex]) for req, ex in queries]
    errors = []

    def work(first, small):
        try:
            c = Context(0)
            c.set_option("andnot.small", small)
            for q in range(first, first + 50):
                req, ex = queries[q]
                out, n = c.andnot_ranges([_ranges(g) for g in req], [_ranges(g) for g in ex])
                assert np.array_equal(out.download(n), wants[q]), q
            c.close()
        except Exception as e:                                             # noqa: BLE001
            errors.append(e)

    ts = [threading.Thread(target=work, args=a) for a in ((0, 1), (100, 0))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
