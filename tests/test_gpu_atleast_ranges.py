"""GPU: ii2_atleast_ranges - the ids in at least m of n groups, minus excluded groups and tombstones - against numpy (np.unique per
group, a count per id over the groups, count >= m, setdiff1d), bit-identical: every case of tests/atleast_cases.py under every form
(the hand-offs, the one-launch form, the counting form with one and with many windows), the equivalences with ii2_andnot_ranges and
ii2_union_ranges, all-or-nothing capacity handling, the scratch left zero, and the error table."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import atleast_cases as ac
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
OK, EINVAL, ECAPACITY, ERANGE = 0, -1, -4, -5
DEFAULTS = {"atleast.small": 1, "atleast.handoff": 1, "union.many_window_log2": 30, "union.many": 0}
# (name, options, the handoff / small values expected_form takes)
MODES = [
    ("default", {}, 1, 1),
    ("small_off", {"atleast.small": 0}, 1, 0),
    ("small_capacity", {"atleast.small": 2}, 1, 2),
    ("count", {"atleast.handoff": 0, "atleast.small": 0}, 0, 0),
    ("count_windows", {"atleast.handoff": 0, "atleast.small": 0, "union.many_window_log2": 11}, 0, 0),
]
ONE_LAUNCH = {"atleast.handoff": 0, "atleast.small": 2}
COUNTING = dict(MODES[3][1])
COUNTING_WINDOWS = dict(MODES[4][1])


class Options:
    def __init__(self, ctx, kv):
        self.ctx, self.kv = ctx, kv

    def __enter__(self):
        for k, v in self.kv.items():
            self.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self.ctx.set_option(k, DEFAULTS[k])


class Laid:
    """a case's lists in n_segs segments (list i in segment i % n_segs): its groups as the ranges the entry points take"""

    def __init__(self, ctx, case, n_segs):
        self.case = case
        per = [[l for i, l in enumerate(case.lists) if i % n_segs == s] for s in range(n_segs)]
        self.segs = [ctx.encode_lists(p) for p in per]
        self.n_segs = n_segs
        self.groups = [self.ranges(g) for g in case.groups]
        self.exclude = [self.ranges(g) for g in case.exclude]
        self.tomb = ctx.tombstones(np.asarray(case.removed, np.uint32))

    def ranges(self, group):
        out = []
        for i in group:
            s, j = self.segs[i % self.n_segs], i // self.n_segs
            if out and out[-1][0] is s and out[-1][2] == j:
                out[-1] = (s, out[-1][1], j + 1)              # consecutive lists of one segment: one range
            else:
                out.append((s, j, j + 1))
        return out


@pytest.fixture(scope="module")
def laid(ctx):
    cache = {}

    def get(name, n_segs=1):
        if (name, n_segs) not in cache:
            cache[name, n_segs] = Laid(ctx, ac.BY_NAME[name], n_segs)
        return cache[name, n_segs]
    return get


def run(ctx, L, m=None, tomb=False, exclude=True):
    out, n, st = ctx.atleast_ranges(L.groups, L.case.m if m is None else m, L.exclude if exclude else (), tomb=L.tomb if tomb else None, stats=True)
    return out.download(n), st


def plan(ctx, n_counted, m, window_log2):
    planes, win, late = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert ctx.lib.ii2_atleast_plan(n_counted, m, window_log2, C.byref(planes), C.byref(win), C.byref(late)) == OK
    return planes.value, win.value, late.value


def bound(case, m=None):
    m = case.m if m is None else m
    sizes = sorted(s for s in (sum(case.lists[i].size for i in g) for g in case.groups) if s)
    return sum(sizes[:max(len(sizes) - m + 1, 0)])


# ---- every case under every form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_every_case_under_every_form(ctx, laid, case):
    req = np.concatenate([case.lists[i] for g in case.groups for i in g] + [ac.EMPTY])
    for n_segs in (1, 2):
        L = laid(case.name, n_segs)
        for name, opts, handoff, small in MODES:
            form = ac.expected_form(case, handoff, small)
            for tomb in (False, True):
                with Options(ctx, opts), path_delta(ctx) as took:
                    got, st = run(ctx, L, tomb=tomb)
                print(case.name, n_segs, name, tomb, "form", st.form, "planes", st.n_planes, "windows", st.n_windows, "late", st.n_late, "ids", got.size)
                assert np.array_equal(got, ac.reference(case, tomb=tomb)), (name, n_segs, tomb)
                assert st.form == form and st.n_counted == case.n_counted, (name, st.form, form)
                assert st.bound == (bound(case) if form != ac.NONE else 0)
                if form == ac.COUNT:
                    wlog2 = opts.get("union.many_window_log2", 30)
                    planes, win, first_late = plan(ctx, case.n_counted, case.m, wlog2)
                    span = int(req.max()) - (int(req.min()) & ~31) + 1
                    assert (st.n_planes, st.n_windows, st.n_late) == (planes, -(-span // win), case.n_counted - first_late), name
                else:
                    assert (st.n_planes, st.n_windows, st.n_late) == (0, 0, 0)
                # the call counts no kernel path of its own: only the hand-offs show up, as the code they run
                if form in (ac.NONE, ac.SMALL, ac.COUNT):
                    assert took == {}, (name, took)
                else:
                    assert took and not any("atleast" in k for k in took), (name, took)
    # without the hand-offs and the one-launch form every query that has a result to compute takes the counting form
    assert ac.expected_form(case, 0, 0) == (ac.COUNT if case.m <= case.n_counted else ac.NONE)


# ---- equivalences -----------------------------------------------------------------------------------------------------------------
EQUIV = ["basic_m2", "exclusion", "two_exclusions", "empty_groups_m3", "seams", "late_groups", "excluded_alone", "multi_block", "many_lists"]


@pytest.mark.parametrize("name", EQUIV)
@pytest.mark.parametrize("opts", [COUNTING, COUNTING_WINDOWS, ONE_LAUNCH], ids=["count", "count_windows", "one_launch"])
def test_and_or_equivalences(ctx, laid, name, opts):
    L = laid(name, 2)
    case = L.case
    n1 = case.n_counted
    nonempty = [g for g, idx in zip(L.groups, case.groups) if case.ids(idx).size]
    for tomb in (None, L.tomb):
        # m = n': ii2_andnot_ranges on the groups that have postings
        want_out, n = ctx.andnot_ranges(nonempty, L.exclude, tomb=tomb)
        want = want_out.download(n)
        with Options(ctx, opts):
            out, n, st = ctx.atleast_ranges(L.groups, n1, L.exclude, tomb=tomb, stats=True)
        assert st.form in (ac.COUNT, ac.SMALL) and np.array_equal(out.download(n), want)
        assert np.array_equal(want, np.setdiff1d(ac.reference(case, m=n1), np.asarray(case.removed, np.uint32) if tomb else ac.EMPTY))
        # m = 1 without exclusion: ii2_union_ranges on all ranges
        want_out, n = ctx.union_ranges([r for g in L.groups for r in g], tomb=tomb)
        want = want_out.download(n)
        with Options(ctx, opts):
            out, n, st = ctx.atleast_ranges(L.groups, 1, (), tomb=tomb, stats=True)
        assert st.form in (ac.COUNT, ac.SMALL) and np.array_equal(out.download(n), want)


# ---- raw calls: capacity, errors -----------------------------------------------------------------------------------------------------
def raw(ctx, groups, flags, m, out, cap, tomb=None, group_first=None, stats=None):
    """(return code, count) of one ii2_atleast_ranges call: flags = None (group_not == NULL) or one byte per group"""
    ranges = [r for g in groups for r in g]
    n = len(ranges)
    gf = [0]
    for g in groups:
        gf.append(gf[-1] + len(g))
    gf = group_first if group_first is not None else gf
    c_gf = (C.c_uint64 * len(gf))(*gf)
    c_flags = (C.c_uint8 * max(len(groups), 1))(*flags) if flags is not None else None
    segs = (C.c_void_p * max(n, 1))(*[s.h for s, _, _ in ranges])
    first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
    end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
    cnt = C.c_uint64(12345)
    rc = ctx.lib.ii2_atleast_ranges(ctx.h, len(groups), c_gf, c_flags, m, segs, first, end, tomb.h if tomb else None,
                                    out.data_ptr() if out is not None else None, cap, C.byref(cnt), C.byref(stats) if stats is not None else None)
    return rc, cnt.value


def sentinel_buffer(ctx, n):
    return ctx.empty(n).upload(np.full(n, SENTINEL, np.uint32))


@pytest.mark.parametrize("opts,name,form", [(ONE_LAUNCH, "basic_m2", ac.SMALL), (COUNTING, "basic_m2", ac.COUNT), (COUNTING, "multi_block_wide", ac.COUNT),
                                            (COUNTING_WINDOWS, "seams", ac.COUNT), (COUNTING_WINDOWS, "multi_block_wide", ac.COUNT)],
                         ids=["one_launch", "count", "count_wide", "count_windows", "count_windows_wide"])
def test_capacity_is_all_or_nothing(ctx, laid, opts, name, form):
    L = laid(name, 2)
    case = L.case
    want = ac.reference(case)
    flags = [0] * len(L.groups) + [1] * len(L.exclude)
    out = sentinel_buffer(ctx, want.size + 8)
    with Options(ctx, opts):
        st = _lib.AtleastStats()
        rc, n = raw(ctx, L.groups + L.exclude, flags, case.m, out, want.size - 1, stats=st)
        assert (rc, n) == (ECAPACITY, want.size) and st.form == form and st.bound == bound(case)
        assert "ii2_atleast_ranges" in ctx.lib.ii2_last_error(ctx.h).decode()
        assert np.all(out.download() == SENTINEL), "written despite II2_ECAPACITY"
        if opts is COUNTING_WINDOWS:
            assert st.n_windows > 1
        rc, n = raw(ctx, L.groups + L.exclude, flags, case.m, out, n)
        assert (rc, n) == (OK, want.size)
        got = out.download()
        assert np.array_equal(got[:n], want) and np.all(got[n:] == SENTINEL)


# ---- the scratch is left zero ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe(ctx):
    """lists over the cases' id range that share no id with any case"""
    used = np.unique(np.concatenate([l for c in ac.CASES for l in c.lists]))
    near = np.asarray([2046, 2049, 4094, 4097, 65534, 65537, 99999, 100001, 199999, 200001], np.uint32)
    a = np.setdiff1d(np.union1d(np.arange(2, 1 << 18, 4099, dtype=np.uint32), near), used).astype(np.uint32)
    b = np.setdiff1d(np.arange(11, 3000, 13, dtype=np.uint32), used).astype(np.uint32)
    seg = ctx.encode_lists([a, b])
    return seg, np.union1d(a, b).astype(np.uint32)


@pytest.mark.parametrize("name", ["basic_m2", "seams", "saturation_m3", "late_groups", "excluded_alone", "many_lists", "many_groups", "multi_block_wide"])
@pytest.mark.parametrize("opts", [COUNTING, COUNTING_WINDOWS], ids=["count", "count_windows"])
def test_scratch_is_left_zero(ctx, laid, probe, name, opts):
    L = laid(name, 1)
    case = L.case
    seg, probe_union = probe
    want = ac.reference(case)
    flags = [0] * len(L.groups) + [1] * len(L.exclude)
    for short in (False, True):                                  # success, then II2_ECAPACITY
        with Options(ctx, opts):
            out = sentinel_buffer(ctx, want.size + 1)
            st = _lib.AtleastStats()
            rc, n = raw(ctx, L.groups + L.exclude, flags, case.m, out, want.size - (1 if short else 0), stats=st)
            assert (rc, n, st.form) == (ECAPACITY if short else OK, want.size, ac.COUNT)
        # a leftover bitmap, plane or summary bit shows up as a ghost id: in the block-wise union over other lists ...
        with Options(ctx, {"union.many": 1, "union.many_window_log2": opts.get("union.many_window_log2", 30)}):
            u, n = ctx.union_ranges([(seg, 0, 2)])
        assert np.array_equal(u.download(n), probe_union), (name, short)
        # ... and in the same query one threshold lower
        with Options(ctx, opts):
            got, st = run(ctx, L, m=case.m - 1 if case.m > 1 else case.m)
        assert st.form == ac.COUNT
        assert np.array_equal(got, ac.reference(case, m=max(case.m - 1, 1))), (name, short)


# ---- nothing to do -------------------------------------------------------------------------------------------------------------------
def test_empty_queries_launch_nothing(ctx, laid):
    L = laid("empty_groups_m4", 1)
    for opts in (dict(), COUNTING, ONE_LAUNCH):
        with Options(ctx, opts), path_delta(ctx) as took:
            st = _lib.AtleastStats()
            assert raw(ctx, L.groups, None, 4, None, 0, stats=st) == (OK, 0)              # min_match above n' = 3: d_out may be NULL
            assert (st.form, st.n_counted, st.bound) == (ac.NONE, 3, 0)
            assert raw(ctx, [], None, 1, None, 0, group_first=[0], stats=st) == (OK, 0)   # no group
            assert (st.form, st.n_counted) == (ac.NONE, 0)
            assert raw(ctx, [[], []], [0, 1], 1, None, 0, stats=st) == (OK, 0)              # groups without ranges
            empty_list = [[(L.segs[0], 6, 7)]]
            assert raw(ctx, empty_list, [0], 1, None, 0, stats=st) == (OK, 0)               # a group over an empty list
        assert took == {}
    # an excluded group without postings is ignored
    with Options(ctx, COUNTING):
        out = sentinel_buffer(ctx, 16)
        rc, n = raw(ctx, L.groups + [[(L.segs[0], 6, 7)], []], [0] * 5 + [1, 1], 3, out, 16)
    assert rc == OK and np.array_equal(out.download()[:n], ac.reference(L.case, m=3))


# ---- the error table ----------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(ctx, laid):
    L = laid("basic_m2", 1)
    seg = L.segs[0]
    G = L.groups
    many = laid("many_groups", 1)
    other = [[(seg, 0, 1)], [(seg, 1, 2)]]
    table = [
        ("min_match 0", dict(groups=G, flags=None, m=0), EINVAL),
        ("no required group", dict(groups=other, flags=[1, 1], m=1), EINVAL),
        ("a flag of 2", dict(groups=other, flags=[0, 2], m=1), EINVAL),
        ("a range that ends before it begins", dict(groups=[[(seg, 2, 1)]], flags=None, m=1), EINVAL),
        ("a range past the segment's lists", dict(groups=[[(seg, 0, 1)], [(seg, 5, 7)]], flags=[0, 1], m=1), EINVAL),
        ("group_first does not ascend", dict(groups=other, flags=None, m=1, group_first=[0, 2, 1]), EINVAL),
        ("min_match 256 of 260 groups", dict(groups=many.groups, flags=None, m=256), ERANGE),
    ]
    for opts in (dict(), COUNTING, ONE_LAUNCH):
        for what, kw, code in table:
            out = sentinel_buffer(ctx, 64)
            st = _lib.AtleastStats(7, 7, 7, 7, 7, 7)
            with Options(ctx, opts), path_delta(ctx) as took:
                rc, n = raw(ctx, out=out, cap=64, stats=st, **kw)
            assert (rc, n) == (code, 12345), what                                           # count untouched
            assert ctx.lib.ii2_last_error(ctx.h).decode().startswith("ii2_atleast_ranges: "), what
            assert np.all(out.download() == SENTINEL) and took == {}, what
            assert [getattr(st, f[0]) for f in st._fields_] == [7] * 6, what               # stats untouched
    # a result to write and nowhere to write it
    assert raw(ctx, G, None, 2, None, 64) == (EINVAL, 12345)
    assert ctx.lib.ii2_last_error(ctx.h).decode() == "ii2_atleast_ranges: output buffer is NULL"
    # min_match = n' above 255 is the AND hand-off whatever the options say
    lists = [ac.A(5, 1000 + g) for g in range(300)]
    segs = ctx.encode_lists(lists)
    with Options(ctx, COUNTING):
        out, n, st = ctx.atleast_ranges([[(segs, g, g + 1)] for g in range(300)], 300, stats=True)
    assert st.form == ac.AND and np.array_equal(out.download(n), ac.A(5))
