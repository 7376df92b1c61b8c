"""GPU: ii2_dict_match (csrc/dict_match.hip) - every case of tests/match_cases.py through the kernels with the LDS stage and
without it; runs at the workgroup boundary of 256 terms, at a dictionary's first and last term and the largest run count; a run
across three workgroups; one very long term that sends its workgroup alone to global memory, and one astride a workgroup edge,
which the workgroup beside it reads from global memory while its own terms are staged; the two-call capacity protocol;
every argument error with the outputs verified untouched; no patterns; and the runs fed verbatim to ii2_union_ranges and
ii2_intersect_ranges against plain Python sets.  The kernel-path counters must not move."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from inverted_index_2_amd.engine import II2Error
from tests import match_cases
from tests.gpu_util import ctx, path_delta  # noqa: F401
from tests.match_cases import CONTAINS, GLOB, NOCASE, SUFFIX

pytestmark = pytest.mark.gpu

FILL64, FILL32 = 0xABABABABABABABAB, 0xCDCDCDCD


@pytest.fixture(scope="module")
def resident(ctx):
    """the dictionaries of every case, made resident once"""
    made = {c.name: [ctx.dictionary(d) for d in c.dicts] for c in match_cases.CASES}
    yield made
    for dicts in made.values():
        for d in dicts:
            d.free()


def _check(got, want):
    run_off, first, end, which, st = got
    w_off, w_first, w_end, w_which, w_matched = want
    assert run_off.tolist() == w_off
    assert first.tolist() == w_first and end.tolist() == w_end and which.tolist() == w_which
    assert st.n_runs == w_off[-1] and st.n_matched == w_matched


@pytest.mark.parametrize("stage", (1, 0))
@pytest.mark.parametrize("case", match_cases.CASES, ids=lambda c: c.name)
def test_table(ctx, resident, case, stage):
    ctx.set_option("match.stage", stage)
    try:
        with path_delta(ctx) as moved:
            got = ctx.dict_match(resident[case.name], case.patterns, np.array(case.kinds, np.uint8))
    finally:
        ctx.set_option("match.stage", 1)
    _check(got, match_cases.expected_table(case))
    st = got[4]
    n_wg = sum((len(d) + 255) // 256 for d in case.dicts)
    assert st.n_terms == sum(len(d) for d in case.dicts)
    assert (st.n_staged, st.n_global) == ((n_wg, 0) if stage else (0, n_wg))
    assert moved == {}                                         # not a set operation: no kernel path is counted


def _numbered(n, hit):
    """n sorted terms of 6 bytes; term i ends in `x` where hit(i), else in `o`"""
    return [b"%05d" % i + (b"x" if hit(i) else b"o") for i in range(n)]


@pytest.mark.parametrize("stage", (1, 0))
@pytest.mark.parametrize("n", (255, 256, 257, 512))
def test_workgroup_boundaries(ctx, n, stage):
    """every term matches, none, and alternate terms (both phases): runs across the boundary, at both ends, the most runs"""
    shapes = {"all": lambda i: True, "none": lambda i: False, "even": lambda i: i % 2 == 0, "odd": lambda i: i % 2 == 1,
              "but-the-boundary": lambda i: i not in (255, 256), "only-the-boundary": lambda i: i in (255, 256),
              "last-of-each": lambda i: i % 256 == 255, "first-of-each": lambda i: i % 256 == 0}
    names = list(shapes)
    dicts = [_numbered(n, shapes[name]) for name in names]
    res = [ctx.dictionary(d) for d in dicts]
    case = match_cases.Case("boundary", dicts, [b"x", b"*x", b"x", b"?????o"], [SUFFIX, GLOB, CONTAINS | NOCASE, GLOB])
    ctx.set_option("match.stage", stage)
    try:
        got = ctx.dict_match(res, case.patterns, np.array(case.kinds, np.uint8))
    finally:
        ctx.set_option("match.stage", 1)
    _check(got, match_cases.expected_table(case._replace(name=f"boundary-{n}")))
    run_off = got[0]
    k = len(names)
    per = lambda p, name: int(run_off[p * k + names.index(name) + 1] - run_off[p * k + names.index(name)])
    assert per(0, "all") == 1 and per(0, "none") == 0 and per(0, "even") == (n + 1) // 2 and per(0, "odd") == n // 2
    assert per(3, "all") == 0 and per(3, "none") == 1 and per(3, "even") == n // 2
    for d in res:
        d.free()


def test_a_run_across_three_workgroups(ctx):
    hit = lambda i: 200 <= i < 700 or i == 0 or i == 899
    terms = _numbered(900, hit)
    d = ctx.dictionary(terms)
    run_off, first, end, st = d.match([b"x", b"o"], SUFFIX)
    assert run_off.tolist() == [0, 3, 5]
    assert list(zip(first.tolist(), end.tolist())) == [(0, 1), (200, 700), (899, 900), (1, 200), (700, 899)]
    assert st.n_terms == 900 and st.n_matched == 2 * 900 - 900 and st.n_staged == 4 and st.n_global == 0
    # one kind for all the patterns may be a numpy scalar
    again = d.match([b"x", b"o"], np.uint8(SUFFIX))
    assert again[0].tolist() == [0, 3, 5] and again[1].tolist() == first.tolist() and again[2].tolist() == end.tolist()
    d.free()


def test_one_very_long_term_takes_the_global_path_alone(ctx):
    long_term = b"m" * 39_990 + b"needle" + b"mmmm"                     # 40 000 bytes: no stage holds its workgroup
    terms = sorted([b"%06d" % i + (b"needle" if i % 7 == 0 else b"") for i in range(1500)] + [long_term])
    at = terms.index(long_term)
    d = ctx.dictionary(terms)
    case = match_cases.Case("long-term", [terms], [b"needle", b"NEEDLE", b"m*needle*", b"needlemmmm", b"needle"],
                            [CONTAINS, CONTAINS | NOCASE, GLOB, SUFFIX, SUFFIX])
    got = ctx.dict_match([d], case.patterns, np.array(case.kinds, np.uint8))
    _check(got, match_cases.expected_table(case))
    st = got[4]
    assert st.n_global == 1 and st.n_staged == (len(terms) + 255) // 256 - 1 and st.n_staged > 0
    assert any(f <= at < e for f, e in zip(got[1][int(got[0][2]):int(got[0][3])].tolist(), got[2][int(got[0][2]):int(got[0][3])].tolist()))
    d.free()


def test_a_long_term_astride_a_workgroup_edge(ctx):
    """term 256 (255) of 512 carries 20 000 bytes more: its own workgroup goes to global memory, the one next to it stages its
    terms but not that neighbour (staged, not wide) and matches it from global memory.  The long term holds an `x` and ends in
    `o`: it joins the CONTAINS run around it and breaks the SUFFIX run - one ends exactly at it, one starts right behind it."""
    tail = b"y" * 19_999 + b"o"
    ats = (256, 255)
    dicts = []
    for at in ats:
        terms = _numbered(512, lambda i: i % 10 != 0)
        assert terms[at].endswith(b"x")
        terms[at] += tail
        dicts.append(terms)
    case = match_cases.Case("long-term-astride", dicts, [b"x", b"x", b"y", b"o"], [SUFFIX, CONTAINS, CONTAINS, SUFFIX])
    want = match_cases.expected_table(case)
    off, first, end = want[0], want[1], want[2]
    runs = lambda p, s: list(zip(first[off[p * 2 + s]:off[p * 2 + s + 1]], end[off[p * 2 + s]:off[p * 2 + s + 1]]))
    for s, at in enumerate(ats):
        assert any(e == at for _, e in runs(0, s)) and any(f == at + 1 for f, _ in runs(0, s))       # SUFFIX x: broken at the long term
        assert (251, 260) in runs(1, s) and runs(2, s) == [(at, at + 1)] and (at, at + 1) in runs(3, s)      # CONTAINS x: across it
    res = [ctx.dictionary(d) for d in dicts]
    got = ctx.dict_match(res, case.patterns, np.array(case.kinds, np.uint8))
    _check(got, want)
    assert got[4].n_staged == 2 and got[4].n_global == 2
    for d in res:
        d.free()


def _raw_setup(ctx):
    terms = _numbered(600, lambda i: i % 3 == 0)
    d = ctx.dictionary(terms)
    pats = [b"x", b"o", b"0*"]
    blob, off = match_cases.flat(pats)
    blob, off = np.frombuffer(blob, np.uint8).copy(), np.array(off, np.uint64)
    kinds = np.array([SUFFIX, SUFFIX, GLOB], np.uint8)
    case = match_cases.Case("raw", [terms, terms], pats, kinds.tolist())
    return d, blob, off, kinds, match_cases.expected_table(case)


def test_capacity_protocol(ctx):
    d, blob, off, kinds, want = _raw_setup(ctx)
    w_off, w_first, w_end, w_which, w_matched = want
    need = w_off[-1]
    assert need == 2 * (200 + 200 + 1)
    for cap, null_runs in ((need - 1, False), (0, False), (0, True)):
        run_off = np.full(7, FILL64, np.uint64)
        first, end, which = np.full(need + 8, FILL64, np.uint64), np.full(need + 8, FILL64, np.uint64), np.full(need + 8, FILL32, np.uint32)
        args = (None, None, None) if null_runs else (first, end, which)
        rc, st = ctx.dict_match_flat([d, d], blob, off, kinds, run_off, *args, cap)
        assert rc == -4                                                    # II2_ECAPACITY
        assert run_off.tolist() == w_off                                   # run_off and the stats are complete ...
        assert (st.n_terms, st.n_matched, st.n_runs, st.n_staged, st.n_global) == (1200, w_matched, need, 6, 0)
        assert (first == FILL64).all() and (end == FILL64).all() and (which == FILL32).all()      # ... the runs untouched
        rc, st2 = ctx.dict_match_flat([d, d], blob, off, kinds, run_off, first, end, which, int(run_off[-1]))      # the second call is exact
        assert rc == 0 and first[:need].tolist() == w_first and end[:need].tolist() == w_end and which[:need].tolist() == w_which
        assert (first[need:] == FILL64).all() and (end[need:] == FILL64).all() and (which[need:] == FILL32).all()
        assert (st2.n_matched, st2.n_runs) == (w_matched, need)
    # run_dict may be NULL
    first, end = np.full(need, FILL64, np.uint64), np.full(need, FILL64, np.uint64)
    rc, _ = ctx.dict_match_flat([d, d], blob, off, kinds, run_off, first, end, None, need)
    assert rc == 0 and first.tolist() == w_first and end.tolist() == w_end
    # the wrapper makes the second call itself
    small = ctx.dictionary(_numbered(20_000, lambda i: i % 2 == 0))
    run_off, first, end, st = small.match([b"x"], SUFFIX)
    assert run_off.tolist() == [0, 10_000] and first.tolist() == list(range(0, 20_000, 2)) and (end - first == 1).all() and st.n_runs == 10_000
    small.free()
    d.free()


def test_argument_errors_leave_the_outputs_untouched(ctx):
    d, blob, off, kinds, want = _raw_setup(ctx)
    need = want[0][-1]
    run_off = np.full(7, FILL64, np.uint64)
    first, end, which = np.full(need, FILL64, np.uint64), np.full(need, FILL64, np.uint64), np.full(need, FILL32, np.uint32)
    stats = np.full(4, FILL64, np.uint64)
    arr = (C.c_void_p * 2)(d.h, d.h)
    p = lambda a: a.ctypes.data if a is not None else None

    def call(k=2, dicts=arr, n=3, b=blob, o=off, kd=kinds, ro=run_off, rf=first, re_=end, rd=which, cap=need):
        return ctx.lib.ii2_dict_match(ctx.h, k, dicts, n, p(b), p(o), p(kd), p(ro), p(rf), p(re_), p(rd), cap, C.cast(p(stats), C.POINTER(_lib.MatchStats)))

    def untouched():
        return (run_off == FILL64).all() and (first == FILL64).all() and (end == FILL64).all() and (which == FILL32).all() and (stats == FILL64).all()

    slash = np.frombuffer(b"xo0\\\0", np.uint8).copy()
    long_blob = np.frombuffer(b"x" * 65 + b"o0\0", np.uint8).copy()
    with path_delta(ctx) as moved:
        for kw in (dict(dicts=None), dict(b=None), dict(o=None), dict(kd=None), dict(ro=None), dict(rf=None), dict(re_=None), dict(k=0), dict(k=65),
                   dict(dicts=(C.c_void_p * 2)(d.h, None)), dict(dicts=(C.c_void_p * 2)(None, d.h)),
                   dict(o=np.array([1, 1, 2, 4], np.uint64)), dict(o=np.array([0, 2, 1, 4], np.uint64)),
                   dict(kd=np.array([SUFFIX, 3, GLOB], np.uint8)), dict(kd=np.array([SUFFIX, SUFFIX, 0x40 | GLOB], np.uint8)),
                   dict(kd=np.array([SUFFIX, SUFFIX, NOCASE | 3], np.uint8)),
                   dict(b=slash), dict(b=slash, kd=np.array([SUFFIX, SUFFIX, GLOB | NOCASE], np.uint8))):
            assert call(**kw) == -1, kw
            assert untouched(), kw
        assert call(b=long_blob, o=np.array([0, 65, 66, 67], np.uint64)) == -5 and untouched()      # a pattern of 65 bytes
        many = np.zeros(66, np.uint64)
        assert call(n=65, o=many, kd=np.zeros(65, np.uint8), ro=np.full(131, FILL64, np.uint64)) == -5 and untouched()      # 65 patterns
        import torch
        if torch.cuda.device_count() > 1:                              # a dictionary of another device (where there is one)
            from inverted_index_2_amd import Context
            other = Context(1)
            foreign = other.dictionary([b"a"])
            assert call(dicts=(C.c_void_p * 2)(d.h, foreign.h)) == -1 and untouched()
            foreign.free()
            other.close()
        assert call(b=slash, kd=np.array([SUFFIX, SUFFIX, SUFFIX], np.uint8)) == 0      # a trailing backslash is a plain byte of a literal kind
        assert run_off.tolist()[:5] == want[0][:5] and run_off[6] == run_off[4]
        assert call() == 0 and run_off.tolist() == want[0] and first.tolist() == want[1] and end.tolist() == want[2] and which.tolist() == want[3]
    assert moved == {}
    with pytest.raises(II2Error) as e:
        ctx.dict_match([d], [b"a\\"], GLOB)
    assert e.value.code == -1
    with pytest.raises(II2Error) as e:
        d.match([b"a"] * 65, CONTAINS)
    assert e.value.code == -5
    d.free()


def test_no_patterns_and_empty_dictionaries(ctx):
    d, empty = ctx.dictionary([b"a", b"ab", b"b"]), ctx.dictionary([])
    run_off = np.full(3, FILL64, np.uint64)
    rc, st = ctx.dict_match_flat([d, empty], None, None, None, run_off, None, None, None, 0, n_patterns=0)
    assert rc == 0 and run_off.tolist() == [0, FILL64, FILL64] and (st.n_terms, st.n_matched, st.n_runs, st.n_staged, st.n_global) == (0, 0, 0, 0, 0)
    run_off, first, end, which, st = ctx.dict_match([d, empty], [], CONTAINS)
    assert run_off.tolist() == [0] and first.size == 0 and st.n_runs == 0
    run_off, first, end, which, st = ctx.dict_match([empty, empty], [b"", b"*"], np.array([CONTAINS, GLOB], np.uint8))      # no term anywhere
    assert run_off.tolist() == [0] * 5 and first.size == 0 and (st.n_terms, st.n_runs, st.n_staged + st.n_global) == (0, 0, 0)
    run_off, first, end, which, st = ctx.dict_match([empty, d, empty], [b"b", b""], SUFFIX)
    assert run_off.tolist() == [0, 0, 1, 1, 1, 2, 2] and first.tolist() == [1, 0] and end.tolist() == [3, 3] and which.tolist() == [1, 1]
    run_off, first, end, st = d.match([b"a*", b"?", b"c"], GLOB)
    assert run_off.tolist() == [0, 1, 3, 3] and list(zip(first.tolist(), end.tolist())) == [(0, 2), (0, 1), (2, 3)]
    d.free()
    empty.free()


def test_runs_feed_the_range_entry_points_verbatim(ctx):
    """patterns -> ii2_dict_match -> ii2_union_ranges (one pattern = one union) and ii2_intersect_ranges (one pattern = one group,
    beside an exact term from ii2_dict_find), against plain sets"""
    rng = np.random.default_rng(33)
    vocab = [b"%s_%s%d" % (a, b, i) for a in (b"conn", b"db", b"http") for b in (b"timeout", b"error", b"retry", b"ok") for i in range(12)]
    k = 3
    terms_of = [sorted(vocab[int(i)] for i in rng.choice(len(vocab), n, replace=False)) for n in (120, 70, 30)]
    lists_of = [[np.unique(rng.integers(0, 5000, int(rng.integers(1, 300)))).astype(np.uint32) for _ in terms] for terms in terms_of]
    segs = [ctx.encode_lists(lists) for lists in lists_of]
    dicts = [ctx.dictionary(terms) for terms in terms_of]
    patterns, kinds = [b"timeout", b"db_*", b"*_e????[0-9]", b"RETRY1", b"1", b"http_ok?"], [CONTAINS, GLOB, GLOB, CONTAINS | NOCASE, SUFFIX, GLOB]
    run_off, first, end, which, _ = ctx.dict_match(dicts, patterns, np.array(kinds, np.uint8))

    def docs_under(match):
        out = set()
        for s in range(k):
            for t, l in zip(terms_of[s], lists_of[s]):
                if match(t):
                    out |= set(l.tolist())
        return out

    exact = terms_of[0][3]
    e_first, e_end, _ = ctx.dict_find(dicts, [exact])
    under_exact = docs_under(lambda t: t == exact)
    assert under_exact
    some = 0
    for p, (pat, kind) in enumerate(zip(patterns, kinds)):
        a, b = int(run_off[p * k]), int(run_off[(p + 1) * k])
        group = [(segs[int(which[j])], int(first[j]), int(end[j])) for j in range(a, b)]
        want = docs_under(match_cases.matcher(kind, pat))
        group = group or [(segs[0], 0, 0)]                          # (a pattern without a match: one empty range)
        out, n = ctx.union_ranges(group)
        assert out.download(n).tolist() == sorted(want), pat
        out.free()
        beside = [(segs[s], int(e_first[0, s]), int(e_end[0, s])) for s in range(k)]
        out, n = ctx.intersect_ranges([group, beside])
        assert out.download(n).tolist() == sorted(want & under_exact), pat
        out.free()
        some += bool(want)
    assert some >= 5 and not docs_under(match_cases.matcher(GLOB, b"*_e????[0-9]"))      # there are no bracket classes
    for x in segs + dicts:
        x.free()
