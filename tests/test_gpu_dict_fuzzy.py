"""GPU: ii2_dict_fuzzy (csrc/dict_fuzzy.hip) - every case of tests/fuzzy_cases.py through the kernels under the four settings of
fuzzy.stage x fuzzy.wide; runs at the workgroup boundary of 256 terms; one very long term that sends its workgroup alone to
global memory; workgroups that stage their own terms but not a neighbour across their edge; the two-call capacity protocol;
every argument error with the outputs verified untouched; no patterns and empty dictionaries; and the runs fed verbatim to
ii2_union_ranges and, as nested distance tiers, to ii2_topk_weighted_ranges.  The kernel-path counters must not move."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from inverted_index_2_amd.engine import II2Error
from tests import fuzzy_cases
from tests.fuzzy_cases import NOCASE, TRANSPOSE, matches
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu

FILL64, FILL32 = 0xABABABABABABABAB, 0xCDCDCDCD


@pytest.fixture(scope="module")
def resident(ctx):
    """the dictionaries of every case, made resident once"""
    made = {c.name: [ctx.dictionary(d) for d in c.dicts] for c in fuzzy_cases.CASES}
    yield made
    for dicts in made.values():
        for d in dicts:
            d.free()


def _u8(v):
    return np.array(v, np.uint8)


def _call(ctx, dicts, case):
    return ctx.dict_fuzzy(dicts, case.patterns, _u8(case.dists), _u8(case.prefixes), _u8(case.flags))


def _check(got, want):
    run_off, first, end, which, st = got
    w_off, w_first, w_end, w_which, w_matched, w_tested = want
    assert run_off.tolist() == w_off
    assert first.tolist() == w_first and end.tolist() == w_end and which.tolist() == w_which
    assert st.n_runs == w_off[-1] and st.n_matched == w_matched and st.n_tested == w_tested


@pytest.mark.parametrize("wide", (0, 1))
@pytest.mark.parametrize("stage", (1, 0))
@pytest.mark.parametrize("case", fuzzy_cases.CASES, ids=lambda c: c.name)
def test_table(ctx, resident, case, stage, wide):
    ctx.set_option("fuzzy.stage", stage)
    ctx.set_option("fuzzy.wide", wide)
    try:
        with path_delta(ctx) as moved:
            got = _call(ctx, resident[case.name], case)
    finally:
        ctx.set_option("fuzzy.stage", 1)
        ctx.set_option("fuzzy.wide", 0)
    _check(got, fuzzy_cases.expected_table(case))
    st = got[4]
    n_wg = sum((len(d) + 255) // 256 for d in case.dicts)
    assert st.n_terms == sum(len(d) for d in case.dicts)
    assert st.n_staged + st.n_global == n_wg and (st.n_staged, st.n_global) == ((n_wg, 0) if stage else (0, n_wg))
    bits = fuzzy_cases.word_bits(case)
    assert st.word_bits == (64 if wide and bits else bits)
    assert moved == {}                                         # not a set operation: no kernel path is counted


def test_one_very_long_term_takes_the_global_path_alone(ctx):
    long_term = b"m" * 39_990 + b"needle" + b"mmmm"                     # 40 000 bytes: no stage holds its workgroup
    terms = sorted([b"%06d" % i + (b"needle" if i % 7 == 0 else b"") for i in range(1500)] + [long_term, b"needle", b"needlf", b"mneedle"])
    d = ctx.dictionary(terms)
    case = fuzzy_cases._case("long-term", [terms], [b"needle", b"NEEDEL", b"000007needle", b"000003", b"m" * 64], [1, 2, 2, 1, 255], [0, 1, 6, 5, 1],
                             [0, NOCASE | TRANSPOSE, 0, TRANSPOSE, 0])
    got = _call(ctx, [d], case)
    _check(got, fuzzy_cases.expected_table(case))
    st = got[4]
    assert st.n_global == 1 and st.n_staged == (len(terms) + 255) // 256 - 1 and st.n_staged > 0 and st.word_bits == 64
    assert st.n_matched >= 10 and got[0][-1] >= 5            # (the inputs are not trivial)
    d.free()


def _numbered(n, hit):
    """n sorted terms; term i is five digits and `x` where hit(i) (6 bytes), else five digits and seven `o` (12 bytes)"""
    return [b"%05d" % i + (b"x" if hit(i) else b"ooooooo") for i in range(n)]


@pytest.mark.parametrize("stage", (1, 0))
@pytest.mark.parametrize("n", (255, 256, 257, 512))
def test_workgroup_boundaries(ctx, n, stage):
    """every term matches, none, and alternate terms (both phases): runs across the boundary, at both ends, the most runs.  Five
    edits cover the digits, not the six bytes between the two lengths: pattern 0 takes the x terms, pattern 1 the o terms"""
    shapes = {"all": lambda i: True, "none": lambda i: False, "even": lambda i: i % 2 == 0, "odd": lambda i: i % 2 == 1,
              "but-the-boundary": lambda i: i not in (255, 256), "only-the-boundary": lambda i: i in (255, 256),
              "last-of-each": lambda i: i % 256 == 255, "first-of-each": lambda i: i % 256 == 0}
    names = list(shapes)
    dicts = [_numbered(n, shapes[name]) for name in names]
    res = [ctx.dictionary(d) for d in dicts]
    case = fuzzy_cases.Case(f"boundary-{n}", dicts, [b"00000x", b"00000ooooooo"], [5, 5], [0, 2], [0, 0])
    ctx.set_option("fuzzy.stage", stage)
    try:
        got = _call(ctx, res, case)
    finally:
        ctx.set_option("fuzzy.stage", 1)
    _check(got, fuzzy_cases.expected_table(case))
    run_off = got[0]
    k = len(names)
    per = lambda p, name: int(run_off[p * k + names.index(name) + 1] - run_off[p * k + names.index(name)])
    assert per(0, "all") == 1 and per(0, "none") == 0 and per(0, "even") == (n + 1) // 2 and per(0, "odd") == n // 2
    assert per(1, "all") == 0 and per(1, "none") == 1 and per(1, "even") == n // 2
    for d in res:
        d.free()


def _runs(want, k, p, s):
    off, first, end = want[0], want[1], want[2]
    return list(zip(first[off[p * k + s]:off[p * k + s + 1]], end[off[p * k + s]:off[p * k + s + 1]]))


def test_a_long_term_astride_a_workgroup_edge(ctx):
    """term 256 (255) of 512 carries 20 000 bytes more: its own workgroup goes to global memory, the one next to it stages its
    terms but not that neighbour (staged, not wide) and matches it from global memory.  No pattern of at most 64 bytes lies
    within 255 edits of such a term, so here it only ever breaks a run: one ends exactly at it, one starts right behind it."""
    tail = b"m" * 20_000
    ats, hits = (256, 255), (lambda i: i % 10 != 0, lambda i: i % 10 == 0)
    dicts = []
    for at, hit in zip(ats, hits):
        terms = _numbered(512, hit)
        terms[at] += tail
        dicts.append(terms)
    case = fuzzy_cases.Case("long-term-astride", dicts, [b"00000x", b"00000ooooooo"], [5, 5], [0, 2], [0, 0])
    want = fuzzy_cases.expected_table(case)
    for s, at in enumerate(ats):                                # the hits of pattern s surround the long term of dictionary s
        runs = _runs(want, 2, s, s)
        assert any(e == at for _, e in runs) and any(f == at + 1 for f, _ in runs) and not any(f <= at < e for f, e in runs)
    res = [ctx.dictionary(d) for d in dicts]
    for wide in (0, 1):
        ctx.set_option("fuzzy.wide", wide)
        try:
            got = _call(ctx, res, case)
        finally:
            ctx.set_option("fuzzy.wide", 0)
        _check(got, want)
        st = got[4]
        assert st.n_staged == 2 and st.n_global == 2 and st.word_bits == (64 if wide else 32)
    for d in res:
        d.free()


def test_neighbours_that_match_outside_a_full_stage(ctx):
    """staged, not wide, with neighbours a pattern can match: one term in the middle of each workgroup is padded until the
    workgroup's own 256 terms fill the 16 KB stage to the byte, so the 6- or 12-byte neighbour across the edge no longer fits and
    is matched from global memory.  One dictionary has a run across the edge, one a run that ends at it and one that starts there."""
    dicts = []
    for hit in (lambda i: 250 <= i < 260, lambda i: i % 3 != 0):
        terms = _numbered(512, hit)
        for mid, w0 in ((100, 0), (400, 256)):
            terms[mid] += b"m" * (16384 - sum(len(t) for t in terms[w0:w0 + 256]))
        assert [sum(len(t) for t in terms[w0:w0 + 256]) for w0 in (0, 256)] == [16384, 16384]
        dicts.append(terms)
    case = fuzzy_cases.Case("full-stage", dicts, [b"00000x", b"00000ooooooo"], [5, 5], [0, 2], [0, 0])
    want = fuzzy_cases.expected_table(case)
    assert (250, 260) in _runs(want, 2, 0, 0) and any(e == 250 for _, e in _runs(want, 2, 1, 0)) and any(f == 260 for f, _ in _runs(want, 2, 1, 0))
    assert any(f == 256 for f, _ in _runs(want, 2, 0, 1)) and any(e == 256 for _, e in _runs(want, 2, 1, 1))      # 255 is an o term, 256 an x term
    res = [ctx.dictionary(d) for d in dicts]
    for wide in (0, 1):
        ctx.set_option("fuzzy.wide", wide)
        try:
            got = _call(ctx, res, case)
        finally:
            ctx.set_option("fuzzy.wide", 0)
        _check(got, want)
        assert got[4].n_staged == 4 and got[4].n_global == 0
    for d in res:
        d.free()


def _raw_setup(ctx):
    terms = _numbered(600, lambda i: i % 3 == 0)
    d = ctx.dictionary(terms)
    pats = [b"00000x", b"00000ooooooo", b"0"]
    blob, off = fuzzy_cases.flat(pats)
    blob, off = np.frombuffer(blob, np.uint8).copy(), np.array(off, np.uint64)
    # five edits cover the digits, not the six bytes between the two lengths: the x terms / the o terms / every term
    dist, pre, fl = _u8([5, 5, 255]), _u8([0, 2, 1]), _u8([0, TRANSPOSE, 0])
    case = fuzzy_cases._case("raw", [terms, terms], pats, dist.tolist(), pre.tolist(), fl.tolist())
    return d, blob, off, dist, pre, fl, fuzzy_cases.expected_table(case)


def _stats(st):
    return (st.n_terms, st.n_matched, st.n_runs, st.n_tested, st.n_staged, st.n_global, st.word_bits)


def test_capacity_protocol(ctx):
    d, blob, off, dist, pre, fl, want = _raw_setup(ctx)
    w_off, w_first, w_end, w_which, w_matched, w_tested = want
    need = w_off[-1]
    assert need == 2 * (200 + 200 + 1)
    for cap, null_runs in ((need - 1, False), (0, False), (0, True)):
        run_off = np.full(7, FILL64, np.uint64)
        first, end, which = np.full(need + 8, FILL64, np.uint64), np.full(need + 8, FILL64, np.uint64), np.full(need + 8, FILL32, np.uint32)
        args = (None, None, None) if null_runs else (first, end, which)
        rc, st = ctx.dict_fuzzy_flat([d, d], blob, off, dist, pre, fl, run_off, *args, cap)
        assert rc == -4                                                    # II2_ECAPACITY
        assert run_off.tolist() == w_off                                   # run_off and the stats are complete ...
        assert _stats(st) == (1200, w_matched, need, w_tested, 6, 0, 32)
        assert (first == FILL64).all() and (end == FILL64).all() and (which == FILL32).all()      # ... the runs untouched
        rc, st2 = ctx.dict_fuzzy_flat([d, d], blob, off, dist, pre, fl, run_off, first, end, which, int(run_off[-1]))      # the second call is exact
        assert rc == 0 and first[:need].tolist() == w_first and end[:need].tolist() == w_end and which[:need].tolist() == w_which
        assert (first[need:] == FILL64).all() and (end[need:] == FILL64).all() and (which[need:] == FILL32).all()
        assert _stats(st2) == _stats(st)
    # run_dict, pat_prefix and pat_flags may be NULL
    first, end = np.full(need, FILL64, np.uint64), np.full(need, FILL64, np.uint64)
    rc, _ = ctx.dict_fuzzy_flat([d, d], blob, off, dist, pre, fl, run_off, first, end, None, need)
    assert rc == 0 and first.tolist() == w_first and end.tolist() == w_end
    rc, st = ctx.dict_fuzzy_flat([d], blob, off, dist, None, None, run_off, first, end, None, need)
    assert rc == 0 and run_off.tolist()[:4] == [0, 200, 400, 401] and first[:400].tolist() == w_first[:200] + w_first[400:600] and end[400] == 600
    # the wrapper makes the second call itself
    small = ctx.dictionary(_numbered(20_000, lambda i: i % 2 == 0))
    run_off, first, end, st = small.fuzzy([b"00000x"], 5)
    assert run_off.tolist() == [0, 10_000] and first.tolist() == list(range(0, 20_000, 2)) and (end - first == 1).all() and st.n_runs == 10_000
    small.free()
    d.free()


def test_argument_errors_leave_the_outputs_untouched(ctx):
    d, blob, off, dist, pre, fl, want = _raw_setup(ctx)
    need = want[0][-1]
    run_off = np.full(7, FILL64, np.uint64)
    first, end, which = np.full(need, FILL64, np.uint64), np.full(need, FILL64, np.uint64), np.full(need, FILL32, np.uint32)
    stats = np.full(6, FILL64, np.uint64)
    arr = (C.c_void_p * 2)(d.h, d.h)
    p = lambda a: a.ctypes.data if a is not None else None

    def call(k=2, dicts=arr, n=3, b=blob, o=off, ds=dist, pr=pre, f=fl, ro=run_off, rf=first, re_=end, rd=which, cap=need):
        return ctx.lib.ii2_dict_fuzzy(ctx.h, k, dicts, n, p(b), p(o), p(ds), p(pr), p(f), p(ro), p(rf), p(re_), p(rd), cap,
                                      C.cast(p(stats), C.POINTER(_lib.FuzzyStats)))

    def untouched():
        return (run_off == FILL64).all() and (first == FILL64).all() and (end == FILL64).all() and (which == FILL32).all() and (stats == FILL64).all()

    long_blob = np.frombuffer(b"x" * 65 + b"o0\0", np.uint8).copy()
    with path_delta(ctx) as moved:
        for kw in (dict(dicts=None), dict(b=None), dict(o=None), dict(ds=None), dict(ro=None), dict(rf=None), dict(re_=None), dict(k=0), dict(k=65),
                   dict(dicts=(C.c_void_p * 2)(d.h, None)), dict(dicts=(C.c_void_p * 2)(None, d.h)),
                   dict(o=np.array([1, 1, 2, 4], np.uint64)), dict(o=np.array([0, 7, 6, 13], np.uint64)),
                   dict(f=_u8([0, 2, 0])), dict(f=_u8([0, 0, 0x40])), dict(f=_u8([NOCASE | TRANSPOSE | 4, 0, 0])),
                   dict(pr=_u8([7, 6, 1])), dict(pr=_u8([6, 6, 2])), dict(pr=_u8([0, 0, 255]))):
            assert call(**kw) == -1, kw
            assert untouched(), kw
        assert call(b=long_blob, o=np.array([0, 65, 66, 67], np.uint64), pr=None) == -5 and untouched()      # a pattern of 65 bytes
        many = np.zeros(18, np.uint64)
        assert call(n=17, o=many, ds=np.zeros(17, np.uint8), pr=None, f=None, ro=np.full(35, FILL64, np.uint64)) == -5 and untouched()      # 17 patterns
        import torch
        if torch.cuda.device_count() > 1:                              # a dictionary of another device (where there is one)
            from inverted_index_2_amd import Context
            other = Context(1)
            foreign = other.dictionary([b"a"])
            assert call(dicts=(C.c_void_p * 2)(d.h, foreign.h)) == -1 and untouched()
            foreign.free()
            other.close()
        assert call() == 0 and run_off.tolist() == want[0] and first.tolist() == want[1] and end.tolist() == want[2] and which.tolist() == want[3]
        assert call(n=16, o=np.zeros(17, np.uint64), ds=np.zeros(16, np.uint8), pr=None, f=None, ro=np.zeros(33, np.uint64), cap=0, rf=None, re_=None) == 0
    assert moved == {}
    with pytest.raises(II2Error) as e:
        ctx.dict_fuzzy([d], [b"ab"], 1, prefix=3)
    assert e.value.code == -1
    with pytest.raises(II2Error) as e:
        d.fuzzy([b"a"] * 17, 1)
    assert e.value.code == -5
    with pytest.raises(ValueError):
        ctx.dict_fuzzy([d], [b"a", b"b"], [1])
    d.free()


def test_no_patterns_and_empty_dictionaries(ctx):
    d, empty = ctx.dictionary([b"a", b"ab", b"b"]), ctx.dictionary([])
    run_off = np.full(3, FILL64, np.uint64)
    rc, st = ctx.dict_fuzzy_flat([d, empty], None, None, None, None, None, run_off, None, None, None, 0, n_patterns=0)
    assert rc == 0 and run_off.tolist() == [0, FILL64, FILL64] and _stats(st) == (0, 0, 0, 0, 0, 0, 0)
    run_off, first, end, which, st = ctx.dict_fuzzy([d, empty], [], 1)
    assert run_off.tolist() == [0] and first.size == 0 and st.n_runs == 0 and st.word_bits == 0
    run_off, first, end, which, st = ctx.dict_fuzzy([empty, empty], [b"", b"a"], [0, 1])      # no term anywhere
    assert run_off.tolist() == [0] * 5 and first.size == 0 and _stats(st) == (0, 0, 0, 0, 0, 0, 0)
    run_off, first, end, which, st = ctx.dict_fuzzy([empty, d, empty], [b"b", b""], [1, 1])
    assert run_off.tolist() == [0, 0, 1, 1, 1, 3, 3] and first.tolist() == [0, 0, 2] and end.tolist() == [3, 1, 3] and which.tolist() == [1, 1, 1]
    run_off, first, end, st = d.fuzzy([b"ab", b"ba", b"c", b"xyz"], [0, 1, 1, 2], flags=[0, TRANSPOSE, 0, 0])
    assert run_off.tolist() == [0, 1, 2, 4, 4] and list(zip(first.tolist(), end.tolist())) == [(1, 2), (0, 3), (0, 1), (2, 3)]
    assert st.word_bits == 32 and st.n_matched == 1 + 3 + 2 and st.n_tested == 1 + 3 + 3 + 3
    d.free()
    empty.free()


def test_runs_feed_the_range_entry_points_verbatim(ctx):
    """patterns -> ii2_dict_fuzzy -> ii2_union_ranges (one pattern = one union), and the nested groups of one pattern at distances
    0, 1 and 2 -> ii2_topk_weighted_ranges: their weights add up, so a doc under the exact term ranks above one under a term two
    edits away"""
    rng = np.random.default_rng(41)
    stems = [b"timeout", b"timeuot", b"timeouts", b"tmeout", b"timed", b"retry", b"retyr", b"retries", b"error", b"eror", b"errors", b"terror", b"ok"]
    vocab = sorted({a + b"_" + s for a in (b"conn", b"db") for s in stems} | set(stems))
    k = 3
    terms_of = [sorted(vocab[int(i)] for i in rng.choice(len(vocab), n, replace=False)) for n in (len(vocab), 25, 12)]
    lists_of = [[np.unique(rng.integers(0, 3000, int(rng.integers(1, 200)))).astype(np.uint32) for _ in terms] for terms in terms_of]
    segs = [ctx.encode_lists(lists) for lists in lists_of]
    dicts = [ctx.dictionary(terms) for terms in terms_of]
    patterns, dist, pre, fl = [b"timeout", b"TIMEOUT", b"retry", b"db_error", b"zzzzzzzzzzzz", b"error"], [1, 2, 1, 2, 2, 1], [0, 1, 3, 3, 0, 0], \
        [0, NOCASE, TRANSPOSE, 0, 0, TRANSPOSE]
    run_off, first, end, which, _ = ctx.dict_fuzzy(dicts, patterns, _u8(dist), _u8(pre), _u8(fl))

    def docs_under(match):
        out = set()
        for s in range(k):
            for t, l in zip(terms_of[s], lists_of[s]):
                if match(t):
                    out |= set(l.tolist())
        return out

    some = 0
    for p, pat in enumerate(patterns):
        a, b = int(run_off[p * k]), int(run_off[(p + 1) * k])
        group = [(segs[int(which[j])], int(first[j]), int(end[j])) for j in range(a, b)] or [(segs[0], 0, 0)]      # (no match: one empty range)
        want = docs_under(lambda t: matches(pat, t, dist[p], pre[p], fl[p]))
        out, n = ctx.union_ranges(group)
        assert out.download(n).tolist() == sorted(want), pat
        out.free()
        some += bool(want)
    assert some == 5 and not docs_under(lambda t: matches(b"zzzzzzzzzzzz", t, 2, 0, 0))
    # tiers: the same pattern at distances 0, 1, 2 - three nested groups with weights 4, 2, 1
    run_off, first, end, which, _ = ctx.dict_fuzzy(dicts, [b"timeout"] * 3, _u8([0, 1, 2]))
    groups = [[(segs[int(which[j])], int(first[j]), int(end[j])) for j in range(int(run_off[p * k]), int(run_off[(p + 1) * k]))] for p in range(3)]
    tier = [docs_under(lambda t, d=d: fuzzy_cases.distance(b"timeout", t, 0) <= d) for d in (0, 1, 2)]
    assert tier[0] and tier[0] < tier[1] < tier[2]
    ids, scores, n = ctx.topk_weighted_ranges(groups, [4, 2, 1], len(tier[2]) + 5)
    got_ids, got_scores = ids.download(n).tolist(), scores.download(n).tolist()
    want_score = {doc: 1 + 2 * (doc in tier[1]) + 4 * (doc in tier[0]) for doc in tier[2]}
    assert dict(zip(got_ids, got_scores)) == want_score and got_scores == sorted(got_scores, reverse=True)
    exact_doc, far_doc = min(tier[0]), min(tier[2] - tier[1])
    assert got_ids.index(exact_doc) < got_ids.index(far_doc) and want_score[exact_doc] == 7 and want_score[far_doc] == 1
    ids.free()
    scores.free()
    for x in segs + dicts:
        x.free()
