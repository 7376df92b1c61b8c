"""GPU: ii2_dict_regex (csrc/dict_regex.hip) - every case of tests/regex_cases.py through the kernel under both settings of
regex.stage, against Python's `re`; a 20 000-byte term at index 255 and at index 256 (staged, not wide); a stage filled to the
byte; the two-call capacity protocol; every argument error with the outputs verified untouched; no patterns and empty
dictionaries; the runs fed verbatim to ii2_union_ranges; a second context.  The kernel-path counters must not move."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from inverted_index_2_amd.engine import II2Error
from tests import regex_cases
from tests.gpu_util import ctx, path_delta  # noqa: F401
from tests.regex_cases import NOCASE, matches

pytestmark = pytest.mark.gpu

FILL64, FILL32 = 0xABABABABABABABAB, 0xCDCDCDCD


@pytest.fixture(scope="module")
def resident(ctx):
    """the dictionaries of every case, made resident once"""
    made = {c.name: [ctx.dictionary(d) for d in c.dicts] for c in regex_cases.CASES}
    yield made
    for dicts in made.values():
        for d in dicts:
            d.free()


def _u8(v):
    return np.array(v, np.uint8)


def _call(ctx, dicts, case):
    return ctx.dict_regex(dicts, case.patterns, _u8(case.flags))


def _check(got, want):
    run_off, first, end, which, st = got
    w_off, w_first, w_end, w_which, w_matched, w_tested = want
    assert run_off.tolist() == w_off
    assert first.tolist() == w_first and end.tolist() == w_end and which.tolist() == w_which
    assert st.n_runs == w_off[-1] and st.n_matched == w_matched and st.n_tested == w_tested


def _stats(st):
    return (st.n_terms, st.n_matched, st.n_runs, st.n_tested, st.n_staged, st.n_global, st.max_positions)


def _positions(case):
    """the largest position count of the case's patterns, from the host-only parse (0: nothing is launched)"""
    from inverted_index_2_amd import term_regex
    if not case.patterns or not any(case.dicts):
        return 0
    return max(term_regex(p, b"")[1] for p in case.patterns)


@pytest.mark.parametrize("stage", (1, 0))
@pytest.mark.parametrize("case", regex_cases.CASES, ids=lambda c: c.name)
def test_table(ctx, resident, case, stage):
    ctx.set_option("regex.stage", stage)
    try:
        with path_delta(ctx) as moved:
            got = _call(ctx, resident[case.name], case)
    finally:
        ctx.set_option("regex.stage", 1)
    _check(got, regex_cases.expected_table(case))
    st = got[4]
    n_wg = sum((len(d) + 255) // 256 for d in case.dicts)
    assert st.n_terms == sum(len(d) for d in case.dicts)
    assert st.n_staged + st.n_global == n_wg and (st.n_staged, st.n_global) == ((n_wg, 0) if stage else (0, n_wg))
    assert st.max_positions == _positions(case)
    known = [regex_cases.N_POS[p] for p in case.patterns if p in regex_cases.N_POS]
    assert not (known and n_wg) or st.max_positions >= max(known)      # (the counts pinned by hand)
    assert moved == {}                                         # not a set operation: no kernel path is counted


def _numbered(n, hit):
    """n sorted terms; term i is five digits and `x` where hit(i) (6 bytes), else five digits and seven `o` (12 bytes)"""
    return [b"%05d" % i + (b"x" if hit(i) else b"ooooooo") for i in range(n)]


PAIR = [b"\\d{5}x", b"[0-9]+o{7}"]                              # the x terms / the o terms


def _runs(want, k, p, s):
    off, first, end = want[0], want[1], want[2]
    return list(zip(first[off[p * k + s]:off[p * k + s + 1]], end[off[p * k + s]:off[p * k + s + 1]]))


def test_a_long_term_astride_a_workgroup_edge(ctx):
    """term 256 (255) of 512 carries 20 000 bytes more: its own workgroup goes to global memory, the one next to it stages its
    terms but not that neighbour (staged, not wide) and matches it from global memory.  Two patterns match the long term (`.*`,
    `\\d.*m`), the others do not: one run ends exactly at it, one starts right behind it."""
    tail = b"m" * 20_000
    ats, hits = (256, 255), (lambda i: i % 10 != 0, lambda i: i % 10 == 0)
    dicts = []
    for at, hit in zip(ats, hits):
        terms = _numbered(512, hit)
        terms[at] += tail
        dicts.append(terms)
    case = regex_cases.Case("long-term-astride", dicts, PAIR + [b".*", b"\\d.*m", b"\\d+[xo]+m{0,60}"], [0] * 5)
    want = regex_cases.expected_table(case)
    for s, at in enumerate(ats):                                # the hits of pattern s surround the long term of dictionary s
        runs = _runs(want, 2, s, s)
        assert any(e == at for _, e in runs) and any(f == at + 1 for f, _ in runs) and not any(f <= at < e for f, e in runs)
        assert _runs(want, 2, 2, s) == [(0, 512)] and _runs(want, 2, 3, s) == [(at, at + 1)] and _runs(want, 2, 4, s) == [(0, at), (at + 1, 512)]
    res = [ctx.dictionary(d) for d in dicts]
    got = _call(ctx, res, case)
    _check(got, want)
    assert got[4].n_staged == 2 and got[4].n_global == 2
    ctx.set_option("regex.stage", 0)
    try:
        _check(_call(ctx, res, case), want)
    finally:
        ctx.set_option("regex.stage", 1)
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
    case = regex_cases.Case("full-stage", dicts, PAIR + [b".*m", b".*"], [0] * 4)
    want = regex_cases.expected_table(case)
    assert (250, 260) in _runs(want, 2, 0, 0) and any(e == 250 for _, e in _runs(want, 2, 1, 0)) and any(f == 260 for f, _ in _runs(want, 2, 1, 0))
    assert any(f == 256 for f, _ in _runs(want, 2, 0, 1)) and any(e == 256 for _, e in _runs(want, 2, 1, 1))      # 255 is an o term, 256 an x term
    res = [ctx.dictionary(d) for d in dicts]
    got = _call(ctx, res, case)
    _check(got, want)
    assert got[4].n_staged == 4 and got[4].n_global == 0
    for d in res:
        d.free()


def _raw_setup(ctx):
    terms = _numbered(600, lambda i: i % 3 == 0)
    d = ctx.dictionary(terms)
    pats = PAIR + [b"0.*"]                                      # the x terms / the o terms / every term
    blob, off = regex_cases.flat(pats)
    blob, off = np.frombuffer(blob, np.uint8).copy(), np.array(off, np.uint64)
    fl = _u8([0, NOCASE, 0])
    case = regex_cases._case("raw", [terms, terms], pats, fl.tolist())
    return d, blob, off, fl, regex_cases.expected_table(case)


def test_capacity_protocol(ctx):
    d, blob, off, fl, want = _raw_setup(ctx)
    w_off, w_first, w_end, w_which, w_matched, w_tested = want
    need = w_off[-1]
    assert need == 2 * (200 + 200 + 1)
    for cap, null_runs in ((need - 1, False), (0, False), (0, True)):
        run_off = np.full(7, FILL64, np.uint64)
        first, end, which = np.full(need + 8, FILL64, np.uint64), np.full(need + 8, FILL64, np.uint64), np.full(need + 8, FILL32, np.uint32)
        args = (None, None, None) if null_runs else (first, end, which)
        rc, st = ctx.dict_regex_flat([d, d], blob, off, fl, run_off, *args, cap)
        assert rc == -4                                                    # II2_ECAPACITY
        assert run_off.tolist() == w_off                                   # run_off and the stats are complete ...
        assert _stats(st) == (1200, w_matched, need, w_tested, 6, 0, 8)
        assert (first == FILL64).all() and (end == FILL64).all() and (which == FILL32).all()      # ... the runs untouched
        rc, st2 = ctx.dict_regex_flat([d, d], blob, off, fl, run_off, first, end, which, int(run_off[-1]))      # the second call is exact
        assert rc == 0 and first[:need].tolist() == w_first and end[:need].tolist() == w_end and which[:need].tolist() == w_which
        assert (first[need:] == FILL64).all() and (end[need:] == FILL64).all() and (which[need:] == FILL32).all()
        assert _stats(st2) == _stats(st)
    # run_dict and pat_flags may be NULL
    first, end = np.full(need, FILL64, np.uint64), np.full(need, FILL64, np.uint64)
    rc, _ = ctx.dict_regex_flat([d, d], blob, off, fl, run_off, first, end, None, need)
    assert rc == 0 and first.tolist() == w_first and end.tolist() == w_end
    rc, st = ctx.dict_regex_flat([d], blob, off, None, run_off, first, end, None, need)
    assert rc == 0 and run_off.tolist()[:4] == [0, 200, 400, 401] and first[:400].tolist() == w_first[:200] + w_first[400:600] and end[400] == 600
    # the wrapper makes the second call itself
    small = ctx.dictionary(_numbered(20_000, lambda i: i % 2 == 0))
    run_off, first, end, st = small.regex([b"\\d{5}x"])
    assert run_off.tolist() == [0, 10_000] and first.tolist() == list(range(0, 20_000, 2)) and (end - first == 1).all() and st.n_runs == 10_000
    small.free()
    d.free()


def test_argument_errors_leave_the_outputs_untouched(ctx):
    d, blob, off, fl, want = _raw_setup(ctx)
    need = want[0][-1]
    run_off = np.full(7, FILL64, np.uint64)
    first, end, which = np.full(need, FILL64, np.uint64), np.full(need, FILL64, np.uint64), np.full(need, FILL32, np.uint32)
    stats = np.full(6, FILL64, np.uint64)
    arr = (C.c_void_p * 2)(d.h, d.h)
    p = lambda a: a.ctypes.data if a is not None else None

    def call(k=2, dicts=arr, n=3, b=blob, o=off, f=fl, ro=run_off, rf=first, re_=end, rd=which, cap=need):
        return ctx.lib.ii2_dict_regex(ctx.h, k, dicts, n, p(b), p(o), p(f), p(ro), p(rf), p(re_), p(rd), cap, C.cast(p(stats), C.POINTER(_lib.RegexStats)))

    def untouched():
        return (run_off == FILL64).all() and (first == FILL64).all() and (end == FILL64).all() and (which == FILL32).all() and (stats == FILL64).all()

    def three(pattern):
        """the call's arrays with `pattern` in the middle"""
        b, o = regex_cases.flat([b"a", pattern, b"b"])
        return dict(b=np.frombuffer(b, np.uint8).copy(), o=np.array(o, np.uint64))

    with path_delta(ctx) as moved:
        for kw in (dict(dicts=None), dict(b=None), dict(o=None), dict(ro=None), dict(rf=None), dict(re_=None), dict(k=0), dict(k=65),
                   dict(dicts=(C.c_void_p * 2)(d.h, None)), dict(dicts=(C.c_void_p * 2)(None, d.h)),
                   dict(o=np.array([1, 1, 2, 4], np.uint64)), dict(o=np.array([0, 7, 6, 13], np.uint64)),
                   dict(f=_u8([0, 1, 0])), dict(f=_u8([0, 0, 0x40])), dict(f=_u8([NOCASE | 4, 0, 0]))):
            assert call(**kw) == -1, kw
            assert untouched(), kw
        for bad in regex_cases.INVALID:                                # a pattern that does not parse
            assert call(**three(bad)) == -1, bad
            assert untouched(), bad
        for bad, _ in regex_cases.TOO_MANY_POSITIONS:                  # the three limits
            assert call(**three(bad)) == -5 and untouched(), bad
        assert call(**three(regex_cases.TOO_LONG)) == -5 and untouched()
        assert call(n=9, o=np.zeros(10, np.uint64), f=None, ro=np.full(19, FILL64, np.uint64)) == -5 and untouched()      # 9 patterns
        import torch
        if torch.cuda.device_count() > 1:                              # a dictionary of another device (where there is one)
            from inverted_index_2_amd import Context
            other = Context(1)
            foreign = other.dictionary([b"a"])
            assert call(dicts=(C.c_void_p * 2)(d.h, foreign.h)) == -1 and untouched()
            foreign.free()
            other.close()
        assert call() == 0 and run_off.tolist() == want[0] and first.tolist() == want[1] and end.tolist() == want[2] and which.tolist() == want[3]
        # the neighbours at the limits: 8 patterns, 256 bytes, 64 positions
        assert call(n=8, o=np.zeros(9, np.uint64), f=None, ro=np.zeros(17, np.uint64), cap=0, rf=None, re_=None) == 0
        for ok in regex_cases.AT_THE_POSITION_LIMIT + [regex_cases.AT_THE_LENGTH_LIMIT]:
            assert call(**three(ok), cap=0, rf=None, re_=None) in (0, -4), ok
    assert moved == {}
    with pytest.raises(II2Error) as e:
        ctx.dict_regex([d], [b"a("])
    assert e.value.code == -1
    with pytest.raises(II2Error) as e:
        d.regex([b"a"] * 9)
    assert e.value.code == -5
    with pytest.raises(ValueError):
        ctx.dict_regex([d], [b"a", b"b"], [0])
    d.free()


def test_no_patterns_and_empty_dictionaries(ctx):
    d, empty = ctx.dictionary([b"a", b"ab", b"b"]), ctx.dictionary([])
    run_off = np.full(3, FILL64, np.uint64)
    rc, st = ctx.dict_regex_flat([d, empty], None, None, None, run_off, None, None, None, 0, n_patterns=0)
    assert rc == 0 and run_off.tolist() == [0, FILL64, FILL64] and _stats(st) == (0, 0, 0, 0, 0, 0, 0)
    run_off, first, end, which, st = ctx.dict_regex([d, empty], [])
    assert run_off.tolist() == [0] and first.size == 0 and st.n_runs == 0 and st.max_positions == 0
    run_off, first, end, which, st = ctx.dict_regex([empty, empty], [b"", b"a"])      # no term anywhere
    assert run_off.tolist() == [0] * 5 and first.size == 0 and _stats(st) == (0, 0, 0, 0, 0, 0, 0)
    run_off, first, end, which, st = ctx.dict_regex([empty, d, empty], [b"a?b", b".*"])
    assert list(zip(first.tolist(), end.tolist(), which.tolist())) == [(1, 3, 1), (0, 3, 1)] and run_off.tolist() == [0, 0, 1, 1, 1, 2, 2]
    run_off, first, end, st = d.regex([b"ab", b"[ab]", b"c", b"a.*"])
    assert run_off.tolist() == [0, 1, 3, 3, 4] and list(zip(first.tolist(), end.tolist())) == [(1, 2), (0, 1), (2, 3), (0, 2)]
    assert st.max_positions == 2 and st.n_matched == 1 + 2 + 0 + 2 and st.n_tested == 1 + 2 + 2 + 3
    d.free()
    empty.free()


def test_runs_feed_the_range_entry_points_verbatim(ctx):
    """patterns -> ii2_dict_regex -> ii2_union_ranges (one pattern = one union) equals the union computed in numpy"""
    rng = np.random.default_rng(43)
    stems = [b"timeout", b"timeouts", b"timed", b"retry", b"retries", b"error", b"errors", b"terror", b"ok", b"fail404", b"fail500", b"error503", b"req-17-a", b"req-x"]
    vocab = sorted({a + b"_" + s for a in (b"conn", b"db") for s in stems} | set(stems))
    k = 3
    terms_of = [sorted(vocab[int(i)] for i in rng.choice(len(vocab), n, replace=False)) for n in (len(vocab), 25, 12)]
    lists_of = [[np.unique(rng.integers(0, 3000, int(rng.integers(1, 200)))).astype(np.uint32) for _ in terms] for terms in terms_of]
    segs = [ctx.encode_lists(lists) for lists in lists_of]
    dicts = [ctx.dictionary(terms) for terms in terms_of]
    patterns = [b".*time.*", b"(conn|db)_.*", b"(.*_)?(error|fail)[0-9]{3}", b"RE(TRY|TRIES)", b"z+", b"req-[0-9]+-.*", b".*s"]
    fl = [0, 0, 0, NOCASE, 0, 0, 0]
    run_off, first, end, which, _ = ctx.dict_regex(dicts, patterns, _u8(fl))
    some = 0
    for p, pat in enumerate(patterns):
        a, b = int(run_off[p * k]), int(run_off[(p + 1) * k])
        group = [(segs[int(which[j])], int(first[j]), int(end[j])) for j in range(a, b)] or [(segs[0], 0, 0)]      # (no match: one empty range)
        hit = [l for s in range(k) for t, l in zip(terms_of[s], lists_of[s]) if matches(pat, t, fl[p])]
        want = np.unique(np.concatenate(hit)) if hit else np.zeros(0, np.uint32)
        out, n = ctx.union_ranges(group)
        assert out.download(n).tolist() == want.tolist(), pat
        out.free()
        some += bool(hit)
    assert some == 6
    for x in segs + dicts:
        x.free()


def test_a_second_context_gives_the_same(ctx):
    from inverted_index_2_amd import Context
    case = next(c for c in regex_cases.CASES if c.name == "k3-unequal")
    other = Context(0)
    try:
        dicts = [other.dictionary(d) for d in case.dicts]
        _check(other.dict_regex(dicts, case.patterns, _u8(case.flags)), regex_cases.expected_table(case))
        for d in dicts:
            d.free()
    finally:
        other.close()
