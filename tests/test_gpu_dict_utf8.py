"""GPU: II2_MATCH_UTF8 through the kernels - every case of tests/utf8_cases.py through ii2_dict_fuzzy under the four settings of
fuzzy.stage x fuzzy.wide and through ii2_dict_match under match.stage, with the instance (word_bits), n_utf8, n_tested and the
staged / global split pinned; the ASCII cases of tests/fuzzy_cases.py and tests/match_cases.py with the flag OR-ed in against
their own expectation; a term of three-byte symbols longer than the stage; an unflagged call; every argument error with the
outputs verified untouched; the two-call capacity protocol; and the runs fed verbatim to ii2_union_ranges.  The kernel-path
counters must not move."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import fuzzy_cases, match_cases, utf8_cases
from tests.gpu_util import ctx, path_delta  # noqa: F401
from tests.utf8_cases import GLOB, NOCASE, TRANSPOSE, UTF8, u

pytestmark = pytest.mark.gpu

FILL64, FILL32 = 0xABABABABABABABAB, 0xCDCDCDCD
ASCII_FUZZY, ASCII_MATCH = utf8_cases.ascii_fuzzy_cases(), utf8_cases.ascii_match_cases()


@pytest.fixture(scope="module")
def resident(ctx):
    """the dictionaries of every case, made resident once (a flagged ASCII case shares its plain case's)"""
    made = {}
    for c in utf8_cases.FUZZY_CASES + [plain for plain, _ in ASCII_FUZZY]:
        made["fuzzy:" + c.name] = [ctx.dictionary(d) for d in c.dicts]
    for c in utf8_cases.MATCH_CASES + [plain for plain, _ in ASCII_MATCH]:
        made["match:" + c.name] = [ctx.dictionary(d) for d in c.dicts]
    yield made
    for dicts in made.values():
        for d in dicts:
            d.free()


def _u8(v):
    return np.array(v, np.uint8)


def _fuzzy(ctx, dicts, case):
    return ctx.dict_fuzzy(dicts, case.patterns, _u8(case.dists), _u8(case.prefixes), _u8(case.flags))


def _check_fuzzy(got, want):
    run_off, first, end, which, st = got
    w_off, w_first, w_end, w_which, w_matched, w_tested = want
    assert run_off.tolist() == w_off
    assert first.tolist() == w_first and end.tolist() == w_end and which.tolist() == w_which
    assert st.n_runs == w_off[-1] and st.n_matched == w_matched and st.n_tested == w_tested


def _check_match(got, want):
    run_off, first, end, which, st = got
    w_off, w_first, w_end, w_which, w_matched = want
    assert run_off.tolist() == w_off
    assert first.tolist() == w_first and end.tolist() == w_end and which.tolist() == w_which
    assert st.n_runs == w_off[-1] and st.n_matched == w_matched


def _split(case, st, stage):
    n_wg = sum((len(d) + 255) // 256 for d in case.dicts)
    assert st.n_terms == sum(len(d) for d in case.dicts)
    assert (st.n_staged, st.n_global) == ((n_wg, 0) if stage else (0, n_wg))


@pytest.mark.parametrize("wide", (0, 1))
@pytest.mark.parametrize("stage", (1, 0))
@pytest.mark.parametrize("case", utf8_cases.FUZZY_CASES, ids=lambda c: c.name)
def test_fuzzy_table(ctx, resident, case, stage, wide):
    ctx.set_option("fuzzy.stage", stage)
    ctx.set_option("fuzzy.wide", wide)
    try:
        with path_delta(ctx) as moved:
            got = _fuzzy(ctx, resident["fuzzy:" + case.name], case)
    finally:
        ctx.set_option("fuzzy.stage", 1)
        ctx.set_option("fuzzy.wide", 0)
    _check_fuzzy(got, utf8_cases.expected_fuzzy(case))
    st = got[4]
    _split(case, st, stage)
    bits = utf8_cases.word_bits(case)
    assert st.word_bits == (64 if wide and bits else bits) and st.n_utf8 == utf8_cases.n_utf8(case) and st.n_utf8 > 0
    assert moved == {}                                         # not a set operation: no kernel path is counted


@pytest.mark.parametrize("pair", ASCII_FUZZY, ids=lambda p: p[0].name)
def test_ascii_fuzzy_cases_answer_as_without_the_flag(ctx, resident, pair):
    plain, flagged = pair
    got = _fuzzy(ctx, resident["fuzzy:" + plain.name], flagged)
    _check_fuzzy(got, fuzzy_cases.expected_table(plain))       # the case's own expectation, n_tested included
    bits = fuzzy_cases.word_bits(plain)
    assert got[4].word_bits == bits and got[4].n_utf8 == (len(plain.patterns) if bits else 0)


@pytest.mark.parametrize("stage", (1, 0))
@pytest.mark.parametrize("case", utf8_cases.MATCH_CASES, ids=lambda c: c.name)
def test_match_table(ctx, resident, case, stage):
    ctx.set_option("match.stage", stage)
    try:
        with path_delta(ctx) as moved:
            got = ctx.dict_match(resident["match:" + case.name], case.patterns, _u8(case.kinds))
    finally:
        ctx.set_option("match.stage", 1)
    _check_match(got, utf8_cases.expected_match(case))
    _split(case, got[4], stage)
    assert moved == {}


@pytest.mark.parametrize("pair", ASCII_MATCH, ids=lambda p: p[0].name)
def test_ascii_match_cases_answer_as_without_the_flag(ctx, resident, pair):
    plain, flagged = pair
    got = ctx.dict_match(resident["match:" + plain.name], flagged.patterns, _u8(flagged.kinds))
    _check_match(got, match_cases.expected_table(plain))


def test_an_unflagged_call_reports_no_utf8_pattern(ctx, resident):
    case = next(c for c in utf8_cases.FUZZY_CASES if c.name == "bytes-against-symbols")
    plain = case._replace(name="bytes-only", flags=[f & ~UTF8 for f in case.flags])
    got = _fuzzy(ctx, resident["fuzzy:" + case.name], plain)
    _check_fuzzy(got, utf8_cases.expected_fuzzy(plain))
    assert got[4].n_utf8 == 0 and got[4].word_bits == 32
    assert _fuzzy(ctx, resident["fuzzy:" + case.name], case)[4].n_utf8 == 6


def test_one_term_of_three_byte_symbols_longer_than_the_stage(ctx):
    """6000 three-byte symbols are 18 000 bytes: no stage holds that workgroup, it reads global memory alone"""
    long_term = u(0x65E5) * 5990 + "日本語".encode() + u(0x65E5) * 7
    assert len(long_term) > 16384
    terms = sorted([b"%04d" % i + ("日本語" if i % 7 == 0 else "日本").encode() for i in range(700)] + [long_term, "日本語".encode(), "日本话".encode(), "日本".encode()])
    d = ctx.dictionary(terms)
    case = utf8_cases._fuzzy("long-term", [terms], ["日本語".encode(), "0007日本語".encode(), "日本語".encode(), u(0x65E5) * 21], [1, 2, 1, 255], [0, 4, 0, 1], [UTF8, UTF8, 0, UTF8])
    got = _fuzzy(ctx, [d], case)
    _check_fuzzy(got, utf8_cases.expected_fuzzy(case))
    st = got[4]
    n_wg = (len(terms) + 255) // 256
    assert st.n_global == 1 and st.n_staged == n_wg - 1 and st.n_utf8 == 3
    assert utf8_cases.expected_fuzzy(case)[4] >= 5 and utf8_cases.expected_fuzzy(case)[0][-1] >= 4        # (the inputs are not trivial)
    mcase = utf8_cases._match("long-term", [terms], [b"*" + "日本語".encode() + b"*", b"????" + "日本?".encode(), b"?" * 64, "日本語".encode()],
                              [GLOB | UTF8, GLOB | UTF8, GLOB | UTF8, UTF8])
    got = ctx.dict_match([d], mcase.patterns, _u8(mcase.kinds))
    _check_match(got, utf8_cases.expected_match(mcase))
    assert got[4].n_global == 1 and got[4].n_staged == n_wg - 1 and got[4].n_matched >= 100
    d.free()


def _raw_setup(ctx):
    terms = utf8_cases.numbered(600, lambda i: i % 3 == 0)
    d = ctx.dictionary(terms)
    pats = [b"00000" + u(0xE9), b"00000" + u(0x20AC) * 7, b"0"]
    blob, off = fuzzy_cases.flat(pats)
    blob, off = np.frombuffer(blob, np.uint8).copy(), np.array(off, np.uint64)
    dist, pre, fl = _u8([5, 5, 255]), _u8([0, 2, 1]), _u8([UTF8, UTF8 | TRANSPOSE, UTF8])
    case = utf8_cases._fuzzy("raw", [terms, terms], pats, dist.tolist(), pre.tolist(), fl.tolist())
    return d, blob, off, dist, pre, fl, utf8_cases.expected_fuzzy(case)


def _stats(st):
    return (st.n_terms, st.n_matched, st.n_runs, st.n_tested, st.n_staged, st.n_global, st.word_bits, st.n_utf8)


def test_capacity_protocol_with_flagged_patterns(ctx):
    d, blob, off, dist, pre, fl, want = _raw_setup(ctx)
    w_off, w_first, w_end, w_which, w_matched, w_tested = want
    need = w_off[-1]
    assert need == 2 * (200 + 200 + 1)
    run_off = np.full(7, FILL64, np.uint64)
    first, end, which = np.full(need + 8, FILL64, np.uint64), np.full(need + 8, FILL64, np.uint64), np.full(need + 8, FILL32, np.uint32)
    rc, st = ctx.dict_fuzzy_flat([d, d], blob, off, dist, pre, fl, run_off, first, end, which, need - 1)
    assert rc == -4 and run_off.tolist() == w_off                       # II2_ECAPACITY: run_off and the stats are complete ...
    assert _stats(st) == (1200, w_matched, need, w_tested, 6, 0, 32, 3)
    assert (first == FILL64).all() and (end == FILL64).all() and (which == FILL32).all()      # ... the runs untouched
    rc, st2 = ctx.dict_fuzzy_flat([d, d], blob, off, dist, pre, fl, run_off, first, end, which, int(run_off[-1]))
    assert rc == 0 and first[:need].tolist() == w_first and end[:need].tolist() == w_end and which[:need].tolist() == w_which
    assert (first[need:] == FILL64).all() and (end[need:] == FILL64).all() and (which[need:] == FILL32).all()
    assert _stats(st2) == _stats(st)
    d.free()


def test_argument_errors_leave_the_outputs_untouched(ctx):
    d, blob, off, dist, pre, fl, want = _raw_setup(ctx)
    need = want[0][-1]
    run_off = np.full(7, FILL64, np.uint64)
    first, end, which = np.full(need, FILL64, np.uint64), np.full(need, FILL64, np.uint64), np.full(need, FILL32, np.uint32)
    stats = np.full(6, FILL64, np.uint64)
    arr = (C.c_void_p * 2)(d.h, d.h)
    p = lambda a: a.ctypes.data if a is not None else None

    def untouched():
        return (run_off == FILL64).all() and (first == FILL64).all() and (end == FILL64).all() and (which == FILL32).all() and (stats == FILL64).all()

    def fuzzy(b=blob, o=off, pr=pre, f=fl):
        return ctx.lib.ii2_dict_fuzzy(ctx.h, 2, arr, 3, p(b), p(o), p(dist), p(pr), p(f), p(run_off), p(first), p(end), p(which), need,
                                      C.cast(p(stats), C.POINTER(_lib.FuzzyStats)))

    def match(b, o, kinds):
        return ctx.lib.ii2_dict_match(ctx.h, 2, arr, 3, p(b), p(o), p(_u8(kinds)), p(run_off), p(first), p(end), p(which), need,
                                      C.cast(p(stats), C.POINTER(_lib.MatchStats)))

    def flat(pats):
        b, o = fuzzy_cases.flat(pats)
        return np.frombuffer(b, np.uint8).copy(), np.array(o, np.uint64)

    with path_delta(ctx) as moved:
        for bad in (b"\x80", b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"a\xe2\x82", b"\xff"):       # an ill-formed pattern, in any place
            for at in range(3):
                pats = [b"a", b"b", b"c"]
                pats[at] = bad
                b, o = flat(pats)
                assert fuzzy(b=b, o=o, pr=None) == -1 and untouched(), (bad, at)
                assert match(b, o, [UTF8, GLOB | UTF8, 1 | UTF8]) == -1 and untouched(), (bad, at)
                only_plain = [UTF8] * 3
                only_plain[at] = 0
                assert fuzzy(b=b, o=o, pr=None, f=_u8(only_plain)) == 0                   # accepted where that pattern is unflagged
                run_off[:], first[:], end[:], which[:], stats[:] = FILL64, FILL64, FILL64, FILL32, FILL64
        assert fuzzy(pr=_u8([7, 2, 1])) == -1 and untouched()                              # a prefix above the SYMBOL count: 00000 + one symbol is 6
        assert fuzzy(pr=_u8([6, 13, 1])) == -1 and untouched()
        assert fuzzy(pr=_u8([6, 12, 2])) == -1 and untouched()
        assert fuzzy(pr=_u8([7, 2, 1]), f=_u8([0, UTF8, UTF8])) == 0                        # seven BYTES: fine without the flag
        run_off[:], first[:], end[:], which[:], stats[:] = FILL64, FILL64, FILL64, FILL32, FILL64
        for f in ([UTF8 | 2, 0, 0], [0, UTF8 | 0x40, 0], [0, 0, UTF8 | 4]):                 # the other bits stay unknown
            assert fuzzy(f=_u8(f)) == -1 and untouched(), f
        b, o = flat([b"a", b"b", b"c"])
        for kinds in ([UTF8 | 3, 0, 0], [0, UTF8 | 0x40 | GLOB, 0], [0, 0, UTF8 | 4]):
            assert match(b, o, kinds) == -1 and untouched(), kinds
        b, o = flat([b"a\\", b"b", b"c"])
        assert match(b, o, [UTF8 | GLOB, 0, 0]) == -1 and untouched()
        b, o = flat([u(0xE9) * 32 + b"a", b"b", b"c"])                                      # 65 bytes: the limit stays in bytes
        assert fuzzy(b=b, o=o, pr=None) == -5 and untouched() and match(b, o, [UTF8, 0, 0]) == -5 and untouched()
        # the regular expressions keep rejecting the bit
        rstats = np.full(6, FILL64, np.uint64)
        b, o = flat([b"a", b"b", b"c"])
        rc = ctx.lib.ii2_dict_regex(ctx.h, 2, arr, 3, p(b), p(o), p(_u8([0, UTF8, 0])), p(run_off), p(first), p(end), p(which), need,
                                    C.cast(p(rstats), C.POINTER(_lib.RegexStats)))
        assert rc == -1 and untouched() and (rstats == FILL64).all()
        assert fuzzy() == 0 and run_off.tolist() == want[0] and first.tolist() == want[1] and end.tolist() == want[2] and which.tolist() == want[3]
    assert moved == {}
    d.free()


def test_runs_feed_union_ranges_verbatim(ctx):
    rng = np.random.default_rng(43)
    vocab = sorted(w.encode("utf-8") for w in ("café", "cafe", "cafés", "caffè", "caf", "carafe", "cafetière", "thé", "the", "日本語", "日本话", "naïve", "naive"))
    k = 3
    terms_of = [sorted(vocab[int(i)] for i in rng.choice(len(vocab), n, replace=False)) for n in (len(vocab), 9, 5)]
    lists_of = [[np.unique(rng.integers(0, 3000, int(rng.integers(1, 200)))).astype(np.uint32) for _ in terms] for terms in terms_of]
    segs = [ctx.encode_lists(lists) for lists in lists_of]
    dicts = [ctx.dictionary(terms) for terms in terms_of]
    pat = "café".encode()
    run_off, first, end, which, st = ctx.dict_fuzzy(dicts, [pat, pat], _u8([1, 1]), 0, _u8([UTF8, 0]))
    assert st.n_utf8 == 1
    sizes = []
    for p, fl in enumerate((UTF8, 0)):
        a, b = int(run_off[p * k]), int(run_off[(p + 1) * k])
        group = [(segs[int(which[j])], int(first[j]), int(end[j])) for j in range(a, b)]
        want = set()
        for s in range(k):
            for t, l in zip(terms_of[s], lists_of[s]):
                if utf8_cases.matches(pat, t, 1, 0, fl):
                    want |= set(l.tolist())
        out, n = ctx.union_ranges(group)
        assert out.download(n).tolist() == sorted(want), fl
        out.free()
        sizes.append(len(want))
    assert sizes[0] > sizes[1] > 0                       # `cafe` is one edit away by symbols, two by bytes
    for x in segs + dicts:
        x.free()
