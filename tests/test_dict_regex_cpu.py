"""CPU: the matcher of ii2_dict_regex (csrc/regex_device.h) through the host-only ii2_term_regex, which parses a pattern into
its position automaton and runs the filter and the step the kernel runs - so every (pattern, term) of tests/regex_cases.py is
pinned here without a GPU against Python's `re`; tests/test_gpu_dict_regex.py runs the same table through the kernel.  Also the
table of patterns that must not parse, a seeded random differential over a small grammar, the position counts, every argument
error of ii2_term_regex, the table's own coverage, and the layers around the kernel."""
import ctypes as C
import itertools
import os
import random
import re

import pytest

from inverted_index_2_amd import _lib, term_regex
from inverted_index_2_amd.engine import II2Error
from tests import regex_cases
from tests.regex_cases import NOCASE, matches

EINVAL, ERANGE = -1, -5


def _raw(flags, pat, term, out=True, want_pos=True):
    lib = _lib.load()
    m, n = C.c_int(77), C.c_uint32(88)
    rc = lib.ii2_term_regex(flags, pat or None, len(pat), term or None, len(term), C.byref(m) if out else None, C.byref(n) if want_pos else None)
    return rc, m.value, n.value


@pytest.mark.parametrize("case", regex_cases.CASES, ids=lambda c: c.name)
def test_every_pattern_against_every_term(case):
    lib = _lib.load()
    m = C.c_int()
    terms = sorted({t for d in case.dicts for t in d})
    for p, fl in zip(case.patterns, case.flags):
        for t in terms:
            assert lib.ii2_term_regex(fl, p or None, len(p), t or None, len(t), C.byref(m), None) == 0, (p, fl)
            assert bool(m.value) == matches(p, t, fl), (p, t, fl)


def test_the_motivating_examples():
    assert term_regex(b"(error|fail|timeout)[0-9]{3}", b"fail404") == (True, 19) and not term_regex(b"(error|fail|timeout)[0-9]{3}", b"fail40")[0]
    assert term_regex(b"[a-f0-9]{32}", b"0123456789abcdef" * 2) == (True, 32) and not term_regex(b"[a-f0-9]{32}", b"0123456789abcdeg" * 2)[0]
    assert term_regex(b"req-[0-9]+-.*", b"req-17-x\ny")[0] and not term_regex(b"req-[0-9]+-.*", b"req--x")[0]
    assert term_regex(b"foo", b"foo")[0] and not term_regex(b"foo", b"xfoo")[0] and not term_regex(b"foo", b"foox")[0]       # the WHOLE term
    assert term_regex(b".*foo.*", b"xfoox")[0]
    assert term_regex(b"", b"") == (True, 0) and term_regex(b"", b"a") == (False, 0)
    assert not term_regex(b"[^a]", b"A", NOCASE)[0] and term_regex(b"[^a]", b"A")[0]
    assert term_regex(b"[Z-a]", b"z", NOCASE)[0] and term_regex(b"[Z-a]", b"A", NOCASE)[0] and not term_regex(b"[Z-a]", b"z")[0]
    for a, b in ((b"\\[", b"{"), (b"@", b"`"), (b"\\xc9", b"\xe9")):                       # only the ASCII letters fold
        assert not term_regex(a, b, NOCASE)[0]


@pytest.mark.parametrize("pattern,n_pos", sorted(regex_cases.N_POS.items()))
def test_positions(pattern, n_pos):
    assert term_regex(pattern, b"")[1] == n_pos and term_regex(pattern, b"", NOCASE)[1] == n_pos


def test_patterns_that_do_not_parse():
    for p in regex_cases.INVALID:
        for fl in (0, NOCASE):
            assert _raw(fl, p, b"a") == (EINVAL, 77, 88), p
    for p, n in regex_cases.TOO_MANY_POSITIONS:
        assert _raw(0, p, b"a") == (ERANGE, 77, n), p            # the count that was too large
        assert _raw(0, p, b"a", want_pos=False)[0] == ERANGE
    for p in regex_cases.AT_THE_POSITION_LIMIT:
        assert _raw(0, p, b"a")[::2] == (0, 64), p
    assert len(regex_cases.TOO_LONG) == 257 and _raw(0, regex_cases.TOO_LONG, b"a") == (ERANGE, 77, 88)
    assert len(regex_cases.AT_THE_LENGTH_LIMIT) == 256 and _raw(0, regex_cases.AT_THE_LENGTH_LIMIT, b"a") == (0, 1, 1)
    assert _raw(0, regex_cases.AT_THE_LENGTH_LIMIT, b"") == (0, 1, 1)                      # (its empty alternatives)
    with pytest.raises(II2Error) as e:
        term_regex(b"a{65}", b"")
    assert e.value.code == ERANGE and e.value.n_pos == 65
    with pytest.raises(II2Error) as e:
        term_regex(b"a**", b"")
    assert e.value.code == EINVAL


def test_argument_errors():
    assert _raw(0, b"a", b"a", out=False)[0] == EINVAL               # NULL match
    lib = _lib.load()
    m = C.c_int(77)
    assert lib.ii2_term_regex(0, None, 1, b"a", 1, C.byref(m), None) == EINVAL and m.value == 77      # NULL pattern of one byte
    assert lib.ii2_term_regex(0, b"a", 1, None, 1, C.byref(m), None) == EINVAL and m.value == 77      # NULL term of one byte
    for flags in (0x01, 0x02, 0x40, 0x7f, 0x100, 0x180, 0x8000, 0xFFFFFFFF, 0x81):      # a flag bit other than NOCASE
        assert _raw(flags, b"a", b"a") == (EINVAL, 77, 88), flags
    assert _raw(0, b"", b"") == (0, 1, 0) and _raw(NOCASE, b"a", b"A") == (0, 1, 1) and _raw(0, b"a", b"A", want_pos=False) == (0, 0, 88)


_ATOMS = [b"a", b"b", b"c", b".", b"[ab]", b"[^a]", b"\\w"]
_QUANTIFIERS = [b"*", b"+", b"?", b"{0}", b"{2}", b"{1,3}", b"{2,}", b"{0,1}", b"{0,}", b"*?", b"+?", b"??", b"{0,2}?", b"{1,}?"]


def _grammar(rng, depth):
    r = rng.random()
    if depth == 0 or r < 0.3:
        return rng.choice(_ATOMS)
    if r < 0.55:
        return b"".join(_grammar(rng, depth - 1) for _ in range(rng.randrange(1, 4)))
    if r < 0.7:
        return b"(" + b"|".join(_grammar(rng, depth - 1) if rng.random() < 0.85 else b"" for _ in range(rng.randrange(2, 4))) + b")"
    if r < 0.8:
        return rng.choice(_ATOMS) + rng.choice(_QUANTIFIERS)
    return rng.choice((b"(", b"(?:")) + _grammar(rng, depth - 1) + b")" + rng.choice(_QUANTIFIERS)


def test_random_patterns_against_re():
    """1200 patterns of a small grammar - concatenation, alternation, empty alternatives, every quantifier form on atoms and
    groups - against every string of length 0 .. 5 over a, b, Z and a line feed, plain and under NOCASE"""
    rng = random.Random(7)
    strings = [bytes(s) for n in range(6) for s in itertools.product(b"abZ\n", repeat=n)]
    lib = _lib.load()
    m, n_pos = C.c_int(), C.c_uint32()
    skipped, total, largest = 0, 1200, 0
    for i in range(total):
        p = _grammar(rng, 3)
        fl = NOCASE if i % 3 == 0 else 0
        rc = lib.ii2_term_regex(fl, p, len(p), None, 0, C.byref(m), C.byref(n_pos))
        if rc == ERANGE and n_pos.value > 64:
            skipped += 1
            continue
        assert rc == 0, p
        largest = max(largest, n_pos.value)
        rx = regex_cases.compiled(p, fl)
        for s in strings:
            assert lib.ii2_term_regex(fl, p, len(p), s or None, len(s), C.byref(m), None) == 0
            assert bool(m.value) == (rx.fullmatch(s) is not None), (p, s, fl)
    assert skipped < total * 0.05 and largest >= 12


def test_the_deepest_nesting():
    """a pattern of 256 bytes nests at most 127 groups around one position: the parser recurses once per group"""
    for depth, inner in ((127, b"ab"), (126, b"a{2}"), (125, b"a|bc"), (84, b"")):
        for opened in (b"(", b"(?:"):
            if depth * (len(opened) + 1) + len(inner) > 256:
                continue
            p = opened * depth + inner + b")" * depth
            rx = regex_cases.compiled(p, 0)
            for t in (b"", b"a", b"aa", b"ab", b"bc", b"abc"):
                assert term_regex(p, t)[0] == (rx.fullmatch(t) is not None), (depth, inner, t)
    assert len(b"(" * 127 + b"ab" + b")" * 127) == 256
    p = b"(" * 60 + b"a" + b"){2}" * 6 + b")" * 54                      # counted repetitions re-parse nested groups: 2^6 positions
    assert term_regex(p, b"a" * 64) == (True, 64) and not term_regex(p, b"a" * 63)[0]
    with pytest.raises(II2Error) as e:
        term_regex(b"(" * 127 + b"ab" + b")" * 126, b"ab")
    assert e.value.code == EINVAL


def test_a_very_long_term():
    term = b"x" * 20_000 + b"needle" + b"y" * 19_994
    assert term_regex(b".*needle.*", term)[0] and term_regex(b"x+needley+", term)[0] and not term_regex(b"x+needlex+", term)[0]
    assert term_regex(b"[xy]*n[^xy]{4}e[xy]*", term)[0] and not term_regex(b".{64}", term)[0] and not term_regex(b"x*", term)[0]


def test_the_table_covers_what_it_claims():
    cases = {c.name: c for c in regex_cases.CASES}
    assert len(cases) == len(regex_cases.CASES)
    assert all(len(c.patterns) <= 8 for c in regex_cases.CASES)
    assert {len(c.dicts) for c in regex_cases.CASES} >= {1, 3, 64}
    assert any(not d for c in regex_cases.CASES for d in c.dicts if len(c.dicts) == 3) and any(c.dicts == [[]] for c in regex_cases.CASES)
    assert any(c.dicts == [[b""]] for c in regex_cases.CASES)
    assert len({len(d) for d in cases["k64-unequal"].dicts}) >= 5
    assert all(len(d) <= 5000 for c in regex_cases.CASES for d in c.dicts) and any(len(d) == 5000 for c in regex_cases.CASES for d in c.dicts)
    # the position counts at the word's edges, each with a term that ends in the last position and one that stops short of it
    we = cases["word-edges"]
    assert [regex_cases.N_POS[p] for p in we.patterns] == [1, 31, 32, 33, 63, 64, 64, 64]
    for p in we.patterns:
        hits = [t for t in we.dicts[0] if matches(p, t, 0)]
        assert hits and any(not matches(p, t[:-1], 0) for t in hits), p
    assert all(regex_cases.N_POS[p] == 64 for p in cases["ternary-5000-8-patterns-of-64-positions"].patterns) and len(regex_cases.CALL_OF_64) == 8
    assert {regex_cases.EVERY_LOOPS, regex_cases.HALF_LOOPS} <= set(cases["every-position-in-the-loop"].patterns)
    # the empty term, the empty pattern
    assert any(b"" in d and b"" in c.patterns for c in regex_cases.CASES for d in c.dicts)
    # the length filter: terms of length min - 1, min, max, max + 1 for the bounded patterns, and unbounded ones
    lf = cases["length-filter"]
    have = {len(t) for t in lf.dicts[0]}
    for p, (lo, hi) in regex_cases.WIDTHS.items():
        assert regex_cases.width(p) == (lo, hi), p
        assert {n for n in (lo - 1, lo, hi, None if hi is None else hi + 1) if n is not None and n >= 0} <= have, p
    assert any(hi is None for _, hi in regex_cases.WIDTHS.values())
    assert all(e[4] < e[5] for e in (regex_cases.expected_table(lf),))
    # terms longer than the word that match, and some that do not
    lt = cases["long-terms"]
    assert sum(len(t) > 64 and matches(p, t, 0) for p in lt.patterns for t in lt.dicts[0]) >= 8
    assert sum(len(t) > 64 and not matches(p, t, 0) for p in lt.patterns for t in lt.dicts[0]) >= 8
    # the fold: both settings on the same inputs
    assert cases["nocase-neighbours-of-the-letters"].patterns == cases["nocase-against-plain"].patterns
    assert regex_cases.expected_table(cases["nocase-neighbours-of-the-letters"])[:3] != regex_cases.expected_table(cases["nocase-against-plain"])[:3]
    assert {f for c in regex_cases.CASES for f in c.flags} == {0, NOCASE}
    # long runs across the workgroup edges in the big dictionary, one from its first term, one to its last, a pair without a run
    off, first, end, _, matched, tested = regex_cases.expected_table(cases["ternary-5000"])
    assert max(e - f for f, e in zip(first, end)) == 5000 and sum(e - f >= 300 and f > 0 and e < 5000 for f, e in zip(first, end)) >= 1
    assert 0 in first and 5000 in end and any(f > 0 and e == 5000 for f, e in zip(first, end)) and any(f == 0 and e < 5000 for f, e in zip(first, end))
    assert any(a == b for a, b in zip(off, off[1:])) and matched < tested < 8 * 5000
    # every II2_EINVAL form is there once
    assert len(set(regex_cases.INVALID)) == len(regex_cases.INVALID) >= 60


# ---- the layers around the kernel keep in step ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_library_exports_both_calls_and_the_makefile_builds_the_kernel():
    lib = _lib.load()
    assert hasattr(lib, "ii2_dict_regex") and hasattr(lib, "ii2_term_regex")
    mk = _read("inverted_index_2_amd", "csrc", "Makefile")
    assert "build/dict_regex.o" in mk and "regex_device.h" in mk and "match_runs.h" in mk
    assert C.sizeof(_lib.RegexStats) == 48
    header = _read("include", "ii2.h")
    for name, value in (("II2_REGEX_MAX_PATTERN", _lib.II2_REGEX_MAX_PATTERN), ("II2_REGEX_MAX_POSITIONS", _lib.II2_REGEX_MAX_POSITIONS),
                        ("II2_REGEX_MAX_PATTERNS", _lib.II2_REGEX_MAX_PATTERNS)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), header), name
    assert (_lib.II2_REGEX_MAX_PATTERN, _lib.II2_REGEX_MAX_POSITIONS, _lib.II2_REGEX_MAX_PATTERNS) == \
        (regex_cases.MAX_PATTERN, regex_cases.MAX_POSITIONS, regex_cases.MAX_PATTERNS) == (256, 64, 8)
    assert "ii2_regex_stats" in header and "ii2_regex_stats;            /* 48 bytes */" in header


def test_the_matcher_and_the_parse_are_defined_once():
    csrc = os.path.join(ROOT, "inverted_index_2_amd", "csrc")
    names = ("regex_parse", "regex_step", "regex_term", "regex_passes")
    defined = {}
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".h", ".hip", ".cpp")):
            src = _read("inverted_index_2_amd", "csrc", f)
            for name in names:
                if re.search(r"\b(?:int|bool|void|uint32_t|uint64_t)\s+%s\s*\(" % name, src):
                    defined.setdefault(name, []).append(f)
    assert defined == {n: ["regex_device.h"] for n in names}
    kernel = _read("inverted_index_2_amd", "csrc", "dict_regex.hip")
    assert '#include "regex_device.h"' in kernel and '#include "match_runs.h"' in kernel
    # the part behind the match word is shared with ii2_dict_match, not copied
    for name in ("k_match_place", "k_match_offsets", "int match_runs_drive("):
        holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".cpp")) and re.search(r"(__global__[^;{]*\b%s\b|^%s)" % (re.escape(name), re.escape(name)),
                                                                                                      _read("inverted_index_2_amd", "csrc", f), re.M)]
        assert holders == ["dict_match.hip"], (name, holders)
    assert "match_runs_tail<2>" in kernel and "match_call<RegexPattern>" in kernel and "TermStage" in kernel
    assert '"regex.stage"' in _read("inverted_index_2_amd", "csrc", "api.cpp") and "opt_regex_stage" in _read("inverted_index_2_amd", "csrc", "internal.h")


def test_go_binding_and_host_mirror_declare_the_calls():
    go = _read("bindings", "go", "ii2.go")
    assert "C.ii2_dict_regex(" in go and "func (c *Ctx) DictRegex(" in go and "C.ii2_term_regex(" in go and "func TermRegex(" in go
    index_go = _read("bindings", "go", "index.go")
    assert "func RegexSearch(" in index_go and "func RegexTerms(" in index_go
    src = _read("inverted_index_2_amd", "host", "host_index.cpp")
    assert "int ii2h_regex_search(" in src and "int ii2h_regex_terms(" in src and "ii2_dict_regex(" in src
    host_py = _read("inverted_index_2_amd", "host.py")
    assert "def regex_search(" in host_py and "def regex_terms(" in host_py
