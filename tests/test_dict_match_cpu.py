"""CPU: the matchers of ii2_dict_match (csrc/match_device.h) through the host-only ii2_term_match, which parses a pattern and
matches it by the functions the kernel runs - so every (pattern, term) of tests/match_cases.py is pinned here without a GPU;
tests/test_gpu_dict_match.py runs the same table through the kernels.  Also every argument error of ii2_term_match, and the
table's own coverage."""
import ctypes as C
import os
import re

import pytest

from inverted_index_2_amd import _lib
from inverted_index_2_amd.engine import II2Error, term_match
from tests import match_cases
from tests.match_cases import CONTAINS, GLOB, NOCASE, SUFFIX


def _raw(kind, pat, pat_len, term, term_len, out=True):
    lib = _lib.load()
    m = C.c_int(77)
    rc = lib.ii2_term_match(kind, pat, pat_len, term, term_len, C.byref(m) if out else None)
    return rc, m.value


@pytest.mark.parametrize("case", match_cases.CASES, ids=lambda c: c.name)
def test_every_pattern_against_every_term(case):
    lib = _lib.load()
    m = C.c_int()
    terms = sorted({t for d in case.dicts for t in d})
    for p, kind in zip(case.patterns, case.kinds):
        want = match_cases.matcher(kind, p)
        for t in terms:
            assert lib.ii2_term_match(kind, p or None, len(p), t or None, len(t), C.byref(m)) == 0
            assert bool(m.value) == want(t), (kind, p, t)


def test_the_motivating_examples():
    assert term_match(CONTAINS, b"timeout", b"connection_timeout") and not term_match(CONTAINS, b"timeout", b"timeou")
    assert term_match(GLOB, b"*.example.com", b"a.example.com") and not term_match(GLOB, b"*.example.com", b"example.com")
    assert term_match(GLOB, b"user_?d", b"user_id") and not term_match(GLOB, b"user_?d", b"user_d")
    assert term_match(CONTAINS | NOCASE, b"ERROR", b"an Error!") and not term_match(CONTAINS, b"ERROR", b"an Error!")
    assert term_match(SUFFIX, b"", b"") and term_match(CONTAINS, b"", b"") and term_match(GLOB, b"", b"") and not term_match(GLOB, b"", b"a")
    # backtracking
    for pat, yes, no in ((b"*ab*ab", [b"abab", b"ababab"], [b"aab"]), (b"a*a*a", [b"aaa", b"aXaYa"], [b"aa"]), (b"*a?", [b"aa", b"aaa"], [b"a"])):
        assert all(term_match(GLOB, pat, t) for t in yes) and not any(term_match(GLOB, pat, t) for t in no), pat
    # only A-Z folds
    for a, b in ((b"[", b"{"), (b"@", b"`"), (b"\xc9", b"\xe9")):
        assert not term_match(GLOB | NOCASE, a, b) and not term_match(SUFFIX | NOCASE, b, a) and term_match(CONTAINS | NOCASE, a, a)
    # a literal, escaped wildcard does not fold into anything, an escaped letter does
    assert term_match(GLOB | NOCASE, b"\\A\\*", b"a*") and not term_match(GLOB | NOCASE, b"\\A\\*", b"ab")


def test_a_long_term_and_the_longest_pattern():
    term = b"x" * 40_000 + b"needle" + b"y" * 9
    assert term_match(CONTAINS, b"needle", term) and term_match(GLOB, b"x*needle*y", term) and term_match(SUFFIX, b"e" + b"y" * 9, term)
    assert not term_match(GLOB, b"x*needle", term) and not term_match(CONTAINS, b"needlex", term)
    pat = b"ab" * 32
    assert term_match(CONTAINS, pat, b"b" + pat + b"a") and term_match(SUFFIX, pat, b"b" + pat) and term_match(GLOB, pat, pat)
    assert term_match(GLOB, b"*" * 64, b"") and term_match(GLOB, b"?" * 64, b"q" * 64) and not term_match(GLOB, b"?" * 64, b"q" * 63)


def test_argument_errors():
    assert _raw(CONTAINS, b"a", 1, b"a", 1, out=False)[0] == -1              # NULL output
    assert _raw(CONTAINS, None, 1, b"a", 1) == (-1, 77)                      # NULL pattern of one byte
    assert _raw(CONTAINS, b"a", 1, None, 1) == (-1, 77)                      # NULL term of one byte
    for kind in (3, 4, 0x7f, 0x83, 0x100, 0x180, 0xFFFFFFFF):                # unknown kinds, with and without the flag
        assert _raw(kind, b"a", 1, b"a", 1) == (-1, 77), kind
    for pat in (b"\\", b"a\\", b"*\\", b"\\\\\\"):                           # a lone backslash at the end of a glob ...
        assert _raw(GLOB, pat, len(pat), b"a", 1) == (-1, 77), pat
        assert _raw(GLOB | NOCASE, pat, len(pat), b"a", 1) == (-1, 77), pat
        assert _raw(CONTAINS, pat, len(pat), pat, len(pat)) == (0, 1), pat   # ... is a plain byte of the literal kinds
        assert _raw(SUFFIX, pat, len(pat), b"x" + pat, len(pat) + 1) == (0, 1), pat
    for kind in (CONTAINS, SUFFIX, GLOB, GLOB | NOCASE):                     # 65 bytes: out of range, 64: fine
        assert _raw(kind, b"a" * 65, 65, b"a" * 65, 65) == (-5, 77), kind
        assert _raw(kind, b"a" * 64, 64, b"a" * 64, 64) == (0, 1), kind
    assert _raw(GLOB, b"\\a" * 32, 64, b"a" * 32, 32) == (0, 1)              # the limit counts the pattern's bytes, escapes included
    assert _raw(GLOB, b"\\a" * 32 + b"a", 65, b"a" * 33, 33) == (-5, 77)
    assert _raw(CONTAINS, None, 0, None, 0) == (0, 1)                        # NULL with length 0 is the empty string
    with pytest.raises(II2Error) as e:
        term_match(GLOB, b"oops\\", b"oops")
    assert e.value.code == -1


def test_the_table_covers_what_it_claims():
    cases = {c.name: c for c in match_cases.CASES}
    assert len(cases) == len(match_cases.CASES)
    assert {len(c.dicts) for c in match_cases.CASES} >= {1, 3, 64}
    assert any(not d for c in match_cases.CASES for d in c.dicts) and any(c.dicts == [[]] for c in match_cases.CASES)
    assert any(len(d) >= 5000 for c in match_cases.CASES for d in c.dicts)
    assert any(len(c.patterns) == 64 and all(len(p) == 64 for p in c.patterns) for c in match_cases.CASES)
    kinds = {k for c in match_cases.CASES for k in c.kinds}
    assert kinds == {CONTAINS, SUFFIX, GLOB, CONTAINS | NOCASE, SUFFIX | NOCASE, GLOB | NOCASE}
    # the empty term with the empty pattern of each kind
    assert any(b"" in d and (b"", k) in zip(c.patterns, c.kinds) for c in match_cases.CASES for d in c.dicts for k in kinds) and \
        all(any(b"" in d and (b"", k) in zip(c.patterns, c.kinds) for c in match_cases.CASES for d in c.dicts) for k in kinds)
    # dense matches and long runs in the big dictionary; some pair without any run
    off, first, end, _, matched = match_cases.expected_table(cases["ternary-5000"])
    assert matched > 20_000 and max(e - f for f, e in zip(first, end)) >= 1000
    assert any(a == b for a, b in zip(off, off[1:]))
    # the expectation's own arithmetic
    assert match_cases.runs_of([1, 1, 0, 1, 0, 0, 1]) == [(0, 2), (3, 4), (6, 7)] and match_cases.runs_of([]) == [] and match_cases.runs_of([0]) == []
    assert match_cases.glob_regex(b"a\\") is None and match_cases.glob_regex(b"a.\\*?*").pattern == b"a\\.\\*..*"


# ---- the layers around the kernel keep in step ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_library_exports_both_calls_and_the_makefile_builds_the_kernel():
    lib = _lib.load()
    assert hasattr(lib, "ii2_dict_match") and hasattr(lib, "ii2_term_match")
    mk = _read("inverted_index_2_amd", "csrc", "Makefile")
    assert "build/dict_match.o" in mk and "match_device.h" in mk
    assert C.sizeof(_lib.MatchStats) == 32
    header = _read("include", "ii2.h")
    for name, value in (("II2_MATCH_MAX_PATTERN", _lib.II2_MATCH_MAX_PATTERN), ("II2_MATCH_MAX_PATTERNS", _lib.II2_MATCH_MAX_PATTERNS)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), header), name
    assert re.search(r"II2_MATCH_CONTAINS = 0, II2_MATCH_SUFFIX = 1, II2_MATCH_GLOB = 2", header) and re.search(r"#define\s+II2_MATCH_NOCASE\s+0x80u", header)
    assert (_lib.II2_MATCH_CONTAINS, _lib.II2_MATCH_SUFFIX, _lib.II2_MATCH_GLOB, _lib.II2_MATCH_NOCASE) == (CONTAINS, SUFFIX, GLOB, NOCASE)


def test_the_matchers_are_defined_once_and_parsed_on_the_host():
    csrc = os.path.join(ROOT, "inverted_index_2_amd", "csrc")
    defined = {}
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".h", ".hip", ".cpp")):
            for name in ("match_glob", "match_contains", "match_suffix", "match_parse"):
                if re.search(r"\b(?:int|bool)\s+%s\s*\(" % name, _read("inverted_index_2_amd", "csrc", f)):
                    defined.setdefault(name, []).append(f)
    assert defined == {n: ["match_device.h"] for n in ("match_glob", "match_contains", "match_suffix", "match_parse")}
    kernel = _read("inverted_index_2_amd", "csrc", "dict_match.hip")
    assert '#include "match_device.h"' in kernel and "'\\\\'" not in kernel      # no backslash handling outside the one parse


def test_go_binding_and_host_mirror_declare_the_calls():
    go = _read("bindings", "go", "ii2.go")
    assert "C.ii2_dict_match(" in go and "func (c *Ctx) DictMatch(" in go and "C.ii2_term_match(" in go
    assert "func MatchSearch(" in _read("bindings", "go", "index.go")
    src = _read("inverted_index_2_amd", "host", "host_index.cpp")
    assert "int ii2h_match_search(" in src and "int ii2h_match_terms(" in src and "ii2_dict_match(" in src
    host_py = _read("inverted_index_2_amd", "host.py")
    assert "def match_search(" in host_py and "def match_terms(" in host_py
