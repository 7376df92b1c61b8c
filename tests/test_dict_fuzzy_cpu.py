"""CPU: the matcher of ii2_dict_fuzzy (csrc/fuzzy_device.h) through the host-only ii2_term_fuzzy, which parses a pattern, builds
its table and runs the filters and the recurrence the kernel runs - so every (pattern, term) of tests/fuzzy_cases.py is pinned
here without a GPU, match and exact distance; tests/test_gpu_dict_fuzzy.py runs the same table through the kernels.  Also a very
long term, every argument error of ii2_term_fuzzy, the table's own coverage, and the layers around the kernel."""
import ctypes as C
import os
import random
import re

import pytest

from inverted_index_2_amd import _lib, term_fuzzy
from inverted_index_2_amd.engine import II2Error
from tests import fuzzy_cases
from tests.fuzzy_cases import NOCASE, TRANSPOSE, distance, levenshtein, matches, osa


def _raw(flags, pat, pat_len, prefix, max_dist, term, term_len, out=True, want_dist=True):
    lib = _lib.load()
    m, d = C.c_int(77), C.c_uint32(88)
    rc = lib.ii2_term_fuzzy(flags, pat, pat_len, prefix, max_dist, term, term_len, C.byref(m) if out else None, C.byref(d) if want_dist else None)
    return rc, m.value, d.value


@pytest.mark.parametrize("case", fuzzy_cases.CASES, ids=lambda c: c.name)
def test_every_pattern_against_every_term(case):
    lib = _lib.load()
    m, dist = C.c_int(), C.c_uint32()
    terms = sorted({t for d in case.dicts for t in d})
    for p, d, pre, fl in zip(case.patterns, case.dists, case.prefixes, case.flags):
        for t in terms:
            assert lib.ii2_term_fuzzy(fl, p or None, len(p), pre, d, t or None, len(t), C.byref(m), C.byref(dist)) == 0
            assert bool(m.value) == matches(p, t, d, pre, fl), (p, t, d, pre, fl)
            assert dist.value == distance(p, t, fl), (p, t, fl)              # exact, whatever the prefix and max_dist are


def test_the_motivating_examples():
    assert term_fuzzy(b"kitten", b"sitting", 3) == (True, 3) and term_fuzzy(b"kitten", b"sitting", 2) == (False, 3)
    assert term_fuzzy(b"ca", b"abc", 2, flags=TRANSPOSE) == (False, 3) and term_fuzzy(b"ca", b"abc", 3) == (True, 3)
    assert term_fuzzy(b"abcd", b"bacd", 1, flags=TRANSPOSE) == (True, 1) and term_fuzzy(b"abcd", b"bacd", 1) == (False, 2)
    assert term_fuzzy(b"search", b"xearch", 1) == (True, 1) and term_fuzzy(b"search", b"xearch", 1, prefix=1) == (False, 1)
    assert term_fuzzy(b"search", b"se", 6, prefix=3) == (False, 4)                     # a term shorter than the prefix
    assert term_fuzzy(b"ERROR", b"errro", 1, flags=NOCASE | TRANSPOSE) == (True, 1) and term_fuzzy(b"ERROR", b"errro", 1, flags=TRANSPOSE) == (False, 5)
    assert term_fuzzy(b"", b"", 0) == (True, 0) and term_fuzzy(b"", b"abc", 2) == (False, 3) and term_fuzzy(b"", b"abc", 3) == (True, 3)
    assert term_fuzzy(b"abc", b"", 3) == (True, 3) and term_fuzzy(b"abc", b"", 2) == (False, 3)
    for a, b in ((b"[", b"{"), (b"@", b"`"), (b"\xc9", b"\xe9")):                       # only A-Z folds
        assert term_fuzzy(a, b, 0, flags=NOCASE) == (False, 1) and term_fuzzy(a, a, 0, flags=NOCASE) == (True, 0)
    assert term_fuzzy(b"abc", b"abc", 2 ** 32 - 1) == (True, 0) and term_fuzzy(b"abc", b"x" * 500, 2 ** 32 - 1) == (True, 500)      # any max_dist


def test_random_pairs_against_the_plain_dp():
    """both word sizes at their edges: pattern lengths around 32 and 64, terms shorter and longer than the word"""
    rng = random.Random(5)
    for _ in range(600):
        m = rng.choice((0, 1, 2, 7, 30, 31, 32, 33, 34, 62, 63, 64))
        alphabet = rng.choice((b"ab", b"abc", b"abcdefgh"))
        pat = bytes(rng.choice(alphabet) for _ in range(m))
        term = fuzzy_cases._edits(rng, pat, rng.randrange(0, 8), alphabet) if rng.random() < 0.7 else bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 90)))
        for fl, dp in ((0, levenshtein), (TRANSPOSE, osa)):
            d = dp(pat, term)
            assert term_fuzzy(pat, term, d, flags=fl) == (True, d), (pat, term, fl)
            if d:
                assert term_fuzzy(pat, term, d - 1, flags=fl) == (False, d), (pat, term, fl)


def test_a_very_long_term():
    term = b"x" * 20_000 + b"needle" + b"y" * 19_994                           # 40 000 bytes
    assert term_fuzzy(b"needle", term, 255) == (False, 40_000 - 6)             # the length filter decides; the distance stays exact
    assert term_fuzzy(b"needle", term, 40_000) == (True, 40_000 - 6) and term_fuzzy(b"needle", term, 39_993) == (False, 39_994)
    assert term_fuzzy(b"", term, 0) == (False, 40_000) and term_fuzzy(b"x" * 64, term, 50_000, prefix=64) == (True, 40_000 - 64)
    assert term_fuzzy(b"y" * 64, term, 50_000, prefix=1) == (False, 40_000 - 64)
    short = b"ab" * 40                                                         # 80 bytes: longer than either word
    for pat in (b"ab" * 16, b"ab" * 32, b"ba" * 32, b"ab" * 8 + b"c"):
        for fl, dp in ((0, levenshtein), (TRANSPOSE, osa)):
            assert term_fuzzy(pat, short, 255, flags=fl) == (True, dp(pat, short)), (pat, fl)


def test_argument_errors():
    assert _raw(0, b"a", 1, 0, 1, b"a", 1, out=False)[0] == -1                 # NULL match
    assert _raw(0, None, 1, 0, 1, b"a", 1) == (-1, 77, 88)                     # NULL pattern of one byte
    assert _raw(0, b"a", 1, 0, 1, None, 1) == (-1, 77, 88)                     # NULL term of one byte
    for flags in (0x02, 0x04, 0x40, 0x7f, 0x100, 0x180, 0x8000, 0xFFFFFFFF, 0x83):      # a flag bit other than the two
        assert _raw(flags, b"a", 1, 0, 1, b"a", 1) == (-1, 77, 88), flags
    for flags in (0, TRANSPOSE, NOCASE, TRANSPOSE | NOCASE):
        assert _raw(flags, b"a", 1, 0, 0, b"a", 1) == (0, 1, 0), flags
        assert _raw(flags, b"ab", 2, 3, 5, b"ab", 2) == (-1, 77, 88), flags              # a prefix above the pattern's length
        assert _raw(flags, b"ab", 2, 2, 0, b"ab", 2) == (0, 1, 0), flags
        assert _raw(flags, b"a" * 65, 65, 0, 1, b"a" * 65, 65) == (-5, 77, 88), flags    # 65 bytes: out of range, 64: fine
        assert _raw(flags, b"a" * 64, 64, 64, 0, b"a" * 64, 64) == (0, 1, 0), flags
    assert _raw(0, None, 0, 0, 0, None, 0) == (0, 1, 0)                        # NULL with length 0 is the empty string
    assert _raw(0, b"ab", 2, 0, 0, b"ba", 2, want_dist=False) == (0, 0, 88)    # dist may be NULL
    with pytest.raises(II2Error) as e:
        term_fuzzy(b"oops", b"oops", 1, prefix=5)
    assert e.value.code == -1
    with pytest.raises(II2Error) as e:
        term_fuzzy(b"o" * 65, b"oops", 1)
    assert e.value.code == -5


def test_the_table_covers_what_it_claims():
    cases = {c.name: c for c in fuzzy_cases.CASES}
    assert len(cases) == len(fuzzy_cases.CASES)
    assert {len(c.dicts) for c in fuzzy_cases.CASES} >= {1, 3, 64}
    assert any(not d for c in fuzzy_cases.CASES for d in c.dicts if len(c.dicts) == 3) and any(c.dicts == [[]] for c in fuzzy_cases.CASES)
    assert any(c.dicts == [[b""]] for c in fuzzy_cases.CASES)
    assert len({len(d) for d in cases["k64-unequal"].dicts}) >= 5
    assert all(len(d) <= 5000 for c in fuzzy_cases.CASES for d in c.dicts) and any(len(d) == 5000 for c in fuzzy_cases.CASES for d in c.dicts)
    # the pattern lengths at the words' edges, a call of patterns <= 32 bytes and one that holds a 33-byte pattern
    assert {len(p) for c in fuzzy_cases.CASES for p in c.patterns} >= {0, 1, 31, 32, 33, 63, 64}
    assert {len(p) for p in cases["lengths-0-1-31-32"].patterns} == {1, 31, 32} and fuzzy_cases.word_bits(cases["lengths-0-1-31-32"]) == 32
    assert 33 in {len(p) for p in cases["lengths-33-63-64"].patterns} and fuzzy_cases.word_bits(cases["lengths-33-63-64"]) == 64
    assert {fuzzy_cases.word_bits(c) for c in fuzzy_cases.CASES} == {0, 32, 64}
    big = cases["16-patterns-of-64-bytes"]
    assert len(big.patterns) == 16 and all(len(p) == 64 for p in big.patterns)
    # the empty term and the empty pattern
    assert any(b"" in d and b"" in c.patterns for c in fuzzy_cases.CASES for d in c.dicts)
    # the length filter: m - d - 1, m - d, m, m + d, m + d + 1 for d = 0, 1, 2 and a d >= m
    lf = cases["length-filter"]
    have = {len(t) for t in lf.dicts[0]}
    for p, d in zip(lf.patterns, lf.dists):
        assert {n for n in (len(p) - d - 1, len(p) - d, len(p), len(p) + d, len(p) + d + 1) if n >= 0} <= have, d
    assert set(lf.dists) >= {0, 1, 2} and any(d >= len(p) for p, d in zip(lf.patterns, lf.dists))
    # terms longer than 64 bytes that match a 64-byte pattern under a large d, and some that do not
    lt = cases["long-terms-large-d"]
    hits = [(p, t) for p, d, pre, fl in zip(lt.patterns, lt.dists, lt.prefixes, lt.flags) for t in lt.dicts[0] if len(t) >= 70 and len(p) == 64 and matches(p, t, d, pre, fl)]
    assert len(hits) >= 3 and 10 in lt.dists
    # single edits and transpositions decide between the flags
    assert osa(b"ca", b"abc") == 3 and levenshtein(b"ca", b"abc") == 3 and osa(b"abcdef", b"badcfe") == 3 and levenshtein(b"abcdef", b"badcfe") > 3
    assert osa(b"abcdef", b"bacdef") == 1 and osa(b"abcdef", b"abcdfe") == 1 and osa(b"abcdef", b"bcadef") == 2 and levenshtein(b"abcdef", b"bacdef") == 2
    tr = cases["transpositions"]
    assert {b"bacdef", b"abcdfe", b"bcadef", b"ca", b"abc"} <= set(tr.dicts[0]) and set(tr.flags) == {0, TRANSPOSE}
    se = cases["single-edits"]
    assert sum(levenshtein(b"kitchens", t) == 1 for t in se.dicts[0]) == 9
    # prefix 0, prefix = the pattern's length, a term shorter than the prefix, a term within distance whose prefix differs
    pr = cases["prefix"]
    assert 0 in pr.prefixes and any(pre == len(p) for p, pre in zip(pr.patterns, pr.prefixes))
    assert any(len(t) < pre and distance(p, t, fl) <= d for p, d, pre, fl in zip(pr.patterns, pr.dists, pr.prefixes, pr.flags) for t in pr.dicts[0])
    assert any(len(t) >= pre and t[:pre] != p[:pre] and distance(p, t, fl) <= d for p, d, pre, fl in zip(pr.patterns, pr.dists, pr.prefixes, pr.flags)
               for t in pr.dicts[0])
    assert {f for c in fuzzy_cases.CASES for f in c.flags} == {0, TRANSPOSE, NOCASE, TRANSPOSE | NOCASE}
    assert any(b"\0" in c.patterns and b"\xff" in c.patterns for c in fuzzy_cases.CASES)
    # long runs across the workgroup edges in the big dictionary, one from its first term, one to its last, a pair without a run
    off, first, end, _, matched, tested = fuzzy_cases.expected_table(cases["ternary-5000"])
    assert max(e - f for f, e in zip(first, end)) == 5000 and sum(e - f >= 300 and f > 0 and e < 5000 for f, e in zip(first, end)) >= 2
    assert 0 in first and 5000 in end and any(f > 0 and e == 5000 for f, e in zip(first, end))
    assert any(a == b for a, b in zip(off, off[1:])) and 2 in cases["ternary-5000"].dists
    assert matched < tested < 16 * 5000
    # the expectation's own arithmetic
    assert levenshtein(b"kitten", b"sitting") == 3 and levenshtein(b"", b"abc") == 3 and osa(b"", b"") == 0
    assert fuzzy_cases.passes(b"abc", b"ab", 1, 2, 0) and not fuzzy_cases.passes(b"abc", b"a", 2, 2, 0) and not fuzzy_cases.passes(b"abc", b"a", 1, 0, 0)


# ---- the layers around the kernel keep in step ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_library_exports_both_calls_and_the_makefile_builds_the_kernel():
    lib = _lib.load()
    assert hasattr(lib, "ii2_dict_fuzzy") and hasattr(lib, "ii2_term_fuzzy")
    mk = _read("inverted_index_2_amd", "csrc", "Makefile")
    assert "build/dict_fuzzy.o" in mk and "fuzzy_device.h" in mk and "match_runs.h" in mk
    assert C.sizeof(_lib.FuzzyStats) == 48
    header = _read("include", "ii2.h")
    for name, value in (("II2_FUZZY_MAX_PATTERN", _lib.II2_FUZZY_MAX_PATTERN), ("II2_FUZZY_MAX_PATTERNS", _lib.II2_FUZZY_MAX_PATTERNS)):
        assert re.search(r"#define\s+%s\s+%du\b" % (name, value), header), name
    assert re.search(r"#define\s+II2_FUZZY_TRANSPOSE\s+0x01u", header) and (_lib.II2_FUZZY_TRANSPOSE, _lib.II2_MATCH_NOCASE) == (TRANSPOSE, NOCASE)
    assert "ii2_fuzzy_stats" in header and "/* 48 bytes */" in header


def test_the_recurrence_and_the_parse_are_defined_once():
    csrc = os.path.join(ROOT, "inverted_index_2_amd", "csrc")
    defined, recurrences = {}, []
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".h", ".hip", ".cpp")):
            src = _read("inverted_index_2_amd", "csrc", f)
            for name in ("fuzzy_parse", "fuzzy_distance", "fuzzy_term", "fuzzy_passes", "fuzzy_peq_build"):
                if re.search(r"\b(?:int|bool|void|uint32_t)\s+%s\s*\(" % name, src):
                    defined.setdefault(name, []).append(f)
            if re.search(r"\+\s*Pv\s*\)\s*\^\s*Pv", src):
                recurrences.append(f)
    assert defined == {n: ["fuzzy_device.h"] for n in ("fuzzy_parse", "fuzzy_distance", "fuzzy_term", "fuzzy_passes", "fuzzy_peq_build")}
    assert recurrences == ["fuzzy_device.h"]
    kernel = _read("inverted_index_2_amd", "csrc", "dict_fuzzy.hip")
    assert '#include "fuzzy_device.h"' in kernel and '#include "match_runs.h"' in kernel
    # the part behind the match word is shared with ii2_dict_match, not copied
    for name in ("k_match_place", "k_match_offsets", "int match_runs_drive("):
        holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".cpp")) and re.search(r"(__global__[^;{]*\b%s\b|^%s)" % (re.escape(name), re.escape(name)),
                                                                                                      _read("inverted_index_2_amd", "csrc", f), re.M)]
        assert holders == ["dict_match.hip"], (name, holders)
    assert "match_runs_tail<2>" in kernel and "match_runs_tail<1>" in _read("inverted_index_2_amd", "csrc", "dict_match.hip")


def test_go_binding_and_host_mirror_declare_the_calls():
    go = _read("bindings", "go", "ii2.go")
    assert "C.ii2_dict_fuzzy(" in go and "func (c *Ctx) DictFuzzy(" in go and "C.ii2_term_fuzzy(" in go and "func TermFuzzy(" in go
    index_go = _read("bindings", "go", "index.go")
    assert "func FuzzySearch(" in index_go and "func FuzzyTerms(" in index_go
    src = _read("inverted_index_2_amd", "host", "host_index.cpp")
    assert "int ii2h_fuzzy_search(" in src and "int ii2h_fuzzy_terms(" in src and "ii2_dict_fuzzy(" in src and "ii2_term_fuzzy(" in src
    host_py = _read("inverted_index_2_amd", "host.py")
    assert "def fuzzy_search(" in host_py and "def fuzzy_terms(" in host_py
