"""Dictionaries and patterns aimed at the seams of the term search (ii2_dict_match / ii2_term_match, csrc/match_device.h), one
table for the CPU test of the matchers and the GPU test of the kernels.

A matcher can go wrong at the empty pattern and the empty term, where the pattern is as long as the term or one byte off, where
a glob has to give bytes back to a `*` it passed, at an escaped wildcard, at the bytes next to the letters under case folding,
and at zero and 0xff bytes.  The kernels can go wrong where a run of matching terms crosses from one workgroup of 256 terms into
the next, starts at a dictionary's first term or ends at its last, and where a pair of (pattern, dictionary) has no term at all.
Every case is (name, dictionaries, patterns, kinds): `dictionaries` are k sorted, duplicate-free lists of bytes, `patterns` a
list of bytes, `kinds` one CONTAINS / SUFFIX / GLOB (| NOCASE) per pattern.

The expectation is computed here in Python alone, never from the library:
  CONTAINS  p in t
  SUFFIX    t.endswith(p)
  GLOB      re.fullmatch of the pattern translated byte by byte (`*` -> `.*`, `?` -> `.`, `\\x` -> x escaped, anything else
            escaped) with re.DOTALL
  NOCASE    folds A-Z to a-z on both sides before any of them
and the runs of a pair are the maximal stretches of consecutive matching term indices.
"""
import random
import re
from typing import List, NamedTuple

from tests.dict_cases import _ternary

CONTAINS, SUFFIX, GLOB, NOCASE = 0, 1, 2, 0x80
KINDS = (CONTAINS, SUFFIX, GLOB)
_FOLD = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))


class Case(NamedTuple):
    name: str
    dicts: List[List[bytes]]
    patterns: List[bytes]
    kinds: List[int]


def glob_regex(pattern):
    """the glob as a compiled bytes regex; None for a pattern that ends in a lone backslash (invalid)"""
    out, i = [], 0
    while i < len(pattern):
        c = pattern[i:i + 1]
        if c == b"\\":
            i += 1
            if i == len(pattern):
                return None
            out.append(re.escape(pattern[i:i + 1]))
        elif c == b"*":
            out.append(b".*")
        elif c == b"?":
            out.append(b".")
        else:
            out.append(re.escape(c))
        i += 1
    return re.compile(b"".join(out), re.DOTALL)


def matcher(kind, pattern):
    """term -> bool for one pattern"""
    nocase, base = bool(kind & NOCASE), kind & ~NOCASE
    if nocase:
        pattern = pattern.translate(_FOLD)
    fold = (lambda t: t.translate(_FOLD)) if nocase else (lambda t: t)
    if base == CONTAINS:
        return lambda t: pattern in fold(t)
    if base == SUFFIX:
        return lambda t: fold(t).endswith(pattern)
    rx = glob_regex(pattern)
    return lambda t: rx.fullmatch(fold(t)) is not None


def runs_of(flags):
    """[(first, end), ...] of the maximal stretches of True in flags"""
    out, start = [], None
    for i, f in enumerate(flags):
        if f and start is None:
            start = i
        if not f and start is not None:
            out.append((start, i))
            start = None
    if start is not None:
        out.append((start, len(flags)))
    return out


_EXPECTED = {}


def expected_table(case):
    """(run_off, run_first, run_end, run_dict, n_matched) as ii2_dict_match lays them out: pair (p, s) is entry p * k + s.
    Computed once per case and shared."""
    if case.name not in _EXPECTED:
        run_off, first, end, which, matched = [0], [], [], [], 0
        for p, kind in zip(case.patterns, case.kinds):
            m = matcher(kind, p)
            for s, d in enumerate(case.dicts):
                flags = [m(t) for t in d]
                matched += sum(flags)
                for a, b in runs_of(flags):
                    first.append(a)
                    end.append(b)
                    which.append(s)
                run_off.append(len(first))
        _EXPECTED[case.name] = (run_off, first, end, which, matched)
    return _EXPECTED[case.name]


def flat(items):
    """(bytes, offsets) of a list of bytes, the bytes padded by one so that the array is never empty."""
    off = [0]
    for t in items:
        off.append(off[-1] + len(t))
    return b"".join(items) + b"\0", off


def _case(name, dicts, patterns, kinds=None):
    """kinds None: every pattern once per kind, plain and folded"""
    dicts = [sorted(set(d)) for d in dicts]
    if kinds is None:
        all_kinds = [k | f for k in KINDS for f in (0, NOCASE)]
        patterns, kinds = [p for p in patterns for _ in all_kinds], [k for _ in patterns for k in all_kinds]
        keep = [(p, k) for p, k in zip(patterns, kinds) if k & ~NOCASE != GLOB or glob_regex(p) is not None]
        patterns, kinds = [p for p, _ in keep], [k for _, k in keep]
    assert len(patterns) == len(kinds) and len(patterns) <= 64, name
    assert all(len(p) <= 64 for p in patterns), name
    return Case(name, dicts, list(patterns), list(kinds))


def build():
    cases = []
    cases.append(_case("empty-dictionary", [[]], [b"", b"a", b"*"]))
    cases.append(_case("empty-term-empty-pattern", [[b"", b"a"]], [b""]))
    cases.append(_case("only-the-empty-term", [[b""]], [b"", b"*", b"?", b"a"]))
    words = [b"timeout", b"connection_timeout", b"timeout_ms", b"timeou", b"imeout", b"xtimeout", b"timeoutx", b"time", b"out"]
    cases.append(_case("equal-longer-shorter", [words], [b"timeout", b"timeoutt", b"ttimeout", b"timeou", b"imeout", b"_timeout", b"timeout_"]))
    short = [b"", b"a", b"b", b"ab", b"ba", b"aa", b"abc"]
    cases.append(_case("stars-and-marks", [short], [b"*", b"**", b"?", b"??", b"?*", b"*?", b"*?*", b"***"]))
    back = [b"abab", b"ababab", b"aab", b"aa", b"aaa", b"aXaYa", b"ab", b"aba", b"abXab", b"a", b""]
    cases.append(_case("backtracking", [back], [b"*ab*ab", b"a*a*a", b"*a?", b"*a", b"a*", b"*b*b*", b"?*?b"],
                       [GLOB] * 7))
    esc = [b"*", b"?", b"\\", b"a*", b"a?", b"a\\", b"a*b", b"a?b", b"a\\b", b"axb", b"ab", b"**", b"\\*", b"n"]
    cases.append(_case("escapes", [esc], [b"\\*", b"\\?", b"\\\\", b"a\\*", b"a\\?b", b"a\\\\b", b"a*b", b"a?b", b"\\a\\*\\b", b"*\\**", b"\\n"],
                       [GLOB] * 11))
    raw = [b"\0", b"\0\0", b"a\0b", b"\xff", b"\xff\xff", b"a\xffb", b"\0\xff", b"\xff\0", b"ab", b"\xfe\xff"]
    cases.append(_case("zero-and-ff-bytes", [raw], [b"\0", b"\xff", b"\0\xff", b"a?b", b"*\xff", b"\0*", b"?\0", b"a\0b"]))
    edge = [b"[", b"@", b"`", b"{", b"A", b"a", b"Z", b"z", b"[a", b"{A", b"@z", b"`Z", b"ERROR", b"error", b"Error", b"eRRoR!", b"\xc9", b"\xe9"]
    cases.append(_case("nocase-neighbours-of-the-letters", [edge], [b"[", b"@", b"`", b"{", b"a", b"Z", b"error", b"ERROR", b"\xc9", b"e*R"]))
    rng = random.Random(11)
    long_pats = [bytes(rng.choice(b"abc") for _ in range(64)) for _ in range(64)]
    long_terms = long_pats[::3] + [p[1:] for p in long_pats[1::5]] + [p + b"a" for p in long_pats[2::7]] + [b"c" + p for p in long_pats[4::9]]
    cases.append(_case("64-patterns-of-64-bytes", [long_terms], long_pats, [KINDS[i % 3] | (NOCASE if i % 5 == 0 else 0) for i in range(64)]))
    # thousands of terms over a 3-letter alphabet with short patterns: matches are dense and runs are long
    big = _ternary(5000, 1)
    cases.append(_case("ternary-5000", [big], [b"a", b"ab", b"abc", b"c", b"", b"bb", b"a*", b"*c", b"a?c*", b"??"]))
    pool = _ternary(900, 3)
    three = [pool[::2], [], pool[:40] + pool[-5:]]
    cases.append(_case("k3-unequal", three, [b"ab", b"c", b"", b"a*b", b"B?c*", b"bca"]))
    many = [[] if s == 17 else rng.sample(pool, rng.choice((1, 2, 5, 33, 200, 640))) for s in range(64)]
    cases.append(_case("k64-unequal", many, [b"abc", b"*a", b"cc", b"b*b*"], [CONTAINS, GLOB, SUFFIX | NOCASE, GLOB]))
    # one kind per pattern, mixed in one call
    cases.append(_case("mixed-kinds", [pool[:300], pool[100:500:3]], [b"ab", b"AB", b"*ca", b"ca", b"?b*", b"\\a*"],
                       [CONTAINS, CONTAINS | NOCASE, GLOB, SUFFIX, GLOB | NOCASE, GLOB]))
    return cases


CASES = build()
