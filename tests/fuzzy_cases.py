"""Dictionaries and patterns aimed at the seams of the typo-tolerant term search (ii2_dict_fuzzy / ii2_term_fuzzy,
csrc/fuzzy_device.h), one table for the CPU test of the matcher and the GPU test of the kernels.

The recurrence keeps a DP column in one 32- or 64-bit word whose bit m - 1 moves the score, so it can go wrong at pattern lengths
0, 1, 31, 32, 33, 63 and 64, at terms longer than the word, and where the carry of its one addition runs into the bits above the
pattern.  The filters in front of it can go wrong at |len(term) - len(pattern)| = d and d + 1, at a prefix as long as the
pattern and at a term shorter than the prefix.  A transposition can go wrong at the first and the last two positions and where two
swaps overlap (optimal string alignment edits no substring twice: `ca` -> `abc` is 3).  The fold touches A-Z only.  The kernels
can go wrong where a run of matching terms crosses from one workgroup of 256 terms into the next, starts at a dictionary's first
term or ends at its last, and where a pair of (pattern, dictionary) has no term at all.
Every case is (name, dictionaries, patterns, dists, prefixes, flags): `dictionaries` are k sorted, duplicate-free lists of bytes,
the other four hold one entry per pattern.

The expectation is computed here in Python alone, never from the library: the two plain DPs below, the prefix rule
(term[:prefix] == pattern[:prefix], so a term shorter than the prefix fails), the fold of A-Z on both sides under NOCASE, and the
runs of a pair as the maximal stretches of consecutive matching term indices (match_cases.runs_of)."""
import random
from typing import List, NamedTuple

from tests.dict_cases import _ternary
from tests.match_cases import _FOLD, flat, runs_of  # noqa: F401

TRANSPOSE, NOCASE = 0x01, 0x80


class Case(NamedTuple):
    name: str
    dicts: List[List[bytes]]
    patterns: List[bytes]
    dists: List[int]
    prefixes: List[int]
    flags: List[int]


def levenshtein(a, b):
    """insert, delete, substitute: 1 each"""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


def osa(a, b):
    """optimal string alignment: as above, and a swap of two adjacent bytes costs 1; no substring is edited twice"""
    rows = [list(range(len(b) + 1))]
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(rows[-1][j] + 1, cur[j - 1] + 1, rows[-1][j - 1] + (a[i - 1] != b[j - 1]))
            if i > 1 and j > 1 and a[i - 1] == b[j - 2] and a[i - 2] == b[j - 1]:
                cur[j] = min(cur[j], rows[-2][j - 2] + 1)
        rows = rows[-1:] + [cur]
    return rows[-1][len(b)]


_DIST = {}


def distance(pattern, term, flags):
    """the exact distance under flags"""
    key = (pattern, term, flags)
    if key not in _DIST:
        a, b = (pattern.translate(_FOLD), term.translate(_FOLD)) if flags & NOCASE else (pattern, term)
        _DIST[key] = (osa if flags & TRANSPOSE else levenshtein)(a, b)
    return _DIST[key]


def passes(pattern, term, dist, prefix, flags):
    """the pair passes the length and prefix filter (what ii2_fuzzy_stats.n_tested counts)"""
    a, b = (pattern.translate(_FOLD), term.translate(_FOLD)) if flags & NOCASE else (pattern, term)
    return abs(len(a) - len(b)) <= dist and a[:prefix] == b[:prefix] and len(b) >= prefix


def matches(pattern, term, dist, prefix, flags):
    return passes(pattern, term, dist, prefix, flags) and distance(pattern, term, flags) <= dist


_EXPECTED = {}


def expected_table(case):
    """(run_off, run_first, run_end, run_dict, n_matched, n_tested) as ii2_dict_fuzzy lays them out: pair (p, s) is entry
    p * k + s.  Computed once per case and shared."""
    if case.name not in _EXPECTED:
        run_off, first, end, which, matched, tested = [0], [], [], [], 0, 0
        for pat, d, pre, fl in zip(case.patterns, case.dists, case.prefixes, case.flags):
            for s, terms in enumerate(case.dicts):
                ok = [passes(pat, t, d, pre, fl) for t in terms]
                hit = [o and distance(pat, t, fl) <= d for o, t in zip(ok, terms)]
                tested += sum(ok)
                matched += sum(hit)
                for a, b in runs_of(hit):
                    first.append(a)
                    end.append(b)
                    which.append(s)
                run_off.append(len(first))
        _EXPECTED[case.name] = (run_off, first, end, which, matched, tested)
    return _EXPECTED[case.name]


def word_bits(case):
    """the kernel instance a call of the case's patterns takes by default (0: nothing is launched)"""
    if not case.patterns or not any(case.dicts):
        return 0
    return 32 if max(len(p) for p in case.patterns) <= 32 else 64


def _case(name, dicts, patterns, dists, prefixes=0, flags=0):
    """dists / prefixes / flags: one value for all the patterns or one per pattern"""
    dicts = [sorted(set(d)) for d in dicts]
    patterns = list(patterns)
    spread = lambda v: [v] * len(patterns) if isinstance(v, int) else list(v)
    dists, prefixes, flags = spread(dists), spread(prefixes), spread(flags)
    assert len(patterns) == len(dists) == len(prefixes) == len(flags) and len(patterns) <= 16, name
    assert all(len(p) <= 64 and pre <= len(p) and 0 <= d <= 255 for p, pre, d in zip(patterns, prefixes, dists)), name
    return Case(name, dicts, patterns, dists, prefixes, flags)


def _cross(patterns, dists, flags=(0,)):
    """every pattern with every distance and every flag: (patterns, dists, flags)"""
    trip = [(p, d, f) for p in patterns for d in dists for f in flags]
    return [p for p, _, _ in trip], [d for _, d, _ in trip], [f for _, _, f in trip]


def _edits(rng, word, n, alphabet):
    """n random single edits of word"""
    w = bytearray(word)
    for _ in range(n):
        kind, at = rng.choice("ids"), rng.randrange(len(w) + 1)
        if kind == "i":
            w.insert(at, rng.choice(alphabet))
        elif w and kind == "d":
            del w[min(at, len(w) - 1)]
        elif w:
            w[min(at, len(w) - 1)] = rng.choice(alphabet)
    return bytes(w)


def build():
    cases = []
    rng = random.Random(23)
    cases.append(_case("empty-dictionary", [[]], [b"", b"a", b"abc"], [0, 1, 2]))
    cases.append(_case("only-the-empty-term", [[b""]], [b"", b"", b"a", b"a", b"ab", b"ab"], [0, 3, 0, 1, 1, 2]))
    cases.append(_case("empty-pattern", [[b"", b"a", b"ab", b"abc", b"abcd", b"b"]], [b""] * 5, [0, 1, 2, 3, 255]))
    # the word's top bit is the score bit: pattern lengths 1, 31, 32 in one call (the 32-bit instance) ...
    abc = b"abc"
    base = {m: bytes(rng.choice(abc) for _ in range(m)) for m in (1, 31, 32, 33, 63, 64)}
    near = lambda m: [base[m]] + [_edits(rng, base[m], e, abc) for e in (1, 1, 1, 2, 2, 3, 4)] + [base[m][1:], base[m][:-1], b"c" + base[m], base[m] + b"c"]
    narrow = [t for m in (1, 31, 32) for t in near(m)] + [b"", b"a", b"b"]
    p, d, f = _cross([base[1], base[31], base[32], b""], (0, 1, 2), (0, TRANSPOSE))
    cases.append(_case("lengths-0-1-31-32", [narrow], p[:16], d[:16], 0, f[:16]))
    cases.append(_case("lengths-31-32-and-empty", [narrow], p[8:], d[8:], 0, f[8:]))
    # ... and one call that holds a 33-byte pattern (the 64-bit instance), with 63 and 64
    wide = [t for m in (1, 32, 33, 63, 64) for t in near(m)] + [b""]
    p, d, f = _cross([base[33], base[63], base[64], base[1], base[32]], (0, 2, 3))
    cases.append(_case("lengths-33-63-64", [wide], p, d, 0, [TRANSPOSE if i % 2 else 0 for i in range(len(p))]))
    # the length filter: terms of length m - d - 1, m - d, m, m + d, m + d + 1 for d = 0, 1, 2 and a d >= m
    m5 = b"abcab"
    lens = sorted({m5[:n] for n in range(0, 6)} | {m5 + b"cabcabc"[:n] for n in range(0, 8)} | {b"", b"c" * 12, b"b" * 11, b"a" * 13})
    cases.append(_case("length-filter", [lens], [m5] * 6, [0, 1, 2, 5, 6, 7]))
    # terms longer than the word under a large d
    long64 = base[64]
    longer = [long64 + b"abcabc", b"abc" + long64 + b"abc", long64[:30] + b"cccccc" + long64[30:], _edits(rng, long64 + b"bbbbbb", 4, abc),
              _edits(rng, long64 + b"bbbbbb", 5, abc), long64 + b"a" * 10, long64 + b"a" * 11, long64, bytes(rng.choice(abc) for _ in range(70))]
    assert sum(len(t) >= 70 for t in longer) >= 5
    cases.append(_case("long-terms-large-d", [longer], [long64, long64, long64, base[32], base[32]], [10, 6, 9, 40, 38], 0, [0, TRANSPOSE, 0, 0, TRANSPOSE]))
    # one insert, delete, substitute at the first, a middle and the last position
    w = b"kitchens"
    single = [b"xkitchens", b"kitxchens", b"kitchensx", b"itchens", b"kithens", b"kitchen", b"xitchens", b"kitxhens", b"kitchenx", w, b"xitchenx", b"ktichens"]
    p, d, f = _cross([w], (0, 1, 2), (0, TRANSPOSE))
    cases.append(_case("single-edits", [single], p, d, 0, f))
    # transpositions at positions 0-1 and at the last two; two overlapping swaps; ca / abc; the same inputs without the flag
    swaps = [b"abcdef", b"bacdef", b"abcdfe", b"acbdef", b"bcadef", b"badcfe", b"ca", b"abc", b"ac", b"acb", b"cab", b"bac", b"ba", b"ab"]
    p, d, f = _cross([b"abcdef", b"ca", b"abc", b"ab"], (1, 2), (TRANSPOSE, 0))
    cases.append(_case("transpositions", [swaps], p, d, 0, f))
    # prefix 0, prefix = the pattern's length, a term shorter than the prefix, a term within distance whose prefix differs
    pre_terms = [b"search", b"serach", b"xearch", b"sxarch", b"sea", b"se", b"s", b"", b"searches", b"searc", b"seerch", b"Search", b"SEARCH"]
    cases.append(_case("prefix", [pre_terms], [b"search"] * 8, [2, 2, 2, 2, 6, 6, 1, 2], [0, 1, 2, 6, 3, 6, 2, 2], [0, 0, 0, 0, 0, 0, TRANSPOSE, NOCASE]))
    # the bytes next to the letters under the fold, and two bytes beyond ASCII that differ by 32
    edge = [b"[", b"@", b"`", b"{", b"A", b"a", b"Z", b"z", b"[a", b"{A", b"@z", b"`Z", b"ERROR", b"error", b"Error", b"eRRoR!", b"\xc9", b"\xe9", b"\xc9a", b"\xe9A"]
    p, d, f = _cross([b"[", b"@", b"`", b"{", b"error", b"ERROR", b"\xc9A", b"Z"], (0, 1), (NOCASE,))
    cases.append(_case("nocase-neighbours-of-the-letters", [edge], p, d, [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 5, 5, 1, 2, 0, 0], f))
    p, d, f = _cross([b"[", b"@", b"error", b"\xc9A"], (0, 1), (0, NOCASE | TRANSPOSE))
    cases.append(_case("nocase-against-plain", [edge], p, d, 0, f))
    # the table's first and last entry
    raw = [b"\0", b"\0\0", b"a\0b", b"\xff", b"\xff\xff", b"a\xffb", b"\0\xff", b"\xff\0", b"ab", b"\xfe\xff", b"\0\xff\0", b"\1\xfe"]
    p, d, f = _cross([b"\0", b"\xff", b"\0\xff", b"a\0b"], (0, 1), (0, TRANSPOSE))
    cases.append(_case("zero-and-ff-bytes", [raw], p, d, [0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 2, 2, 0, 1, 2, 3], f))
    # 16 patterns of 64 bytes over a 3-letter alphabet
    long_pats = [bytes(rng.choice(abc) for _ in range(64)) for _ in range(16)]
    long_terms = long_pats[::3] + [q[1:] for q in long_pats[1::4]] + [q + b"a" for q in long_pats[2::5]] + [_edits(rng, q, e, abc) for q in long_pats for e in (1, 3, 5)]
    cases.append(_case("16-patterns-of-64-bytes", [long_terms], long_pats, [i % 5 for i in range(16)], [0, 64, 1, 0] * 4,
                       [(TRANSPOSE if i % 2 else 0) | (NOCASE if i % 3 == 0 else 0) for i in range(16)]))
    # thousands of terms over a 3-letter alphabet: short patterns with d = 2, and distances that make the runs long - every term
    # (a run from the dictionary's first term to its last, across every workgroup edge), every term behind one first byte
    big = _ternary(5000, 1)
    cases.append(_case("ternary-5000", [big],
                       [b"abc", b"aaa", b"abcabca", b"cabbacab", b"", b"", b"abc", b"bcabcabc", b"c", b"ab", b"zzzzzzzz", b"abcabcabc", b"aabbccaabbcc", b"acb", b"BCA", b"a"],
                       [2, 2, 2, 2, 3, 12, 12, 12, 12, 11, 2, 4, 5, 2, 2, 9],
                       [0, 0, 0, 2, 0, 0, 0, 1, 1, 2, 0, 3, 0, 1, 0, 1],
                       [0, TRANSPOSE, 0, TRANSPOSE, 0, 0, TRANSPOSE, 0, 0, 0, 0, TRANSPOSE, 0, TRANSPOSE, NOCASE, 0]))
    pool = _ternary(900, 3)
    three = [pool[::2], [], pool[:40] + pool[-5:]]
    cases.append(_case("k3-unequal", three, [b"abc", b"", b"cabcab", b"bbb", b"abcabcabcabc", b"c"], [1, 3, 2, 2, 3, 12], [0, 0, 1, 0, 2, 1],
                       [0, 0, TRANSPOSE, 0, 0, 0]))
    many = [[] if s == 17 else rng.sample(pool, rng.choice((1, 2, 5, 33, 200, 640))) for s in range(64)]
    cases.append(_case("k64-unequal", many, [b"abcabc", b"ccc", b"b", b"bcbcbcbcb"], [2, 1, 12, 3], [0, 0, 1, 0], [0, TRANSPOSE, 0, NOCASE]))
    return cases


CASES = build()
