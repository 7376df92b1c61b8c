"""Dictionaries and patterns aimed at the seams of the regular-expression term search (ii2_dict_regex / ii2_term_regex,
csrc/regex_device.h), one table for the CPU test of the matcher and the GPU test of the kernel.

The matcher keeps the states of a Glushkov position automaton in one 64-bit word, so it can go wrong at patterns of 1, 31, 32,
33, 63 and 64 positions (the shift across bit 31 -> 32, bit 63 as an accepting state whose shift falls off), where a follow set
is more than "the next position" (loops backwards, nested nullable stars, empty alternatives, the expansion of counted
repetitions, every position in the follow loop at once), at the empty term and the empty pattern, at the length filter's two
ends, in the byte classes (0x00, 0xff, negation, the escapes, `]` and `-` as literals) and in the fold (only ASCII letters).
The kernel can go wrong where a run of matching terms crosses from one workgroup of 256 terms into the next, starts at a
dictionary's first term or ends at its last, where a pair of (pattern, dictionary) has no term at all, and with the largest call's
tables in LDS.  Every case is (name, dictionaries, patterns, flags): `dictionaries` are k sorted, duplicate-free lists of bytes,
`flags` holds one entry per pattern.

The expectation is Python's `re` alone, never the library: the pattern compiled with re.DOTALL (and re.IGNORECASE under NOCASE),
fullmatch on bytes; the length filter from the parser's own width of the pattern; the runs of a pair as the maximal stretches of
consecutive matching term indices (match_cases.runs_of)."""
import itertools
import random
import re
import warnings
from typing import List, NamedTuple

try:
    from re import _parser as _sre_parse
except ImportError:                                 # before Python 3.11
    import sre_parse as _sre_parse

from tests.dict_cases import _ternary
from tests.match_cases import flat, runs_of  # noqa: F401

NOCASE = 0x80
MAX_PATTERN, MAX_POSITIONS, MAX_PATTERNS = 256, 64, 8


class Case(NamedTuple):
    name: str
    dicts: List[List[bytes]]
    patterns: List[bytes]
    flags: List[int]


_RX, _WIDTH = {}, {}


def compiled(pattern, flags):
    key = (pattern, flags)
    if key not in _RX:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _RX[key] = re.compile(pattern, re.DOTALL | (re.IGNORECASE if flags & NOCASE else 0))
    return _RX[key]


def matches(pattern, term, flags):
    return compiled(pattern, flags).fullmatch(term) is not None


def width(pattern):
    """(shortest, longest) term of the pattern's language as Python's parser computes it; longest None: unbounded"""
    if pattern not in _WIDTH:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            lo, hi = _sre_parse.parse(pattern, re.DOTALL).getwidth()
        _WIDTH[pattern] = (int(lo), None if hi >= 1 << 31 else int(hi))
    return _WIDTH[pattern]


def passes(pattern, term):
    """the pair passes the length filter (what ii2_regex_stats.n_tested counts)"""
    lo, hi = width(pattern)
    return lo <= len(term) and (hi is None or len(term) <= hi)


_EXPECTED = {}


def expected_table(case):
    """(run_off, run_first, run_end, run_dict, n_matched, n_tested) as ii2_dict_regex lays them out: pair (p, s) is entry
    p * k + s.  Computed once per case and shared."""
    if case.name not in _EXPECTED:
        run_off, first, end, which, matched, tested = [0], [], [], [], 0, 0
        for pat, fl in zip(case.patterns, case.flags):
            rx = compiled(pat, fl)
            for s, terms in enumerate(case.dicts):
                hit = [rx.fullmatch(t) is not None for t in terms]
                tested += sum(passes(pat, t) for t in terms)
                matched += sum(hit)
                for a, b in runs_of(hit):
                    first.append(a)
                    end.append(b)
                    which.append(s)
                run_off.append(len(first))
        _EXPECTED[case.name] = (run_off, first, end, which, matched, tested)
    return _EXPECTED[case.name]


def _case(name, dicts, patterns, flags=0):
    """flags: one value for all the patterns or one per pattern"""
    dicts = [sorted(set(d)) for d in dicts]
    patterns = list(patterns)
    flags = [flags] * len(patterns) if isinstance(flags, int) else list(flags)
    assert len(patterns) == len(flags) and len(patterns) <= MAX_PATTERNS and all(len(p) <= MAX_PATTERN for p in patterns), name
    return Case(name, dicts, patterns, flags)


def _all(alphabet, upto):
    """every string over the alphabet of length 0 .. upto"""
    return [bytes(s) for n in range(upto + 1) for s in itertools.product(alphabet, repeat=n)]


def chain(n):
    """a literal pattern of n positions"""
    return bytes(b"abc"[i % 3] for i in range(n))


# ---- the positions of the patterns at the word's edges, pinned by hand (ii2_term_regex reports them) ----
LAST_LOOPS = b"a{63}b*"                                         # 64 positions, the last one follows itself
EVERY_LOOPS = b"a*" * 64                                        # 64 positions, none of them advances by the shift alone
HALF_LOOPS = b"a*b*" * 32
CALL_OF_64 = [b"[abc]{0,64}", b"[ab]{0,64}", b"a[abc]{0,63}", b"[abc]{0,63}c", b"([ab]{0,31}c)?[abc]{0,32}", b"[abc]{0,32}b[abc]{0,31}",
              b"(ab|c){0,21}a?", b".{0,64}"]
N_POS = {chain(1): 1, chain(31): 31, chain(32): 32, chain(33): 33, chain(63): 63, chain(64): 64, b"[ab]{64}": 64, LAST_LOOPS: 64,
         EVERY_LOOPS: 64, HALF_LOOPS: 64, b"": 0, b"()": 0, b"a|": 1, b"(a|)b": 2, b"(ab)*": 2, b"(a|bc)+d": 4, b"(a*b*)*": 2,
         b"x{0}": 0, b"x{2}": 2, b"x{2,4}": 4, b"x{3,}": 4, b"x{0,1}": 1, b"[ab]{2,4}": 4, b"(ab|c){2,4}": 12, b"(ab|c){3,}": 12,
         b"(ab|c){0}": 0, b"[ab]{60,}": 61, b"\\d\\w\\s.": 4, b"(?:a|b)c": 3}
N_POS.update({p: 64 for p in CALL_OF_64})

# ---- the length filter's patterns with the widths they must have, pinned by hand ----
WIDTHS = {b"ab{2,4}c": (4, 6), b"[a-c]{3}": (3, 3), b"a?b?c?": (0, 3), b"ab+": (2, None), b".{5}": (5, 5), b"(abc|a)": (1, 3),
          b"(a{0})*": (0, 0), b"(ab|c){2,}": (2, None)}

# ---- patterns that must not parse: II2_EINVAL, one form each ----
INVALID = [b"\\q", b"\\a", b"\\b", b"\\A", b"\\Z", b"\\1", b"\\0", b"\\ ", b"\\", b"a\\", b"\\x4", b"\\xg0", b"\\x", b"[\\q]", b"[a\\",
           b"[b-a]", b"[\\xff-\\x00]", b"[abc", b"[", b"[]", b"[^]", b"[^", b"[a-", b"[\\d-z]", b"[a-\\d]", b"[a-\\W]",
           b"(?=a)", b"(?!a)", b"(?P<n>a)", b"(?i)a", b"(?", b"(?#c)", b"(a", b"a)", b")", b"((a)", b"(a))", b"(",
           b"a**", b"a*+", b"a++", b"a+*", b"a?*", b"a???", b"a*??", b"a{2}{3}", b"a{2}*", b"a*{2}", b"a{2}?{3}", b"a{2}??",
           b"*a", b"+", b"?", b"{2}", b"(*a)", b"|*", b"a|+", b"(|?)",
           b"a{,3}", b"a{3,2}", b"a{", b"a{x}", b"a{2", b"a{2,", b"a{2,x}", b"a{}", b"a{ 2}", b"a{2, 3}", b"{",
           b"^a", b"a$", b"(^a)", b"a|$", b"^", b"$"]
# ... and the limits at limit + 1, II2_ERANGE, with the positions ii2_term_regex reports; their neighbours at the limit parse
TOO_MANY_POSITIONS = [(b"a{65}", 65), (chain(65), 65), (b"[ab]{64}c", 65), (b"(abc){22}", 66), (b"a{64,}", 65), (b"(a{9}){8}", 72), (b"a{1000}", 1000)]
AT_THE_POSITION_LIMIT = [b"a{64}", chain(64), b"[ab]{63}c", b"(abc){21}a", b"a{63,}", b"(a{8}){8}", b"a{0,64}"]
TOO_LONG = b"a" + b"|" * 256                                    # 257 raw bytes, one position
AT_THE_LENGTH_LIMIT = b"a" + b"|" * 255


def build():
    cases = []
    rng = random.Random(29)
    # ---- the empty cases ----
    nullable = [b"", b"a*", b"a", b"()", b"a|", b".*", b"a?b?", b"x{0}"]
    cases.append(_case("empty-dictionary", [[]], nullable))
    cases.append(_case("only-the-empty-term", [[b""]], nullable))
    cases.append(_case("empty-pattern", [[b"", b"a", b"ab", b"\n", b"\0"]], [b"", b"()", b"(|)", b"(?:)", b"a{0}", b"(a{0}){3}", b"()*", b"(){2,}"]))
    # ---- the word: 1, 31, 32, 33, 63, 64 positions, terms that end in the last position ----
    sizes = (1, 31, 32, 33, 63, 64)
    ends = [t for n in sizes for t in (chain(n), chain(n)[:-1], chain(n) + b"a", chain(n)[:-1] + b"x", b"x" + chain(n)[1:])]
    ends += [b"a" * 63, b"a" * 63 + b"b", b"a" * 63 + b"bbb", b"a" * 62 + b"b", b"a" * 64, b"a" * 62, b"ab" * 32, b"ab" * 31 + b"a", b"ab" * 32 + b"a",
             b"ab" * 31 + b"ac", b"b" * 64, b""]
    cases.append(_case("word-edges", [ends], [chain(n) for n in sizes] + [b"[ab]{64}", LAST_LOOPS]))
    cases.append(_case("word-edges-nocase", [ends + [t.upper() for t in ends]], [chain(n).upper() if n % 2 else chain(n) for n in sizes] + [b"[aB]{64}", LAST_LOOPS],
                       NOCASE))
    # ---- the follow loop ----
    small = _all(b"abcd", 4) + [b"ab" * 3, b"ab" * 4, b"bcbcad", b"abcabcd", b"bcad", b"aabbab", b"bbaaba"]
    cases.append(_case("loops-backwards", [small], [b"(ab)*", b"(a|bc)+d", b"(a*b*)*", b"(a|)b", b"a|", b"()", b"(a|b|)(c|d)?", b"((a|b)*c)*d?"]))
    cases.append(_case("loops-and-groups", [small], [b"(?:a|b)c", b"(a(b(c)?)?)?", b"(a|ab)(c|bcd)", b"a*a", b"(a*)*b", b"(a+)+", b"(a?)*d", b"(|a)(|b)(|c)"]))
    counted = _all(b"abx", 5) + [b"ab" * 4, b"ab" * 5, b"abcabc", b"ccc", b"cc", b"cabc", b"ababc", b"abcabcab", b"c" * 5, b"x" * 6, b"x" * 7, b"abab", b"cabab",
                                 b"ababab"]
    cases.append(_case("counted-byte-and-class", [counted], [b"x{0}", b"x{2}", b"x{2,4}", b"x{3,}", b"x{0,1}", b"[ab]{2,4}", b"[ab]{3,}", b"[ab]{0}x"]))
    cases.append(_case("counted-group", [counted], [b"(ab|c){2,4}", b"(ab|c){3,}", b"(ab|c){0}", b"(ab|c){2}", b"(ab|c){0,1}", b"(a{2}b){1,2}", b"(x{1,2}){2}", b"(a|b{2,3}){2}x{0,2}"]))
    cases.append(_case("lazy", [counted], [b"a+?b", b"a{1,2}?", b"(ab)??", b".*?x", b"x{2,}?", b"x??a", b"(a|b)*?x+?", b"a{2}?b"]))
    # (the terms that do not match fail Python's backtracking matcher early: a byte outside the pattern in front, or a short term)
    runs_ab = [b"a" * n for n in range(0, 71)] + [b"ab" * n for n in range(1, 33)] + [b"aab", b"ba", b"abba", b"c", b"ac", b"aac", b"aaac", b"ca", b"abc", b"b" * 64,
                                                                                       b"c" + b"a" * 69, b"c" + b"ab" * 32, b"bbaa", b"abab" + b"b" * 60]
    cases.append(_case("every-position-in-the-loop", [runs_ab], [EVERY_LOOPS, HALF_LOOPS, b".*" * 64, b"(a*b*)*" * 8]))
    # ---- the length filter ----
    lens = _all(b"abc", 4) + [b"abbbc", b"abbbbc", b"abbbbbc", b"abbbbbbc", b"abcab", b"abcabc", b"aaaaa", b"ab" * 3, b"ccccc", b"cccccc", b"abbbbbbbb"]
    cases.append(_case("length-filter", [lens], list(WIDTHS)))
    # ---- classes ----
    singles = [bytes([c]) for c in range(256)]
    pairs = [b"\0\0", b"\xff\xff", b"a\n", b"\n\n", b"a-", b"-a", b"a]", b"]]", b"()", b"+?", b"{}", b"}}", b"^$", b"a\nb", b"a\0b", b"a\xffb", b"ab", b"\0\xff", b"1a ", b"1_\t",
             b"9Z\n", b" 1a", b"1a x"]
    cl = singles + pairs
    cases.append(_case("zero-and-ff", [cl], [b"\\x00", b"\\xff", b"\0", b"\xff", b"[\\x00-\\x10]", b"[\\xf0-\\xff]", b"[^\\x00]", b"[^\\xff]"]))
    cases.append(_case("zero-and-ff-raw-ranges", [cl], [b"[\0-\x01]", b"[\xfe-\xff]", b"[^\0-\xfe]", b"[^\x01-\xff]", b"[\0\xff]+", b"a[\0\xff]b", b".", b"a.b"]))
    cases.append(_case("escapes", [cl], [b"\\d", b"\\D", b"\\w", b"\\W", b"\\s", b"\\S", b"\\d\\w\\s.", b"\\n|\\r|\\t|\\f|\\v"]))
    cases.append(_case("escapes-in-classes", [cl], [b"[\\d\\s]", b"[^\\w]", b"[\\Wa]", b"[\\D]", b"[^\\S\\d]", b"[\\n\\x41-\\x43\\]]", b"[^\\D5]", b"[\\w-]"]))
    cases.append(_case("brackets-and-dashes", [cl], [b"[]a]", b"[a-]", b"[^]]", b"[-a]", b"[a\\]]", b"[^]a-]", b"[]-a]", b"[a-c-e]"]))
    cases.append(_case("escaped-metacharacters", [cl], [b"\\.", b"\\*|\\\\", b"\\[|\\]", b"\\(\\)", b"\\+\\?", b"\\{\\}", b"\\^\\$", b"[.]|[*+?]|[$^]|[(|)]"]))
    cases.append(_case("literal-brace-and-bracket", [cl], [b"]", b"}", b"a]", b"]]", b"}{2}", b"\\x41", b"\\x7a|\\x5A", b"[\\x30-\\x39]a "]))
    # ---- NOCASE: the bytes next to the letters, two bytes beyond ASCII that differ by 32, the same inputs without the flag ----
    edge = [b"@", b"[", b"`", b"{", b"A", b"a", b"Z", b"z", b"\\", b"]", b"^", b"_", b"\xc9", b"\xe9", b"Az", b"aZ", b"ERROR", b"error", b"Error", b"eRRoR", b"@[", b"`{", b"",
            b"\xc9\xe9", b"M", b"m"]
    fold_pats = [b"[Z-a]", b"[^a]", b"@|\\[|`|\\{", b"error", b"\\xc9|[\\xe9]{2}", b"[A-Z]+", b"[^A-Z]+", b"[^@-\\[]|\\x4d"]
    cases.append(_case("nocase-neighbours-of-the-letters", [edge], fold_pats, NOCASE))
    cases.append(_case("nocase-against-plain", [edge], fold_pats, 0))
    cases.append(_case("nocase-mixed", [edge], [b"ERROR", b"ERROR", b"[^\\W_]", b"[^\\W_]", b"\\x61z", b"\\x61z", b"[a-z][^a-z]", b"[a-z][^a-z]"], [0, NOCASE] * 4))
    # ---- terms longer than the word ----
    long_terms = [b"ab" * 40, b"ab" * 40 + b"a", b"a" + b"b" * 100 + b"z", b"a" + b"b" * 100, b"b" * 59, b"b" * 60, b"b" * 61, b"ab" * 50, b"c" * 80, b"ab" * 32 + b"c" + b"ba" * 20,
                  b"a" * 65 + b"z", bytes(rng.choice(b"ab") for _ in range(90)), bytes(rng.choice(b"abc") for _ in range(200)), b"z" * 66]
    assert sum(len(t) > 64 for t in long_terms) >= 10
    cases.append(_case("long-terms", [long_terms], [b"(ab)*", b"a.*z", b"[ab]{60,}", b".*c.*", b"(ab)*a?", b"[^c]{62,}", b".{63}.+", b"(a|b)*c(a|b)*"]))
    # ---- thousands of terms: runs across every workgroup edge, from the first term, to the last, none ----
    big = _ternary(5000, 1)
    cases.append(_case("ternary-5000", [big], [b".*", b"a.*", b"c.*", b"(|a.*)", b"d+", b"[abc]{13,}", b".*abc.*", b"(a|b)*c{2}(a|b|c){0,3}"]))
    cases.append(_case("ternary-5000-8-patterns-of-64-positions", [big], CALL_OF_64))
    pool = _ternary(900, 3)
    three = [pool[::2], [], pool[:40] + pool[-5:]]
    cases.append(_case("k3-unequal", three, [b".*", b"", b"(ab|c)+", b"b.*b", b"[ab]{3,8}", b"ca?b?.*", b"z", b"(a|b|c){7}"]))
    many = [[] if s == 17 else rng.sample(pool, rng.choice((1, 2, 5, 33, 200, 640))) for s in range(64)]
    cases.append(_case("k64-unequal", many, [b".*", b"[ab]*c[ab]*", b"B.*", b"(abc|cba|b)+"], [0, 0, NOCASE, 0]))
    return cases


CASES = build()
