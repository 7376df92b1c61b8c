"""Dictionaries and patterns aimed at the seams of II2_MATCH_UTF8 (csrc/utf8_device.h and its users in fuzzy_device.h and
match_device.h), one table for the CPU test of the matchers and the GPU test of the kernels.

Under the flag a byte string is a sequence of symbols: a well-formed UTF-8 sequence is its code point, any other byte b alone is
0xDC00 + b.  The decoder can go wrong where the width changes (U+007F / 0080, 07FF / 0800, FFFF / 10000), at the bounds of the
second byte (overlong forms, the surrogates, above U+10FFFF), and at a sequence the term's end cuts off - in the kernels' LDS
stage the next term's bytes lie right behind, so a decoder that reads on sees a sequence that is not there.  The fuzzy search can
go wrong where symbols and bytes count differently (length filter, prefix, distance, the choice of the 32- or 64-bit instance) and
in the hashed lookup of the symbols above 0x7f (collisions, a miss that probes occupied slots).  The glob can go wrong where `?`
or a `*` that gives back takes a byte instead of a symbol.  The kernels can go wrong at a workgroup's edge of 256 terms.

The expectation is computed here in Python alone, never from the library: the greedy decoder below (asserted equal to
bytes.decode("utf-8", "surrogateescape") on every string of the table by tests/test_utf8_cpu.py), the two plain DPs of
tests/fuzzy_cases.py run on lists of ints, a small symbol-wise glob, and match_cases.runs_of.  A pattern without the flag keeps the
byte rule of fuzzy_cases / match_cases."""
from typing import List, NamedTuple

from tests import fuzzy_cases, match_cases
from tests.fuzzy_cases import NOCASE, TRANSPOSE, levenshtein, osa
from tests.match_cases import _FOLD, CONTAINS, GLOB, SUFFIX, runs_of

UTF8 = 0x08


def decode(b):
    """the symbols of b: greedy, left to right"""
    out, i, n = [], 0, len(b)
    while i < n:
        b0 = b[i]
        width, cp = 1, 0xDC00 + b0
        if b0 < 0x80:
            cp = b0
        elif 0xC2 <= b0 <= 0xF4:
            need = 2 if b0 < 0xE0 else 3 if b0 < 0xF0 else 4
            lo = 0xA0 if b0 == 0xE0 else 0x90 if b0 == 0xF0 else 0x80
            hi = 0x9F if b0 == 0xED else 0x8F if b0 == 0xF4 else 0xBF
            if i + need <= n and lo <= b[i + 1] <= hi and all(0x80 <= c <= 0xBF for c in b[i + 2:i + need]):
                cp = b0 & (0x7F >> need)
                for c in b[i + 1:i + need]:
                    cp = (cp << 6) | (c & 0x3F)
                width = need
        out.append(cp)
        i += width
    return out


def surrogateescape(b):
    return [ord(c) for c in b.decode("utf-8", "surrogateescape")]


def well_formed(b):
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def u(*code_points):
    return "".join(chr(c) for c in code_points).encode("utf-8")


# ---- fuzzy ----
def _seq(b, flags):
    b = b.translate(_FOLD) if flags & NOCASE else b
    return decode(b) if flags & UTF8 else list(b)


_DIST = {}


def distance(pattern, term, flags):
    key = (pattern, term, flags)
    if key not in _DIST:
        _DIST[key] = (osa if flags & TRANSPOSE else levenshtein)(_seq(pattern, flags), _seq(term, flags))
    return _DIST[key]


def passes(pattern, term, dist, prefix, flags):
    a, b = _seq(pattern, flags), _seq(term, flags)
    return abs(len(a) - len(b)) <= dist and len(b) >= prefix and a[:prefix] == b[:prefix]


def matches(pattern, term, dist, prefix, flags):
    return passes(pattern, term, dist, prefix, flags) and distance(pattern, term, flags) <= dist


_EXPECTED = {}


def expected_fuzzy(case):
    """(run_off, run_first, run_end, run_dict, n_matched, n_tested), laid out as fuzzy_cases.expected_table"""
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


def positions(pattern, flags):
    return len(decode(pattern)) if flags & UTF8 else len(pattern)


def word_bits(case):
    """the kernel instance a call of the case's patterns takes by default (0: nothing is launched)"""
    if not case.patterns or not any(case.dicts):
        return 0
    return 32 if max(positions(p, f) for p, f in zip(case.patterns, case.flags)) <= 32 else 64


def n_utf8(case):
    return sum(bool(f & UTF8) for f in case.flags) if case.patterns and any(case.dicts) else 0


def _fuzzy(name, dicts, patterns, dists, prefixes=0, flags=UTF8):
    dicts = [sorted(set(d)) for d in dicts]
    patterns = list(patterns)
    spread = lambda v: [v] * len(patterns) if isinstance(v, int) else list(v)
    dists, prefixes, flags = spread(dists), spread(prefixes), spread(flags)
    assert len(patterns) == len(dists) == len(prefixes) == len(flags) and len(patterns) <= 16, name
    for p, pre, d, f in zip(patterns, prefixes, dists, flags):
        assert len(p) <= 64 and pre <= positions(p, f) and 0 <= d <= 255 and (not f & UTF8 or well_formed(p)), (name, p)
    assert all(len(d) <= 5000 for d in dicts), name
    return fuzzy_cases.Case(name, dicts, patterns, dists, prefixes, flags)


SEAMS = (0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x10FFFF)
ILL_FORMED = [b"\x80", b"\xbf", b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xe0\x9f\xbf", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf0\x8f\xbf\xbf",
              b"\xf4\x90\x80\x80", b"\xe2\x82", b"\xf0\x9f\x98", b"\xc3", b"\xe2\x28\xa1", b"\xf0\x9f\x28\x80"] + [bytes([c]) for c in range(0xF5, 0x100)]
TRAP = [b"\x8f\xe2\x82", b"\xac"]         # adjacent in the dictionary: the stage holds 8F E2 82 AC


def _near(symbols, spare):
    """a string of symbols and its neighbours: one and two symbols replaced by `spare` ones, one dropped, one added, two swapped"""
    s, n = list(symbols), len(symbols)
    out = [s, s[:n // 2] + [spare[0]] + s[n // 2 + 1:], [spare[1]] + s[1:], s[:-1] + [spare[0]], s[1:], s[:-1], s + [spare[1]], [spare[0]] + s,
           [spare[0]] + s[1:-1] + [spare[1]], s[:3] + [s[4], s[3]] + s[5:], s[2:], s + [spare[0], spare[1]]]
    return [u(*t) for t in out]


def build_fuzzy():
    cases = []
    # every width seam as a pattern symbol and as a term symbol
    singles = [u(c) for c in SEAMS]
    pairs = [u(a, b) for a in SEAMS for b in SEAMS if a != b][::3]
    seam_terms = singles + pairs + [b"a" + s for s in singles] + [s + b"a" for s in singles] + [b"", b"a"]
    cases.append(_fuzzy("width-seams-d0", [seam_terms], singles + [u(0x7F, 0x80), u(0x7FF, 0x800), u(0xFFFF, 0x10000), u(0x10FFFF, 0xD7FF, 0xE000)], 0))
    cases.append(_fuzzy("width-seams-d1", [seam_terms], singles + [u(0x7F, 0x80), u(0x7FF, 0x800), u(0xFFFF, 0x10000), u(0x10FFFF, 0xD7FF, 0xE000)], 1,
                        [0] * 9 + [1, 1, 0, 2]))
    # ill-formed bytes in terms: each is one symbol that no pattern holds
    bad = ILL_FORMED + [b"a" + t for t in ILL_FORMED[:12]] + [t + b"a" for t in ILL_FORMED[:12]] + [u(0x20AC), u(0x1F600), b"a", b"", u(0x20AC) + b"\x82"]
    cases.append(_fuzzy("ill-formed-term-bytes", [bad], [u(0x20AC)] * 4 + [b"a"] * 3 + [b""] * 4 + [u(0x1F600)] * 3 + [u(0x20AC), b"a"],
                        [0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 4, 1, 3, 4, 2, 2], 0, [UTF8] * 14 + [0, 0]))
    # the end-of-term trap: x + EURO SIGN is 3 symbols and 2 bytes away from 8F E2 82; reading on into AC makes it 1
    trap_terms = TRAP + [b"x" + u(0x20AC), b"x", b"a", u(0x20AC), b"\x8f"]
    assert sorted(trap_terms)[sorted(trap_terms).index(TRAP[0]) + 1] == TRAP[1]
    cases.append(_fuzzy("end-of-term-trap", [trap_terms], [b"x" + u(0x20AC)] * 5 + [u(0x20AC)] * 2, [1, 2, 3, 1, 2, 1, 2], 0, [UTF8, UTF8, UTF8, 0, 0, UTF8, UTF8]))
    # the same bytes under both rules in ONE call
    both = ["cafe", "café", "caffe", "cafés", "日本語", "日本话", "日本", "éà", "àé", "éé", "É", "é", "e", "E", "éa", "èa", "ea", "éb", "a"]
    both = [t.encode("utf-8") for t in both]
    pats = ["café", "café", "日本語", "日本語", "éà", "éà", "É", "É", "É", "É", "éa", "éa"]
    cases.append(_fuzzy("bytes-against-symbols", [both], [p.encode("utf-8") for p in pats], [1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 1, 1], [0] * 10 + [1, 1],
                        [UTF8, 0, UTF8, 0, UTF8 | TRANSPOSE, TRANSPOSE, UTF8 | NOCASE, NOCASE, UTF8 | NOCASE, NOCASE, UTF8, 0]))
    # the word's edge counts symbols: 31 and 32 two-byte symbols (64 bytes) take the 32-bit instance, 33 symbols the 64-bit one
    e, spare = 0xE9, (0xE8, 0x153)
    t31, t32, t33 = [e] * 30 + [0xEA], [e] * 31 + [0xEA], [e] * 31 + [0x61, 0x62]
    edge_terms = _near(t31, spare) + _near(t32, spare) + _near(t33, spare) + [b""]
    cases.append(_fuzzy("31-and-32-two-byte-symbols", [edge_terms], [u(*t31), u(*t32)] * 4, [0, 0, 1, 1, 2, 2, 3, 3], 0,
                        [UTF8, UTF8, UTF8, UTF8, UTF8 | TRANSPOSE, UTF8 | TRANSPOSE, UTF8, UTF8]))
    cases.append(_fuzzy("33-symbols-in-64-bytes", [edge_terms], [u(*t33), u(*t32)] * 3, [0, 0, 1, 1, 2, 2], [0, 0, 0, 0, 33, 32], [UTF8] * 4 + [UTF8 | TRANSPOSE] * 2))
    cjk = [0x4E00 + 7 * i for i in range(21)]
    cases.append(_fuzzy("21-three-byte-symbols", [_near(cjk, (0x3042, 0x4E01)) + [b""]], [u(*cjk)] * 4, [0, 1, 2, 2], [0, 0, 0, 3], [UTF8, UTF8, UTF8 | TRANSPOSE, UTF8]))
    emoji = [0x1F600 + i for i in range(16)]
    cases.append(_fuzzy("16-four-byte-symbols", [_near(emoji, (0x1F680, 0x10000)) + [b""]], [u(*emoji)] * 4, [0, 1, 2, 2], [0, 0, 16, 0],
                        [UTF8, UTF8, UTF8, UTF8 | TRANSPOSE]))
    a64 = [0x61 + (i * 7) % 26 for i in range(64)]
    cases.append(_fuzzy("64-ascii-symbols-flagged", [_near(a64, (0x41, 0x7A)) + [b""]], [u(*a64)] * 4, [0, 1, 2, 2], 0, [UTF8, UTF8 | NOCASE, UTF8 | TRANSPOSE, 0]))
    # the symbol lookup under load: 32 distinct two-byte symbols, and three-byte symbols 64, 256 and 4096 apart (of the last kind
    # only 15 exist: b + 13 * 4096 is a surrogate for every three-byte b, and 16 steps leave the three-byte range); the terms hold
    # symbols of the same family that the pattern lacks
    fams = {"cyrillic-32": [0x400 + i for i in range(32)], "step-64": [0x4E00 + 64 * i for i in range(21)], "step-256": [0x3000 + 256 * i for i in range(21)],
            "step-4096": [0x800 + 4096 * i for i in range(16) if i != 13]}
    step = {"cyrillic-32": 1, "step-64": 64, "step-256": 256, "step-4096": 4096}
    pats, terms = [], []
    for name, fam in fams.items():
        assert len(set(fam)) == len(fam) and len(u(*fam)) <= 64 and well_formed(u(*fam)), name
        lacks = (fam[-1] + step[name] if name != "step-4096" else 0x800 + 13 * 4096 + 0x800, fam[0] - step[name] if name != "step-4096" else 0xFFF)
        assert not set(lacks) & set(fam)
        pats.append(u(*fam))
        terms += _near(fam, lacks) + [u(*fam[::-1])]
    cases.append(_fuzzy("lookup-under-load", [terms], [p for p in pats for _ in range(3)], [0, 1, 2] * 4, 0, [UTF8, UTF8, UTF8 | TRANSPOSE] * 4))
    # kernel seams: runs of multi-byte terms across the workgroup edge of 256 terms (the neighbour matcher), at 255 / 256 / 257
    shapes = {"all": lambda i: True, "even": lambda i: i % 2 == 0, "but-the-edge": lambda i: i not in (255, 256), "only-the-edge": lambda i: i in (255, 256),
              "last-of-each": lambda i: i % 256 == 255}
    for n in (255, 256, 257, 513):
        cases.append(_fuzzy(f"workgroup-edge-{n}", [numbered(n, hit) for hit in shapes.values()], [b"00000" + u(0xE9), b"00000" + u(0x20AC) * 7], [5, 5], [0, 2]))
    # k = 3 with an empty dictionary
    words = [w.encode("utf-8") for w in ("naïve", "naive", "naïf", "niave", "señor", "senor", "señora", "日本語", "日本", "über", "uber", "ubër")]
    cases.append(_fuzzy("k3-with-an-empty-dictionary", [words, [], words[::2] + [b"zz"]], [w.encode("utf-8") for w in ("naïve", "señor", "日本語", "über", "über")],
                        [1, 1, 1, 2, 1], [0, 2, 0, 1, 0], [UTF8, UTF8 | NOCASE, UTF8, UTF8 | TRANSPOSE, 0]))
    return cases


def numbered(n, hit):
    """n sorted terms: five digits and one two-byte symbol where hit(i) (6 symbols), else five digits and seven three-byte ones"""
    return [b"%05d" % i + (u(0xE9) if hit(i) else u(0x20AC) * 7) for i in range(n)]


FUZZY_CASES = build_fuzzy()


# ---- match ----
def _glob_tokens(pattern):
    """[("*",) | ("?",) | ("=", symbol)]; None for a lone backslash at the end"""
    out, syms, i = [], decode(pattern), 0
    while i < len(syms):
        c = syms[i]
        if c == 0x5C:
            i += 1
            if i == len(syms):
                return None
            out.append(("=", syms[i]))
        elif c == 0x2A:
            out.append(("*",))
        elif c == 0x3F:
            out.append(("?",))
        else:
            out.append(("=", c))
        i += 1
    return out


def glob_symbols(tokens, term):
    """the whole term, symbol by symbol"""
    t = decode(term)
    reach = {0}                                  # the term positions the tokens so far can end at
    for tok in tokens:
        if tok[0] == "*":
            reach = set(range(min(reach), len(t) + 1)) if reach else set()
        elif tok[0] == "?":
            reach = {i + 1 for i in reach if i < len(t)}
        else:
            reach = {i + 1 for i in reach if i < len(t) and t[i] == tok[1]}
    return len(t) in reach


def matcher(kind, pattern):
    """term -> bool; without II2_MATCH_UTF8, or for CONTAINS / SUFFIX, match_cases' byte rule"""
    if not kind & UTF8 or kind & ~(NOCASE | UTF8) != GLOB:
        return match_cases.matcher(kind & ~UTF8, pattern)
    nocase = bool(kind & NOCASE)
    tokens = _glob_tokens(pattern.translate(_FOLD) if nocase else pattern)
    return lambda t: glob_symbols(tokens, t.translate(_FOLD) if nocase else t)


def expected_match(case):
    """(run_off, run_first, run_end, run_dict, n_matched), laid out as match_cases.expected_table"""
    key = "match:" + case.name
    if key not in _EXPECTED:
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
        _EXPECTED[key] = (run_off, first, end, which, matched)
    return _EXPECTED[key]


def _match(name, dicts, patterns, kinds):
    dicts = [sorted(set(d)) for d in dicts]
    assert len(patterns) == len(kinds) <= 64 and all(len(p) <= 64 for p in patterns), name
    assert all(not k & UTF8 or well_formed(p) for p, k in zip(patterns, kinds)), name
    assert all(len(d) <= 5000 for d in dicts), name
    return match_cases.Case(name, dicts, list(patterns), list(kinds))


def build_match():
    cases = []
    G = GLOB | UTF8
    e, euro, grin = u(0xE9), u(0x20AC), u(0x1F600)
    terms = [e, euro, grin, b"\x80", b"\xff", b"", b"a", b"ab", b"abc", "café".encode(), b"cafe", b"caf", "CAFÉ".encode(), b"caf\xc3", b"?", e + b"?", b"a" + e, e + e,
             b"a" + euro + b"b", euro + euro, b"x" + grin, b"\xc3\xa9\xa9", b"\xe2\x82", b"*" + e]
    pats = [b"?", b"??", b"*??", b"*?", b"caf?", b"\\?", b"\\" + e, b"*" + e, b"*" + euro + b"b", b"?" + e, b"*?" + e, b"a*", b"???", b"*", b"", b"?*?", b"\\*" + e, b"?\\?"]
    cases.append(_match("glob-by-symbols", [terms], pats * 2 + [b"CAF?", b"CAF?", b"caf" + e, "CAFÉ".encode()],
                        [G] * len(pats) + [GLOB] * len(pats) + [G | NOCASE, GLOB | NOCASE, G | NOCASE, G | NOCASE]))
    # the end-of-term trap with `?`: AC is one symbol, 8F E2 82 three - and neither grows by its neighbour's bytes
    trap_terms = TRAP + [b"x" + euro, euro, b"a", b"\x8f", b"\x8e" + euro]
    assert sorted(trap_terms)[sorted(trap_terms).index(TRAP[0]) + 1] == TRAP[1]
    cases.append(_match("end-of-term-trap", [trap_terms], [b"?", b"??", b"???", b"*?", b"?*", b"?", b"???", b"*" + euro], [G, G, G, G, G, GLOB, GLOB, G]))
    # CONTAINS and SUFFIX with the flag answer as without it, also with ill-formed bytes around the hit
    around = [b"\xff" + e + b"\x80", b"\xe2" + e, e + b"\xa9", b"\xc3" + e, b"\xc3\xc3\xa9", b"\xc3\xa9\xa9", b"\xa9", b"\xc3", euro + e, b"\xe2\x82" + e,
              b"\xe2\x82\xc3\xa9", e, b"x" + e + b"y", b"\xf0\x9f" + e + b"\x98\x80", "CAFÉ".encode(), "café".encode()]
    lits = [e, euro, b"x" + e, e + b"y", b"caf" + e, b""]
    cases.append(_match("contains-and-suffix", [around], lits * 6,
                        [CONTAINS | UTF8] * 6 + [CONTAINS] * 6 + [SUFFIX | UTF8] * 6 + [SUFFIX] * 6 + [CONTAINS | UTF8 | NOCASE] * 6 + [SUFFIX | NOCASE] * 6))
    shapes = {"all": lambda i: True, "even": lambda i: i % 2 == 0, "but-the-edge": lambda i: i not in (255, 256), "only-the-edge": lambda i: i in (255, 256),
              "last-of-each": lambda i: i % 256 == 255}
    for n in (255, 256, 257, 513):
        cases.append(_match(f"workgroup-edge-{n}", [numbered(n, hit) for hit in shapes.values()], [b"?????" + e, b"?????", b"*" + euro, b"??????", b"*0?" + e],
                            [G, G, G, G, G]))
    words = [w.encode("utf-8") for w in ("naïve", "naive", "naïf", "señor", "senor", "日本語", "日本", "über", "uber")]
    cases.append(_match("k3-with-an-empty-dictionary", [words, [], words[::2] + [b"zz"]], [b"na?ve", b"na?ve", b"*\xc3\xb1*", "日本?".encode(), b"?ber", b"se*r"],
                        [G, GLOB, G, G, G | NOCASE, CONTAINS | UTF8]))
    return cases


MATCH_CASES = build_match()


def ascii_fuzzy_cases():
    """every case of fuzzy_cases.CASES whose patterns and terms are all below 0x80, with the flag OR-ed into every pattern"""
    plain = lambda c: all(max(b, default=0) < 0x80 for b in c.patterns + [t for d in c.dicts for t in d])
    return [(c, c._replace(name="utf8:" + c.name, flags=[f | UTF8 for f in c.flags])) for c in fuzzy_cases.CASES if plain(c)]


def ascii_match_cases():
    plain = lambda c: all(max(b, default=0) < 0x80 for b in c.patterns + [t for d in c.dicts for t in d])
    return [(c, c._replace(name="utf8:" + c.name, kinds=[k | UTF8 for k in c.kinds])) for c in match_cases.CASES if plain(c)]


def all_strings():
    """every pattern and term of the table"""
    out = set(ILL_FORMED)
    for c in FUZZY_CASES + MATCH_CASES:
        out |= set(c.patterns) | {t for d in c.dicts for t in d}
    return sorted(out)
