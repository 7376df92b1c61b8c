"""CPU: II2_MATCH_UTF8 without a GPU - the decoder (csrc/utf8_device.h) through ii2_utf8_decode against Python's
bytes.decode("utf-8", "surrogateescape"), and the two matchers through the host-only ii2_term_fuzzy / ii2_term_match, which run
the parse, the table build, the symbol lookup, the filters, the recurrence and the glob the kernels run - so every (pattern, term)
of tests/utf8_cases.py is pinned here, match and exact distance; tests/test_gpu_dict_utf8.py runs the same table through the
kernels.  Also the argument errors, the table's own coverage, and the layers around the kernels."""
import ctypes as C
import os
import random
import re

import pytest

from inverted_index_2_amd import _lib, term_fuzzy, term_match, term_regex, utf8_decode
from inverted_index_2_amd.engine import II2Error
from tests import fuzzy_cases, match_cases, utf8_cases
from tests.utf8_cases import CONTAINS, GLOB, NOCASE, SUFFIX, TRANSPOSE, UTF8, decode, surrogateescape, u


def test_the_tables_decoder_is_surrogateescape():
    for s in utf8_cases.all_strings():
        assert decode(s) == surrogateescape(s), s
    for cp in utf8_cases.SEAMS:
        assert decode(u(cp)) == [cp]


def test_decode_on_the_table_and_on_every_code_point():
    for s in utf8_cases.all_strings():
        assert utf8_decode(s) == (surrogateescape(s), utf8_cases.well_formed(s)), s
    everything = "".join(chr(c) for c in range(0x110000) if not 0xD800 <= c <= 0xDFFF)
    syms, ok = utf8_decode(everything.encode("utf-8"))
    assert ok and syms == [ord(c) for c in everything]


def test_decode_on_random_strings_over_the_seam_bytes():
    lib = _lib.load()
    seam = bytes([0x00, 0x41, 0x7F, 0x80, 0x8F, 0x90, 0x9F, 0xA0, 0xBF, 0xC0, 0xC1, 0xC2, 0xDF, 0xE0, 0xE1, 0xEC, 0xED, 0xEE, 0xEF, 0xF0, 0xF1, 0xF3, 0xF4, 0xF5, 0xFF])
    rng = random.Random(7)
    out = (C.c_uint32 * 16)()
    n, ok = C.c_uint64(), C.c_int()
    for _ in range(100_000):
        s = bytes(rng.choice(seam) for _ in range(rng.randrange(0, 9)))
        assert lib.ii2_utf8_decode(s or None, len(s), out, 16, C.byref(n), C.byref(ok)) == 0
        want = surrogateescape(s)
        assert out[:n.value] == want and bool(ok.value) == utf8_cases.well_formed(s), s


def test_decode_argument_errors_and_the_cap_rule():
    lib = _lib.load()
    out = (C.c_uint32 * 4)(7, 7, 7, 7)
    n, ok = C.c_uint64(99), C.c_int(55)
    s = "a€😀é".encode() + b"\xff"
    assert lib.ii2_utf8_decode(s, len(s), out, 2, C.byref(n), C.byref(ok)) == 0
    assert n.value == 5 and list(out) == [0x61, 0x20AC, 7, 7] and ok.value == 0                # the full count, at most cap symbols
    assert lib.ii2_utf8_decode(s, len(s), None, 0, C.byref(n), None) == 0 and n.value == 5     # symbols and well_formed may be NULL
    assert lib.ii2_utf8_decode(None, 0, None, 0, C.byref(n), C.byref(ok)) == 0 and n.value == 0 and ok.value == 1
    n.value, ok.value = 99, 55
    assert lib.ii2_utf8_decode(s, len(s), out, 4, None, C.byref(ok)) == -1                      # NULL n_symbols
    assert lib.ii2_utf8_decode(None, 3, out, 4, C.byref(n), C.byref(ok)) == -1                  # NULL bytes with len > 0
    assert lib.ii2_utf8_decode(s, len(s), None, 4, C.byref(n), C.byref(ok)) == -1               # NULL symbols with cap > 0
    assert n.value == 99 and ok.value == 55 and list(out) == [0x61, 0x20AC, 7, 7]


@pytest.mark.parametrize("case", utf8_cases.FUZZY_CASES, ids=lambda c: c.name)
def test_fuzzy_every_pattern_against_every_term(case):
    lib = _lib.load()
    m, dist = C.c_int(), C.c_uint32()
    terms = sorted({t for d in case.dicts for t in d})
    if len(terms) > 600:
        terms = terms[:40] + terms[250:262] + terms[-40:]
    for p, d, pre, fl in zip(case.patterns, case.dists, case.prefixes, case.flags):
        for t in terms:
            assert lib.ii2_term_fuzzy(fl, p or None, len(p), pre, d, t or None, len(t), C.byref(m), C.byref(dist)) == 0
            assert bool(m.value) == utf8_cases.matches(p, t, d, pre, fl), (p, t, d, pre, fl)
            assert dist.value == utf8_cases.distance(p, t, fl), (p, t, fl)


@pytest.mark.parametrize("case", utf8_cases.MATCH_CASES, ids=lambda c: c.name)
def test_match_every_pattern_against_every_term(case):
    terms = sorted({t for d in case.dicts for t in d})
    if len(terms) > 600:
        terms = terms[:40] + terms[250:262] + terms[-40:]
    for p, kind in zip(case.patterns, case.kinds):
        want = utf8_cases.matcher(kind, p)
        for t in terms:
            assert term_match(kind, p, t) == want(t), (p, kind, t)


def test_ascii_cases_answer_as_without_the_flag():
    for plain, flagged in utf8_cases.ascii_fuzzy_cases():
        terms = sorted({t for d in plain.dicts for t in d})[:300]
        for p, d, pre, fl in zip(plain.patterns, plain.dists, plain.prefixes, plain.flags):
            for t in terms:
                assert term_fuzzy(p, t, d, pre, fl | UTF8) == (fuzzy_cases.matches(p, t, d, pre, fl), fuzzy_cases.distance(p, t, fl)), (p, t, fl)
    for plain, flagged in utf8_cases.ascii_match_cases():
        terms = sorted({t for d in plain.dicts for t in d})[:300]
        for p, kind in zip(plain.patterns, plain.kinds):
            want = match_cases.matcher(kind, p)
            for t in terms:
                assert term_match(kind | UTF8, p, t) == want(t), (p, kind, t)
    assert len(utf8_cases.ascii_fuzzy_cases()) >= 10 and len(utf8_cases.ascii_match_cases()) >= 8


def test_the_motivating_examples():
    e = lambda s: s.encode("utf-8")
    assert term_fuzzy(e("café"), b"cafe", 1, flags=UTF8) == (True, 1) and term_fuzzy(e("café"), b"cafe", 1) == (False, 2)
    assert term_fuzzy(e("日本語"), e("日本话"), 1, flags=UTF8) == (True, 1) and term_fuzzy(e("日本語"), e("日本话"), 1) == (False, 2)
    assert term_fuzzy(e("éà"), e("àé"), 1, flags=UTF8 | TRANSPOSE) == (True, 1) and term_fuzzy(e("éà"), e("àé"), 1, flags=TRANSPOSE) == (False, 2)
    assert term_fuzzy(e("É"), e("é"), 0, flags=UTF8 | NOCASE) == (False, 1) and term_fuzzy(e("É"), e("é"), 0, flags=NOCASE) == (False, 1)     # only A-Z folds
    assert term_fuzzy(e("éa"), e("èa"), 1, prefix=1, flags=UTF8) == (False, 1) and term_fuzzy(e("éa"), e("èa"), 1, prefix=1) == (True, 1)
    # the end-of-term trap, on the host: 3 symbols away, 2 bytes away
    assert term_fuzzy(b"x" + u(0x20AC), b"\x8f\xe2\x82", 2, flags=UTF8) == (False, 3) and term_fuzzy(b"x" + u(0x20AC), b"\x8f\xe2\x82", 2) == (True, 2)
    assert term_fuzzy(b"", e("日本語"), 3, flags=UTF8) == (True, 3) and term_fuzzy(b"", e("日本語"), 3) == (False, 9)
    G = GLOB | UTF8
    for sym in (e("é"), e("€"), e("😀"), b"\x80", b"\xff"):
        assert term_match(G, b"?", sym) and not term_match(G, b"??", sym)
    assert term_match(GLOB, b"??", e("é")) and not term_match(GLOB, b"?", e("é"))
    assert not term_match(G, b"*??", e("€")) and term_match(G, b"*?", e("€")) and term_match(GLOB, b"*??", e("€"))
    assert term_match(G, b"caf?", e("café")) and not term_match(GLOB, b"caf?", e("café"))
    assert term_match(G, b"\\?", b"?") and not term_match(G, b"\\?", e("é")) and term_match(G, b"\\" + e("é"), e("é"))
    assert term_match(G | NOCASE, b"CAF?", e("café")) and not term_match(G | NOCASE, e("CAFÉ"), e("café"))
    assert term_match(G, b"?", b"\xac") and not term_match(G, b"?", b"\x8f\xe2\x82") and term_match(G, b"???", b"\x8f\xe2\x82")


def _fz(flags, pat, prefix, term=b"a"):
    lib = _lib.load()
    m, d = C.c_int(77), C.c_uint32(88)
    return lib.ii2_term_fuzzy(flags, pat, len(pat), prefix, 1, term, len(term), C.byref(m), C.byref(d)), m.value, d.value


def test_pattern_errors():
    lib = _lib.load()
    for bad in utf8_cases.ILL_FORMED + [b"a\x80", b"\xc3\xa9\xc3", b"ab\xe2\x82"]:
        for fl in (UTF8, UTF8 | NOCASE, UTF8 | TRANSPOSE):
            assert _fz(fl, bad, 0) == (-1, 77, 88), bad                        # an ill-formed pattern with the flag ...
        assert _fz(0, bad, 0)[0] == 0, bad                                    # ... and accepted without
        for kind in (CONTAINS, SUFFIX, GLOB):
            m = C.c_int(77)
            assert lib.ii2_term_match(kind | UTF8, bad, len(bad), b"a", 1, C.byref(m)) == -1 and m.value == 77, (bad, kind)
            assert lib.ii2_term_match(kind, bad, len(bad), b"a", 1, C.byref(m)) == 0, (bad, kind)
    ee = "éé".encode()
    assert _fz(UTF8, ee, 3) == (-1, 77, 88) and _fz(0, ee, 3)[0] == 0 and _fz(UTF8, ee, 2)[0] == 0 and _fz(0, ee, 5) == (-1, 77, 88)      # the prefix counts symbols
    assert _fz(UTF8, "é".encode() * 32, 32)[0] == 0 and _fz(UTF8, "é".encode() * 32 + b"a", 0)[0] == -5                                     # the limit stays 64 bytes
    for flags in (0x02, 0x04, 0x40, 0x7f, 0x83, 0x0A, 0x4C):                     # the other bits stay unknown, with the new one as well
        assert _fz(flags, b"a", 0) == (-1, 77, 88), flags
    for kind in (3, 4, 0x0B, 0x0C, 0x40 | GLOB, 0x48 | GLOB, 0x7f, 0x83):
        with pytest.raises(II2Error):
            term_match(kind, b"a", b"a")
    with pytest.raises(II2Error) as e:                                           # the regular expressions keep rejecting the bit
        term_regex(b"a", b"a", UTF8)
    assert e.value.code == -1
    with pytest.raises(II2Error):
        term_regex(b"a", b"a", UTF8 | NOCASE)
    assert term_regex(b"a", b"a", NOCASE)[0]


def test_random_symbol_strings_against_the_plain_dp():
    rng = random.Random(3)
    alphabets = ([0x61, 0xE9, 0x20AC], [0x61, 0x62, 0x400, 0x401, 0x4E00, 0x1F600], [0x7F, 0x80, 0x7FF, 0x800, 0xFFFF, 0x10000])
    for _ in range(400):
        al = rng.choice(alphabets)
        pat = [rng.choice(al) for _ in range(rng.choice((0, 1, 2, 7, 15, 16, 17, 21)))]
        term = list(pat)
        for _ in range(rng.randrange(0, 5)):
            at = rng.randrange(len(term) + 1)
            term[at:at + rng.randrange(0, 2)] = [rng.choice(al)] * rng.randrange(0, 2)
        if rng.random() < 0.3:
            term = [rng.choice(al) for _ in range(rng.randrange(0, 40))]
        for fl, dp in ((UTF8, fuzzy_cases.levenshtein), (UTF8 | TRANSPOSE, fuzzy_cases.osa)):
            d = dp(pat, term)
            assert term_fuzzy(u(*pat), u(*term), d, flags=fl) == (True, d), (pat, term, fl)
            if d:
                assert term_fuzzy(u(*pat), u(*term), d - 1, flags=fl) == (False, d), (pat, term, fl)


def test_the_table_covers_what_it_claims():
    fz = {c.name: c for c in utf8_cases.FUZZY_CASES}
    mt = {c.name: c for c in utf8_cases.MATCH_CASES}
    assert len(fz) == len(utf8_cases.FUZZY_CASES) and len(mt) == len(utf8_cases.MATCH_CASES)
    assert all(len(d) <= 5000 for c in utf8_cases.FUZZY_CASES + utf8_cases.MATCH_CASES for d in c.dicts)
    # the instance goes by symbols
    assert utf8_cases.word_bits(fz["31-and-32-two-byte-symbols"]) == 32 and max(len(p) for p in fz["31-and-32-two-byte-symbols"].patterns) == 64
    assert utf8_cases.word_bits(fz["33-symbols-in-64-bytes"]) == 64 and utf8_cases.word_bits(fz["21-three-byte-symbols"]) == 32
    assert {len(p) for p in fz["21-three-byte-symbols"].patterns} == {63} and {len(p) for p in fz["16-four-byte-symbols"].patterns} == {64}
    assert utf8_cases.word_bits(fz["16-four-byte-symbols"]) == 32 and utf8_cases.word_bits(fz["64-ascii-symbols-flagged"]) == 64
    assert utf8_cases.word_bits(fz["lookup-under-load"]) == 32 and len(decode(fz["lookup-under-load"].patterns[0])) == 32
    # the trap: the stage holds 8F E2 82 AC, and only reading on makes the pair close
    trap = fz["end-of-term-trap"]
    assert utf8_cases.distance(trap.patterns[0], b"\x8f\xe2\x82", UTF8) == 3 and utf8_cases.distance(trap.patterns[0], b"\x8f\xe2\x82", 0) == 2
    assert utf8_cases.distance(trap.patterns[0], b"\x8f\xe2\x82\xac", UTF8) == 1 and {1, 2} <= {d for d, f in zip(trap.dists, trap.flags) if f & UTF8}
    i = trap.dicts[0].index(b"\x8f\xe2\x82")
    assert trap.dicts[0][i + 1] == b"\xac" and mt["end-of-term-trap"].dicts[0][mt["end-of-term-trap"].dicts[0].index(b"\x8f\xe2\x82") + 1] == b"\xac"
    # both rules in one call, and they disagree
    both = fz["bytes-against-symbols"]
    hits = [{t for t in both.dicts[0] if utf8_cases.matches(p, t, d, pre, fl)} for p, d, pre, fl in zip(both.patterns, both.dists, both.prefixes, both.flags)]
    assert {f & UTF8 for f in both.flags} == {0, UTF8} and [f & UTF8 for f in both.flags] == [UTF8, 0] * 6
    e = lambda s: s.encode("utf-8")
    assert e("cafe") in hits[0] - hits[1] and e("日本话") in hits[2] - hits[3] and e("àé") in hits[4] - hits[5] and e("èa") in hits[11] - hits[10]
    assert e("é") in hits[6] & hits[7] and e("é") not in hits[8] | hits[9]                # É / é under NOCASE: 1 both ways
    for c in utf8_cases.FUZZY_CASES:                       # (every case matches something and rejects something)
        w = utf8_cases.expected_fuzzy(c)
        assert 0 < w[4] < len(c.patterns) * sum(len(d) for d in c.dicts), c.name
    for c in utf8_cases.MATCH_CASES:
        w = utf8_cases.expected_match(c)
        assert 0 < w[4] < len(c.patterns) * sum(len(d) for d in c.dicts), c.name
    # a run of multi-byte terms across the edge of 256
    w = utf8_cases.expected_fuzzy(fz["workgroup-edge-513"])
    assert any(f < 256 < e for f, e in zip(w[1], w[2])) and any(e == 256 for e in w[2]) and any(f == 256 for f in w[1])
    assert any(not d for d in fz["k3-with-an-empty-dictionary"].dicts) and any(not d for d in mt["k3-with-an-empty-dictionary"].dicts)
    # the ill-formed forms the decoder has to refuse
    for s in (b"\x80", b"\xc0\x80", b"\xc1\xbf", b"\xe0\x80\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\xe2\x82", b"\xf0\x9f\x98", b"\xf5", b"\xff"):
        assert s in utf8_cases.ILL_FORMED and decode(s) == [0xDC00 + b for b in s]
    # the glob's own arithmetic
    g = lambda p, t: utf8_cases.matcher(GLOB | UTF8, p)(t)
    assert g(b"?", u(0x20AC)) and not g(b"*??", u(0x20AC)) and g(b"*?", u(0x20AC)) and not g(b"??", u(0xE9)) and g(b"a*b", b"ab") and not g(b"", b"a")


# ---- the layers around the kernels keep in step ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_layers_name_the_flag_and_the_decoder_is_defined_once():
    header = _read("include", "ii2.h")
    assert re.search(r"#define\s+II2_MATCH_UTF8\s+0x08u", header) and _lib.II2_MATCH_UTF8 == UTF8 == 0x08
    assert "int ii2_utf8_decode(" in header and "uint32_t n_utf8;" in header and "/* 48 bytes */" in header
    assert C.sizeof(_lib.FuzzyStats) == 48 and _lib.FuzzyStats.n_utf8.offset == 44
    lib = _lib.load()
    assert hasattr(lib, "ii2_utf8_decode")
    mk = _read("inverted_index_2_amd", "csrc", "Makefile")
    assert "utf8_device.h" in mk
    csrc = os.path.join(ROOT, "inverted_index_2_amd", "csrc")
    holders = [f for f in sorted(os.listdir(csrc)) if f.endswith((".h", ".hip", ".cpp")) and re.search(r"\buint32_t\s+utf8_at\s*\(", _read("inverted_index_2_amd", "csrc", f))]
    assert holders == ["utf8_device.h"]
    # nobody else takes sequences apart: the lead-byte bounds occur in the decoder alone
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".h", ".hip", ".cpp")) and f != "utf8_device.h":
            assert "0xF4u" not in _read("inverted_index_2_amd", "csrc", f) and "0xC2u" not in _read("inverted_index_2_amd", "csrc", f), f
    assert '#include "utf8_device.h"' in _read("inverted_index_2_amd", "csrc", "match_device.h")      # (fuzzy_device.h includes match_device.h)
    assert "utf8_at(" in _read("inverted_index_2_amd", "csrc", "fuzzy_device.h") and "utf8_at(" in _read("inverted_index_2_amd", "csrc", "dict_match.hip")
    go = _read("bindings", "go", "ii2.go")
    assert re.search(r"MatchUtf8\s+uint8\s*=\s*0x08", go) and "func Utf8Decode(" in go and "C.ii2_utf8_decode(" in go
    src = _read("inverted_index_2_amd", "host", "host_index.cpp")
    assert "II2_MATCH_UTF8" in src and "ii2_utf8_decode(" in src
    assert "II2_MATCH_UTF8" in _read("inverted_index_2_amd", "host.py") and "def utf8_decode(" in _read("inverted_index_2_amd", "engine.py")
