"""Dictionaries and probes aimed at the seams of the term lookup (ii2_dict_find / ii2_term_bounds, csrc/term_device.h), one
table for the CPU test of the arithmetic and the GPU test of the kernel.

A lookup that compares 8-byte big-endian keys first and bytes on ties can go wrong where a term or a probe ends at, just before
or just after the key's width, where the zero padding of a short key meets a term that holds real zero bytes, where a prefix
covers a part of the key, all of it, or more, and where thousands of terms share a few hundred keys, so that most steps of a
bisection are decided by the bytes.  Every case is (name, dictionaries, probes, flags): `dictionaries` are k sorted, duplicate-free lists of bytes,
`probes` a list of bytes, `flags` one 0 (exact) / 1 (prefix) per probe.

The expectation is computed here from Python's own order of bytes and bytes.startswith, never from the library:
  exact   [j, j + 1) when term j is the probe, else [j, j) with j the number of terms below the probe
  prefix  [number of terms below the probe, that plus the number of terms that start with it)
"""
import bisect
import itertools
import random
from typing import List, NamedTuple


class Case(NamedTuple):
    name: str
    dicts: List[List[bytes]]
    probes: List[bytes]
    flags: List[int]


def expected(terms, probe, prefix):
    """[first, end) of one probe in one sorted dictionary."""
    j = bisect.bisect_left(terms, probe)
    if not prefix:
        return j, j + (1 if j < len(terms) and terms[j] == probe else 0)
    e = j
    while e < len(terms) and terms[e].startswith(probe):      # the terms that start with the probe are one run, from j on
        e += 1
    return j, e


def expected_table(case):
    """(list_first, list_end, n_found) as ii2_dict_find lays them out: entry p * k + s."""
    first, end = [], []
    for p, f in zip(case.probes, case.flags):
        for d in case.dicts:
            a, b = expected(d, p, f)
            first.append(a)
            end.append(b)
    return first, end, sum(1 for a, b in zip(first, end) if b > a)


def flat(terms):
    """(bytes, offsets) of a list of bytes, the bytes padded by one so that the array is never empty."""
    off = [0]
    for t in terms:
        off.append(off[-1] + len(t))
    return b"".join(terms) + b"\0", off


def _both(dicts, probes):
    """every probe once exact and once as a prefix"""
    return list(probes) * 2, [0] * len(probes) + [1] * len(probes)


def _case(name, dicts, probes, flags=None):
    dicts = [sorted(set(d)) for d in dicts]
    if flags is None:
        probes, flags = _both(dicts, probes)
    return Case(name, dicts, list(probes), list(flags))


def _around(terms):
    """every term, its neighbours in byte order and its prefixes: probes that land on, before and after each term"""
    out = set()
    for t in terms:
        out.update({t, t + b"\0", t + b"\xff", t[:-1], t[:-1] + bytes([max(t[-1] - 1, 0)]) if t else b"", t[:8], t[:7], t[:9]})
        if t and t[-1] < 255:
            out.add(t[:-1] + bytes([t[-1] + 1]))
    return sorted(out)


def _ternary(n, seed):
    """n distinct terms over a 3-letter alphabet, lengths 0 .. 12: far more terms than distinct 8-byte keys share among them"""
    rng = random.Random(seed)
    out = set()
    while len(out) < n:
        out.add(bytes(rng.choice(b"abc") for _ in range(rng.choice((0, 3, 7, 8, 9, 9, 10, 11, 12, 12)))))
    return sorted(out)


def build():
    cases = []
    widths = [b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefgh\0", b"abcdefghj", b"abcdefghia", b"abcdefgi", b"abcdefg\0", b"abcdef"]
    cases.append(_case("empty-dictionary", [[]], [b"", b"a", b"\xff" * 9]))
    cases.append(_case("empty-term", [[b"", b"\0", b"\0\0", b"a"]], [b"", b"\0", b"\0\0", b"\0\0\0", b"\1", b"a", b"b"]))
    cases.append(_case("one-term", [[b"m"]], [b"", b"a", b"m", b"m\0", b"ma", b"z"]))
    cases.append(_case("below-and-above", [[b"bb", b"cc", b"dd"]], [b"", b"a", b"b", b"bb", b"bc", b"dd", b"dda", b"e", b"\xff"]))
    cases.append(_case("lengths-7-8-9", [widths], _around(widths)))
    ties = [b"tiebreak" + s for s in (b"", b"\0", b"\0\0", b"a", b"aa", b"ab", b"b", b"\xff", b"\xff\xff")]
    cases.append(_case("key-ties-at-byte-9", [ties], _around(ties) + [b"tiebrea", b"tiebreal", b"tiebreak\0\0\0"]))
    zeros = [b"a", b"a\0", b"a\0\0", b"a\0\1", b"a\1", b"b"]
    cases.append(_case("zero-padding", [zeros], [b"a", b"a\0", b"a\0\0", b"a\0\0\0", b"a\0\1", b"a\1", b"", b"\0"]))
    cases.append(_case("zero-padding-at-the-key-width",
                       [[b"1234567", b"1234567\0", b"1234567\0\0", b"1234567\0\0\0", b"12345678", b"1234567\0a"]],
                       [b"1234567", b"1234567\0", b"1234567\0\0", b"1234567\0\0\0", b"1234567\0\0\0\0", b"123456", b"12345678", b"1234567\1"]))
    pre = [b"prefix00", b"prefix00a", b"prefix00ab", b"prefix00b", b"prefix01", b"prefix0", b"prefiy", b"prefix00aa"]
    cases.append(_case("prefixes-of-8-and-9-bytes", [pre], [b"prefix00", b"prefix00a", b"prefix0", b"prefix00aa", b"prefix00ac", b"prefix00\0", b"prefix"]))
    ff = [b"\xff" * n for n in range(1, 13)] + [b"\xfe\xff", b"\xff\xfe", b"\xff" * 8 + b"\xfe", b"\xff" * 7 + b"\xfe"]
    cases.append(_case("ff-runs", [ff], [b"\xff" * n for n in range(0, 14)] + [b"\xfe", b"\xff\xfe", b"\xff" * 8 + b"\xfe"]))
    cases.append(_case("prefix-longer-than-every-term", [[b"ab", b"abc", b"abd", b"b"]], [b"abcdefghijklmnop", b"abcz", b"abdefghij", b"bbbbbbbbbbbb"]))
    cases.append(_case("run-reaches-the-end", [[b"a", b"za", b"zb", b"zzzzzzzzz", b"zzzzzzzzzz"]], [b"z", b"zz", b"zzzzzzzz", b"zzzzzzzzz", b"zzzzzzzzzz", b"zzzzzzzzzzz"]))
    # thousands of terms over a 3-letter alphabet: heavy ties of the keys, most steps are decided by the bytes
    big = _ternary(5000, 1)
    rng = random.Random(2)
    probes = rng.sample(big, 150) + [t + rng.choice((b"", b"a", b"c", b"\0")) for t in rng.sample(big, 60)]
    probes += [bytes(rng.choice(b"abc") for _ in range(n)) for n in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11) for _ in range(6)]
    probes += [b"", b"a", b"c", b"cccccccccccc", b"cccccccccccca", b"d", b"aaaaaaaa", b"aaaaaaaaa", b"`"]
    cases.append(_case("ternary-5000", [big], probes))
    # k = 3 and k = 64, dictionaries of unequal sizes (an empty one among them)
    pool = _ternary(900, 3)
    three = [pool[::2], pool[1::7], pool[:40] + pool[-5:]]
    probes3 = rng.sample(pool, 40) + [b"", b"a", b"abc", b"c", b"cc", b"abcabcabc", b"abcabcab"]
    cases.append(_case("k3-unequal", three, probes3))
    many = [[] if s == 17 else rng.sample(pool, rng.choice((1, 2, 5, 33, 200, 640))) for s in range(64)]
    cases.append(_case("k64-unequal", many, rng.sample(pool, 24) + [b"", b"b", b"bca", b"cccccccccccc\0"]))
    # mixed flags in one call
    mixed = list(itertools.chain.from_iterable((t, t[:5]) for t in pool[:60:3]))
    cases.append(_case("mixed-flags", [pool[:300], pool[100:500:3]], mixed, [i & 1 for i in range(len(mixed))]))
    return cases


CASES = build()
