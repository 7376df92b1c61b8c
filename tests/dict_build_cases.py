"""The named inputs of ii2_dict_build shared by tests/test_dict_build_cpu.py (the order and the plan, no GPU) and
tests/test_gpu_dict_build.py (the kernels).  The reference everywhere is Python: sorted(set(terms)) on bytes - which is
bytes.Compare order - and index() into it."""
import random
import string
from collections import namedtuple

import numpy as np

MAX_TERM = 256          # II2_DICT_BUILD_MAX_TERM

# name, terms (list of bytes, any order, repeats allowed), expect: facts of the plan the case was written for
Case = namedtuple("Case", "name terms expect")

SEAMS = (7, 8, 15, 16, 17)
VOCAB37 = [b"t%02d" % i + b"x" * (i % 11) for i in range(37)]


def few_distinct(n, seed=3):
    """n draws from the 37-term vocabulary: runs of equal terms cross every wave and tile end once sorted"""
    rng = np.random.default_rng(seed)
    return [VOCAB37[int(i)] for i in rng.integers(0, len(VOCAB37), n)]


def all_distinct(n, seed=258):
    """n distinct terms of [a-zA-Z]{10..19}: the reference's randomString (shard_test.go:258-266)"""
    rnd = random.Random(seed)
    seen, out = set(), []
    while len(out) < n:
        t = "".join(rnd.choice(string.ascii_letters) for _ in range(rnd.randint(10, 19))).encode()
        if t not in seen:
            seen.add(t)
            out.append(t)
    return out


def _ff_00_nine():
    base = b"abcdefghi"
    out = [base]
    for p in range(9):
        for v in (0x00, 0xFF):
            out.append(base[:p] + bytes([v]) + base[p + 1:])
    return out + [b"\xff" * 9, b"\0" * 9]


def _seams():
    out = []
    for p in SEAMS:
        a = bytes(range(65, 65 + 20))
        out += [a, a[:p] + b"~" + a[p + 1:]]                # equal except at byte p
        out += [a[:p], a[:p + 1]]                           # one is the other's prefix at length p
        out += [a[:p] + b"\0", a[:p] + b"\0\0"]             # ... and the zero-padding ties there
    return out


def _lengths(cap):
    rng = np.random.default_rng(11)
    out = []
    for n in range(3, 301):
        out.append(bytes(rng.integers(97, 100, min(n, cap)).astype(np.uint8)))
    return out


CASES = [
    Case("hand", [b"b", b"a", b"b", b"", b"ab", b"a\0", b"a"], {}),
    Case("zero_ties", [b"a", b"a\0", b"a\0\0", b"a\0b", b"", b"\0", b"\0\0", b"a\0", b"\0"], {}),
    Case("ff_00_nine", _ff_00_nine(), {}),
    Case("seams", _seams(), {}),
    Case("lengths", [b"q" * n for n in (0, 1, 7, 8, 9, 15, 16, 17, 255, 256)] + [b"q" * 255 + b"\0"], {"len_pass": [1, 1]}),
    Case("common_prefix", [b"request_id=ab" + b"%04x" % ((i * 7919) % 65536) for i in range(500)], {"no_pass_before": 13, "len_pass": [0, 0]}),
    Case("identical", [b"the same term"] * 5000, {"n_passes": 0, "n_unique": 1}),
    Case("fixed_length", [b"%06d" % ((i * 31) % 1000) for i in range(700)], {"len_pass": [0, 0]}),
    # the lengths 3 .. 300 as data, capped at the limit: 256 = 0x100 occurs next to lengths below it, the second length byte varies
    Case("lengths_3_300_cap256", _lengths(256), {"len_pass": [1, 1]}),
    # ... and capped one below it: a second length byte never varies below 256
    Case("lengths_3_300_cap255", _lengths(255), {"len_pass": [1, 0]}),
    Case("all_distinct", all_distinct(20000), {"n_unique": 20000}),
    Case("few_distinct", few_distinct(9000), {"n_unique": 37}),
]
TOO_LONG = [b"ok", b"z" * 257]            # alone: II2_ERANGE

BY_NAME = {c.name: c for c in CASES}


def flat(terms):
    """(u8 bytes - one spare byte so that the array is never empty -, u64 offsets [n + 1])"""
    off = np.zeros(len(terms) + 1, np.uint64)
    if terms:
        off[1:] = np.cumsum([len(t) for t in terms])
    return np.frombuffer(b"".join(terms) + b"\0", np.uint8).copy(), off


def reference(terms):
    """(sorted distinct terms, index of every input term in them)"""
    uniq = sorted(set(terms))
    where = {t: i for i, t in enumerate(uniq)}
    return uniq, [where[t] for t in terms]


def numpy_plan(terms):
    """The plan restated: the terms padded with zeros to 8 * C columns; a byte position gets a pass iff its column is not
    constant, a length byte iff it is not constant.  -> (pos_pass[256], len_pass[2], n_passes, min_len, max_len)"""
    pos, lp = np.zeros(256, np.uint8), np.zeros(2, np.uint8)
    if not terms:
        return pos, lp, 0, 0, 0
    lens = np.array([len(t) for t in terms], np.int64)
    width = 8 * ((int(lens.max()) + 7) // 8)
    if width:
        m = np.zeros((len(terms), width), np.uint8)
        for i, t in enumerate(terms):
            m[i, :len(t)] = np.frombuffer(t, np.uint8)
        pos[:width] = (m != m[0]).any(axis=0)
    for b in range(2):
        col = (lens >> (8 * b)) & 0xFF
        lp[b] = int((col != col[0]).any())
    return pos, lp, int(pos.sum() + lp.sum()), int(lens.min()), int(lens.max())
