"""The window arithmetic of the word-by-word two-list AND (csrc/intersect_words.hip k_and2_words: both lists as cached dense forms,
result bits = wa & wb & ~tomb) restated in plain numpy, and the pairs of lists that its tests add to tests/dense_form_cases.py.
tests/test_and2_words_cpu.py proves the table sound without a device, tests/test_gpu_and2_words.py runs it.

The window is the run of 32-doc words that both forms cover: from the later of the two origins to the earlier of the two ends.
Workgroup g of the kernel owns the words [g W, (g + 1) W) of it; a form's word i of the window is its own word i + (window's first
word - its origin's word); words from the window's end on, and tombstone words past that bitmap's end, read as zero."""
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from tests import dense_form_cases as dc

W = 2048                        # words of the window a workgroup owns (csrc/intersect_words.hip: AW_W) ...
WG_DOCS = 32 * W                # ... = 65 536 docs
LB_GROUP = 64                   # workgroups per look-back group (csrc/internal.h)


def window(x, y):
    """(first word, words) of the window of two lists; words = 0: no common word.  Word = doc >> 5"""
    lo = max(int(x[0]) >> 5, int(y[0]) >> 5)
    hi = min(int(x[-1]) >> 5, int(y[-1]) >> 5) + 1
    return lo, max(hi - lo, 0)


def workgroups(x, y):
    """rows of cycle counters the kernel fills: its grid, or none where the window is empty (one workgroup stores the count only)"""
    return (window(x, y)[1] + W - 1) // W


def form_offset(l, lo):
    """a form's word that is the window's word 0"""
    return lo - (dc.form_origin(l) >> 5)


def tomb_words(removed, lo, n):
    """the tombstone bitmap's words [lo, lo + n): the bitmap ends with its last removed doc's word, words past it read as zero"""
    out = np.zeros(n, np.uint32)
    if removed is None or removed.size == 0 or n == 0:
        return out
    r = removed.astype(np.int64)                          # (64-bit, and only the asked words: a bitmap up to doc 2^32 - 1 is 512 MiB)
    r = r[(r >= 32 * lo) & (r < 32 * (lo + n))]
    bits = np.zeros(32 * n, np.uint8)
    bits[r - 32 * lo] = 1
    out[:] = np.packbits(bits, bitorder="little").view("<u4")
    return out


def result_words(x, y, removed=None):
    """(first word, the window's result words) as the kernel forms them"""
    lo, n = window(x, y)
    if n == 0:
        return lo, np.zeros(0, np.uint32)
    wx, wy = dc.form_words(x), dc.form_words(y)
    ox, oy = form_offset(x, lo), form_offset(y, lo)
    assert 0 <= ox and ox + n <= wx.size and 0 <= oy and oy + n <= wy.size          # the window lies inside both forms
    return lo, wx[ox:ox + n] & wy[oy:oy + n] & ~tomb_words(removed, lo, n)


def ids_of(lo, words):
    bits = np.unpackbits(words.astype("<u4").view(np.uint8), bitorder="little")
    return (np.flatnonzero(bits).astype(np.int64) + 32 * lo).astype(np.uint32)


def per_workgroup(words):
    """ids each workgroup publishes"""
    pad = np.zeros((-words.size) % W, np.uint32)
    pc = np.unpackbits(np.concatenate([words, pad]).astype("<u4").view(np.uint8)).reshape(-1, 32 * W).sum(axis=1)
    return pc.astype(np.int64)


def reference(x, y, removed=None):
    want = np.intersect1d(x, y, assume_unique=True)
    if removed is not None:
        want = np.setdiff1d(want, removed, assume_unique=True)
    return want.astype(np.uint32)


def with_docs(l, docs):
    return np.union1d(l, np.asarray(docs, np.uint32)).astype(np.uint32)


@dataclass
class Case:
    name: str
    make: Callable[[], tuple]                 # -> (x, y[, removed]) in the order the query names them
    check: Callable                           # the property the case is there for: predicate on (x, y, removed, lo, result words)
    _cache: Optional[tuple] = None

    def data(self):
        if self._cache is None:
            d = self.make()
            self._cache = (d[0], d[1], d[2] if len(d) > 2 else None)
        return self._cache


U = 820_000
FULL = (3 * WG_DOCS, 6 * WG_DOCS)             # both lists hold every doc: workgroups 3, 4 and 5 of a window that starts at doc 0
REMOVED_WG = 4                                # ... of which this one is tombstoned away in `stretches_removed`
APART = (7 * WG_DOCS, 10 * WG_DOCS)           # the lists alternate: no common doc in workgroups 7, 8 and 9


def _stretches(removed):
    def make():
        rng = np.random.default_rng(31)
        b, a = dc.bern(rng, 0.25, 0, U), dc.bern(rng, 0.45, 0, U)
        full = np.arange(*FULL, dtype=np.uint32)
        even = np.arange(APART[0], APART[1], 2, dtype=np.uint32)
        cut = lambda l: dc.punch(l, [FULL, APART])
        b = with_docs(np.concatenate([cut(b), full, even + 1]), [0])
        a = with_docs(np.concatenate([cut(a), full, even]), [0])          # doc 0 in both: the window starts at word 0
        if not removed:
            return b, a
        gone = np.arange(REMOVED_WG * WG_DOCS, (REMOVED_WG + 1) * WG_DOCS, dtype=np.uint32)
        return b, a, gone
    return make


def _all_ones(words, g):
    return bool(np.all(words[g * W:(g + 1) * W] == 0xFFFFFFFF))


def _disjoint():
    rng = np.random.default_rng(32)
    return dc.bern(rng, 0.7, 0, 400_000), dc.bern(rng, 0.5, 500_000, 1_320_000)


ONE_WORD = 819_200                            # a multiple of 32: the word both forms share


def _one_word():
    rng = np.random.default_rng(33)
    b = with_docs(dc.bern(rng, 0.7, ONE_WORD + 6, ONE_WORD + 400_000), [ONE_WORD + 5, ONE_WORD + 7, ONE_WORD + 20])
    a = with_docs(dc.bern(rng, 0.5, 0, ONE_WORD), [ONE_WORD + 5, ONE_WORD + 7, ONE_WORD + 20])
    a = a[a <= ONE_WORD + 20]
    return b, a


def _offset(d):
    def make():
        rng = np.random.default_rng(34 + d)
        b = with_docs(dc.bern(rng, 0.34, 32 * d + 3, U), [32 * d + 3])      # B's form starts d words behind A's
        a = with_docs(dc.bern(rng, 0.5, 0, U), [1])
        removed = dc.bern(rng, 0.05, 0, U // 2)
        return b, a, removed
    return make


def _two_groups():
    rng = np.random.default_rng(38)
    n = (2 * LB_GROUP + 3) * WG_DOCS
    return dc.bern(rng, 0.33, 0, n), dc.bern(rng, 0.5, 0, n)


CASES = [
    Case("stretches", _stretches(False),                                     # (a) the stage's worst case, (c) workgroups that publish 0
         lambda x, y, r, lo, w: lo == 0 and FULL[1] - FULL[0] > 2 * WG_DOCS and all(_all_ones(w, g) for g in (3, 4, 5)) and
         not np.any(w[APART[0] >> 5:APART[1] >> 5]) and list(per_workgroup(w)[7:10]) == [0, 0, 0] and per_workgroup(w)[6] > 0 and per_workgroup(w)[10] > 0),
    Case("stretches_removed", _stretches(True),                              # (b) every bit removed in one workgroup, none in the next
         lambda x, y, r, lo, w: lo == 0 and not np.any(w[REMOVED_WG * W:(REMOVED_WG + 1) * W]) and _all_ones(w, REMOVED_WG - 1) and
         _all_ones(w, REMOVED_WG + 1) and (int(r[-1]) >> 5) + 1 == (REMOVED_WG + 1) * W),
    Case("disjoint", _disjoint, lambda x, y, r, lo, w: window(x, y)[1] == 0 and w.size == 0),      # (d)
    Case("one_word", _one_word,                                              # (e)
         lambda x, y, r, lo, w: window(x, y) == (ONE_WORD >> 5, 1) and list(ids_of(lo, w)) == [ONE_WORD + 5, ONE_WORD + 7, ONE_WORD + 20]),
] + [
    Case(f"offset_{d}", _offset(d),                                          # (f) the unaligned 16-byte loads
         lambda x, y, r, lo, w, d=d: lo == d and abs(form_offset(x, lo) - form_offset(y, lo)) == d and lo % 4 == d)
    for d in (1, 2, 3)
] + [
    Case("two_groups", _two_groups, lambda x, y, r, lo, w: workgroups(x, y) > 2 * LB_GROUP),      # (g)
]
BY_NAME = {c.name: c for c in CASES}
