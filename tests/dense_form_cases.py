"""The case table of the dense form (a list of a two-list AND cached as a bitmap over its docs: csrc/setop.cpp dense_form_get,
csrc/intersect_and2.hip k_dense_form_build and k_and2_fused<true>).  Plain numpy: tests/test_dense_form_cpu.py checks the table
itself without a device, tests/test_gpu_dense_form.py runs it.

A case is a pair of lists.  B, the one with fewer blocks, paces the waves of the kernel (16 of its blocks a wave, 64 a workgroup);
A, the one with more blocks, is the list that gets a form.  The one-launch two-list AND takes a pair whose B holds >= 1024 blocks
at <= 1100 docs per block - the smallest shapes are B ~ 266 k postings against A ~ 400 k over ~ 800 k docs."""
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

BLOCK = 256                     # postings of a DV1 block
CAPW = 16384                    # docs of a wave's LDS window (csrc/internal.h: DENSE_CAPW)
MIN_BLOCKS = 1024               # the dense path: blocks of the driver at least ...
MAX_DOCS_PER_BLOCK = 1100.0     # ... and its docs per block at most
WG_BLOCKS = 64                  # driver blocks per workgroup of k_and2_fused


def bern(rng, p, lo, hi):
    return (np.flatnonzero(rng.random(hi - lo) < p) + lo).astype(np.uint32)


def punch(x, holes):
    keep = np.ones(x.size, bool)
    for lo, hi in holes:
        keep &= ~((x >= lo) & (x < hi))
    return x[keep]


def blocks(l):
    return (len(l) + BLOCK - 1) // BLOCK


def docs_per_block(l):
    """what the AND chooser looks at: (first doc of the last block - first doc) / (blocks - 1)"""
    n = blocks(l)
    return (int(l[(n - 1) * BLOCK]) - int(l[0])) / (n - 1)


def gaps_in_blocks(l):
    """the gaps a DV1 payload holds: every posting's distance to the one before it, except a block's first posting"""
    g = np.diff(l.astype(np.int64))
    return g[(np.arange(1, l.size) % BLOCK) != 0]


def payload_bytes(l):
    g = gaps_in_blocks(l)
    return int(g.size + np.count_nonzero(g >= 1 << 7) + np.count_nonzero(g >= 1 << 14) + np.count_nonzero(g >= 1 << 21) + np.count_nonzero(g >= 1 << 28))


def form_origin(l):
    return int(l[0]) & ~31


def form_words(l):
    """the packed-bits reference: bit d - origin of the word array is set when doc d is in the list"""
    o = form_origin(l)
    n = ((int(l[-1]) - o) >> 5) + 1
    bits = np.zeros(32 * n, np.uint8)
    bits[l.astype(np.int64) - o] = 1
    return np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)


def form_bytes(l):
    return 4 * (((int(l[-1]) - form_origin(l)) >> 5) + 1)


def criterion_b(l):
    """(b) of the issue: the form's bytes are at most half the list's payload bytes"""
    return 2 * form_bytes(l) <= payload_bytes(l)


def roles(x, y):
    """(B, A) as the AND chooser assigns them: a stable sort by blocks"""
    return (x, y) if blocks(x) <= blocks(y) else (y, x)


def has_multibyte_gap(l):
    return bool(np.any(gaps_in_blocks(l) >= 128))


def has_wide_group(l):
    """some aligned group of four one-byte gaps of a full block sums to >= 32 docs (a2_mark_rows places it posting by posting)"""
    for b in range(blocks(l) - 1):
        g = np.diff(l[b * BLOCK:(b + 1) * BLOCK].astype(np.int64))[:252]
        if np.all(g < 128) and np.any(g.reshape(-1, 4).sum(axis=1) >= 32):
            return True
    return False


@dataclass
class Case:
    name: str
    make: Callable[[], tuple]                 # -> (x, y[, removed]) in the order the query names them
    form: bool = True                         # (b) holds for A: option 1 makes a form
    removed: bool = False
    checks: dict = field(default_factory=dict)   # further properties the CPU test asserts (name -> predicate on (B, A, removed))
    _cache: Optional[tuple] = None

    def data(self):
        if self._cache is None:
            d = self.make()
            self._cache = (d[0], d[1], d[2] if len(d) > 2 else None)
        return self._cache


def _uniform(swap):
    def make():
        rng = np.random.default_rng(1)
        U = 820_000
        a, b = bern(rng, 1 / 2, 0, U), bern(rng, 1 / 3, 0, U)
        return (a, b) if swap else (b, a)
    return make


def _alignment(last_bit):
    def make():
        rng = np.random.default_rng(2)
        U = 820_000
        b = bern(rng, 0.34, 0, U)
        last = 800_000 + last_bit                               # 800 000 is a multiple of 32: the last doc sits at this bit of the last word
        a = bern(rng, 0.5, 37, last)
        a = np.union1d(a, np.array([37, last], np.uint32)).astype(np.uint32)
        return b, a
    return make


def _b_wider():
    rng = np.random.default_rng(3)
    b = bern(rng, 0.3, 0, 1_000_000)
    a = bern(rng, 0.6, 100_010, 900_000)
    a = np.union1d(a, np.array([100_010], np.uint32)).astype(np.uint32)      # origin 100 000: ten empty bits, then the list
    return b, a


def _a_wider():
    rng = np.random.default_rng(4)
    b = bern(rng, 0.45, 100_010, 700_000)
    a = bern(rng, 0.5, 0, 1_000_000)
    return b, a


GAP_WINDOW = (300_000, 320_000)        # longer than CAPW docs: the wave that holds it takes two windows
GAP_WIDE = (500_000, 570_000)          # longer than 65 535 docs: that wave's ids do not fit 16-bit offsets


def gap_over(l, doc):
    """the gap of l that reaches over `doc`"""
    i = int(np.searchsorted(l, doc))
    return int(l[i]) - int(l[i - 1])


def _gap_in_b():
    rng = np.random.default_rng(5)
    b = punch(bern(rng, 0.5, 0, 700_000), [GAP_WINDOW, GAP_WIDE])
    a = bern(rng, 0.62, 0, 700_000)
    return b, a


def _holes(rng, U, n, width):
    return [(int(s), int(s) + width) for s in rng.integers(1000, U - 1000, n)]


def _hard_b():
    rng = np.random.default_rng(6)
    U = 820_000
    b = punch(bern(rng, 0.4, 0, U), _holes(rng, U, 60, 300))
    if b.size % BLOCK == 0:
        b = b[:-1]
    a = bern(rng, 0.55, 0, U)
    return b, a


THIN = (400_000, 420_000)


def _slow_a():
    rng = np.random.default_rng(7)
    U = 820_000
    b = bern(rng, 0.34, 0, U)
    a = punch(bern(rng, 0.55, 0, U), _holes(rng, U, 60, 300))
    thin = (a >= THIN[0]) & (a < THIN[1]) & (rng.random(a.size) > 0.08)     # a stretch at ~ 4 %: groups of four postings ~ 90 docs wide
    a = a[~thin]
    if a.size % BLOCK == 0:
        a = a[:-1]
    return b, a


def _tombstones(whole_window):
    def make():
        rng = np.random.default_rng(8)
        U = 820_000
        b, a = bern(rng, 0.34, 0, U), bern(rng, 0.5, 0, U)
        removed = bern(rng, 0.05, 0, U // 2)                   # the bitmap ends long before the lists' last windows
        if whole_window:
            removed = np.union1d(removed, np.arange(200_000, 240_000, dtype=np.uint32)).astype(np.uint32)
        return b, a, removed
    return make


def _criterion():
    rng = np.random.default_rng(11)
    b = bern(rng, 0.3, 0, 1_000_000)
    a = bern(rng, 0.2, 0, 2_200_000)          # one posting per 5 docs: the form is 5 / 8 of the payload
    return b, a


def _many_workgroups():
    rng = np.random.default_rng(12)
    U = 2_900_000
    return bern(rng, 0.4, 0, U), bern(rng, 0.5, 0, U)


def _removed_everywhere(B, A, removed):
    hits = np.intersect1d(B, A, assume_unique=True)
    return all(np.intersect1d(x, removed, assume_unique=True).size > 100 for x in (B, A, hits)) and int(removed[-1]) + 2 * CAPW < int(B[-1])


CASES = [
    Case("uniform", _uniform(False)),
    Case("uniform_swapped", _uniform(True)),
    Case("alignment_last_bit31", _alignment(31),
         checks={"first_unaligned": lambda B, A, r: int(A[0]) % 32 != 0, "last_bit": lambda B, A, r: (int(A[-1]) - form_origin(A)) % 32 == 31}),
    Case("alignment_last_bit0", _alignment(0),
         checks={"first_unaligned": lambda B, A, r: int(A[0]) % 32 != 0, "last_bit": lambda B, A, r: (int(A[-1]) - form_origin(A)) % 32 == 0}),
    Case("b_wider", _b_wider,
         checks={"contains": lambda B, A, r: int(B[0]) + 4 * CAPW < int(A[0]) and int(A[-1]) + 4 * CAPW < int(B[-1]),
                 "first_word_partial": lambda B, A, r: int(A[0]) != form_origin(A),
                 "b_around_origin": lambda B, A, r: np.any((B >= form_origin(A) - 32) & (B < form_origin(A))) and np.any((B >= form_origin(A)) & (B < int(A[0])))}),
    Case("a_wider", _a_wider,
         checks={"contains": lambda B, A, r: int(A[0]) + 4 * CAPW < int(B[0]) and int(B[-1]) + 4 * CAPW < int(A[-1])}),
    Case("gap_in_b", _gap_in_b,
         checks={"gap_window": lambda B, A, r: CAPW < gap_over(B, GAP_WINDOW[0]) <= 65535,
                 "gap_wide": lambda B, A, r: gap_over(B, GAP_WIDE[0]) > 65535,
                 "dense_on_average": lambda B, A, r: docs_per_block(B) <= MAX_DOCS_PER_BLOCK,
                 "a_dense_through": lambda B, A, r: all(np.count_nonzero((A >= lo) & (A < hi)) > (hi - lo) // 2 for lo, hi in (GAP_WINDOW, GAP_WIDE))}),
    Case("hard_rows_in_b", _hard_b,
         checks={"multibyte": lambda B, A, r: has_multibyte_gap(B), "short_last": lambda B, A, r: B.size % BLOCK != 0}),
    Case("slow_paths_in_a", _slow_a,
         checks={"multibyte": lambda B, A, r: has_multibyte_gap(A), "wide_group": lambda B, A, r: has_wide_group(A),
                 "short_last": lambda B, A, r: A.size % BLOCK != 0}),
    Case("tombstones", _tombstones(False), removed=True, checks={"removed_everywhere": _removed_everywhere}),
    Case("tombstones_whole_window", _tombstones(True), removed=True,
         checks={"removed_everywhere": _removed_everywhere,
                 "covers_windows": lambda B, A, r: np.intersect1d(np.arange(200_000, 240_000, dtype=np.uint32), r).size == 40_000 > 2 * CAPW}),
    Case("criterion", _criterion, form=False),
    Case("many_workgroups", _many_workgroups,
         checks={"beyond_one_group": lambda B, A, r: blocks(B) > 64 * WG_BLOCKS}),
]
BY_NAME = {c.name: c for c in CASES}


def reference(case):
    x, y, removed = case.data()
    want = np.intersect1d(x, y, assume_unique=True)
    if removed is not None:
        want = np.setdiff1d(want, removed, assume_unique=True)
    return want.astype(np.uint32)
