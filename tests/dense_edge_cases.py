"""The dense two-list AND family at the edges of the id space: the pairs of tests/dense_form_cases.py and tests/and2_words_cases.py
moved up to the last doc id, 0xFFFFFFFF, and across 0x80000000, and the family itself - the kernels a two-term AND of dense lists
can run through, each with the options that select it and the path it must take.  The table is plain numpy:
tests/test_dense_edge_cases_cpu.py proves it sound without a device, tests/test_gpu_dense_edges.py runs the family on every shifted
case and tests/test_gpu_segment_kinds_dense.py on every way of making a segment (run_family takes the context it is given).

A case is moved by a multiple of 65 536 docs - a workgroup of k_and2_words, 512 words of 128 docs, four LDS windows of a wave - so
word alignment, the window's first word modulo 4 and every window and workgroup boundary stay where the source case put them:
  top   the largest such shift that keeps the last doc <= 0xFFFFFFFF; then 0xFFFFFFFF joins both lists (a hit, and the last bit
        of the last word of both forms) and 0xFFFFFFFE the shorter one only (not a hit).  `one_word` is about two lists that
        share one word: there only the list that reaches the top gets 0xFFFFFFFF, a doc in both would join their windows
  mid   the shift that puts the median doc at 0x80000000, rounded to the multiple (to the nearest one at which both lists hold
        postings on both sides of 0x80000000 inside one 256-posting block)
Removed sets move with their lists.  At the top every tombstoned case has a second removed set that also removes 0xFFFFFFFE and
the last hit below it: its bitmap holds all 2^27 words, so no word of the lists lies past the bitmap's end."""
import zlib
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from tests import and2_words_cases as wc
from tests import dense_form_cases as dc

TOP = 0xFFFFFFFF
HALF = 0x80000000
UNIT = wc.WG_DOCS                       # docs a case moves by: a multiple of 128 and of dc.CAPW
TOMB_WORDS_ALL = 1 << 27                # words of a tombstone bitmap that reaches the last doc id
assert UNIT % 128 == 0 and UNIT % dc.CAPW == 0

SOURCES = [(dc, "uniform", ("top", "mid")), (dc, "alignment_last_bit31", ("top",)), (dc, "gap_in_b", ("top", "mid")),
           (dc, "tombstones_whole_window", ("top",)), (wc, "stretches_removed", ("top",)), (wc, "one_word", ("top",)),
           (wc, "offset_1", ("top", "mid")), (wc, "offset_3", ("top",))]
TOP_IN_ONE_LIST = ("one_word",)


def add_docs(l, docs):
    return np.union1d(l, np.asarray(docs, np.uint32)).astype(np.uint32)


def moved(l, by):
    out = l.astype(np.int64) + by
    assert out.size == 0 or (0 <= int(out[0]) and int(out[-1]) <= TOP)
    return out.astype(np.uint32)


def straddles(l):
    """postings on both sides of 0x80000000 inside one block of l"""
    i = int(np.searchsorted(l, HALF))
    return 0 < i < l.size and i % dc.BLOCK != 0


@dataclass
class Edge:
    module: object
    source: str
    at: str                                   # "top" or "mid"
    _cache: Optional[tuple] = None

    @property
    def name(self):
        return f"{self.source}@{self.at}"

    @property
    def case(self):
        return self.module.BY_NAME[self.source]

    def data(self):
        """(x, y in the order the query names them, [removed sets], shift)"""
        if self._cache is None:
            x, y, removed = self.case.data()
            if self.at == "top":
                by = (TOP - max(int(x[-1]), int(y[-1]))) // UNIT * UNIT
            else:
                nearest = int(round((HALF - float(np.median(np.concatenate([x, y])))) / UNIT))
                by = next(k * UNIT for d in range(64) for k in (nearest + d, nearest - d) if straddles(moved(x, k * UNIT)) and straddles(moved(y, k * UNIT)))
            x, y = moved(x, by), moved(y, by)
            sets = [] if removed is None else [moved(removed, by)]
            if self.at == "top":
                short_is_x = dc.blocks(x) <= dc.blocks(y)
                if self.source in TOP_IN_ONE_LIST:
                    if int(x[-1]) > int(y[-1]):
                        x = add_docs(x, [TOP])
                    else:
                        y = add_docs(y, [TOP])
                else:
                    x = add_docs(x, [TOP, TOP - 1] if short_is_x else [TOP])
                    y = add_docs(y, [TOP] if short_is_x else [TOP, TOP - 1])
                if sets:
                    hits = np.intersect1d(x, y, assume_unique=True)
                    sets.append(add_docs(sets[0], [TOP - 1, hits[hits < TOP - 1][-1]]))
            self._cache = (x, y, sets, by)
        return self._cache

    def source_coordinates(self):
        """(x, y, first removed set) moved back by the shift, the docs added at the top included: what the source case's own
        predicate is asked about"""
        x, y, sets, by = self.data()
        return moved(x, -by), moved(y, -by), (moved(sets[0], -by) if sets else None)

    def source_holds(self):
        x, y, r = self.source_coordinates()
        if self.module is dc:
            B, A = dc.roles(x, y)
            return all(bool(f(B, A, r)) for f in self.case.checks.values())
        lo, w = wc.result_words(x, y, r)
        return bool(self.case.check(x, y, r, lo, w))

    def third(self):
        """a third dense list over the pair's docs (mode 7), with the last doc id where the pair ends there"""
        x, y, _, _ = self.data()
        lo, hi = min(int(x[0]), int(y[0])), max(int(x[-1]), int(y[-1]))
        t = dc.bern(np.random.default_rng(zlib.crc32(self.name.encode())), 0.6, lo, hi + 1)
        return add_docs(t, [TOP]) if hi == TOP else t


EDGES = [Edge(m, s, at) for m, s, ats in SOURCES for at in ats]
BY_NAME = {e.name: e for e in EDGES}


def reference(lists, removed=None, union=False):
    want = lists[0]
    for l in lists[1:]:
        want = np.union1d(want, l) if union else np.intersect1d(want, l, assume_unique=True)
    if removed is not None:
        want = np.setdiff1d(want, removed, assume_unique=True)
    return want.astype(np.uint32)


def dense_driver(lists):
    """the AND chooser's streaming kernels take these lists: 2 - 4 of them, the one with the fewest blocks holds >= 1024 blocks at
    <= 1100 docs per block"""
    d = min(lists, key=dc.blocks)
    return 2 <= len(lists) <= 4 and dc.blocks(d) >= dc.MIN_BLOCKS and 0 < dc.docs_per_block(d) <= dc.MAX_DOCS_PER_BLOCK


def stream_pacer(lists):
    """the OR chooser's streaming kernel takes these lists (the ranking off): the one with the most blocks holds >= 1024 blocks at
    <= 1100 docs per block, and the lists reach at most a quarter of its span + 65536 docs beyond it"""
    p = max(lists, key=dc.blocks)
    own = int(p[-1]) - int(p[0]) + 1
    reach = max(int(l[-1]) for l in lists) - min(int(l[0]) for l in lists) + 1
    return 2 <= len(lists) <= 4 and dc.blocks(p) >= dc.MIN_BLOCKS and 0 < dc.docs_per_block(p) <= dc.MAX_DOCS_PER_BLOCK and reach <= own + own // 4 + 65536


def tomb_bitmap_words(removed):
    """words of the tombstone bitmap of a removed set: it ends with its last removed doc's word"""
    return (int(removed[-1]) >> 5) + 1


# ---- the family ------------------------------------------------------------------------------------------------------------------
FILL = 0xDEADBEEF
FUSED = ({"and.and2_fused": 1}, {"and.and2_fused": 1, "and.and2_split": 1})     # (a look-back wait that ran out repeats the call)
DEFAULTS = {"intersect.dense": 1, "intersect.and2": 1, "intersect.dense_bpw": 0, "intersect.dense_form": 1, "intersect.and2_tiles": 0,
            "intersect.and2_words": 1, "intersect.and2_words_min": 0, "union.rank": 1, "union.stream": 1, "debug.stamps": 0}


def fused_rows(B):
    """workgroups of the kernels that give a wave 16 blocks of the shorter list B - k_dense_tiles, k_and2_tiles, k_and2_fused at one
    tile a wave -: 64 blocks each"""
    return (dc.blocks(B) + dc.WG_BLOCKS - 1) // dc.WG_BLOCKS


@dataclass
class Mode:
    name: str
    options: dict
    paths: tuple                              # the path deltas the call may show
    rows: Optional[Callable] = None           # (B, A) -> workgroups of the mode's kernel (the rows of cycle counters it fills): two
    lists: str = "pair"                       # modes of one path differ in them.  lists: "pair", "three" or "union"
    forms: str = "as_before"                  # after the call: "none", "A" (A's and not B's), "both", or whatever was there before
    tombstones: bool = True


MODES = [
    Mode("dense2", {"intersect.and2": 0}, ({"and.dense2": 1},), lambda B, A: fused_rows(B)),
    Mode("dense2_bpw32", {"intersect.and2": 0, "intersect.dense_bpw": 32}, ({"and.dense2": 1},), lambda B, A: ((dc.blocks(B) + 31) // 32 + 3) // 4),
    Mode("split", {"intersect.and2": 2}, ({"and.and2_split": 1},), lambda B, A: fused_rows(B)),
    Mode("fused_marking", {"intersect.and2": 1, "intersect.dense_form": 0}, FUSED, lambda B, A: fused_rows(B), forms="none"),
    Mode("fused_form", {"intersect.and2": 1, "intersect.dense_form": 1, "intersect.and2_tiles": 1}, FUSED, lambda B, A: fused_rows(B), forms="A"),
    Mode("fused_form_x2", {"intersect.and2": 1, "intersect.dense_form": 1, "intersect.and2_tiles": 2}, FUSED, lambda B, A: (fused_rows(B) + 1) // 2, forms="A"),
    Mode("words", {"intersect.and2_words": 2}, FUSED, lambda B, A: wc.workgroups(B, A), forms="both"),
    Mode("dense3", {}, ({"and.dense3": 1},), lambda B, A: fused_rows(B), lists="three"),
    Mode("union", {"union.rank": 0}, ({"or.stream2": 1},), lists="union", tombstones=False),
]


@contextmanager
def options(ctx, values):
    try:
        for k, v in values.items():
            ctx.set_option(k, v)
        yield
    finally:
        for k in values:
            ctx.set_option(k, DEFAULTS[k])


def call(ctx, fn, ls, want, tomb, out, unmirrored=None):
    """one call into `out`, filled beforehand: the result is `want` bit for bit and nothing behind it was written; -> path delta.
    unmirrored: {id(segment): set of lists} for the segments that keep no host span mirror - the first call that names one of
    their lists fetches its span from the device (path span.fetch, once per list, counted here and taken out of the delta)"""
    from tests.gpu_util import path_delta
    fetch = 0
    for seg, i in ls:
        seen = (unmirrored or {}).get(id(seg))
        if seen is not None and i not in seen:
            seen.add(i)
            fetch += 1
    out.upload(np.full(out.count, FILL, np.uint32))
    with path_delta(ctx) as took:
        _, n = fn(ls, tomb=tomb, out=out)
    got = out.download()
    assert n == want.size, (n, want.size)
    assert got.dtype == np.uint32 and np.array_equal(got[:n], want)
    assert np.all(got[n:] == FILL), "ids written behind the result"
    assert took.pop("span.fetch", 0) == fetch, (took, fetch)
    return took


def stamp_rows(ctx, ls, tomb=None):
    """workgroups of the call's kernel, by the rows of cycle counters it fills (debug.stamps; cleared per call)"""
    import ctypes as C
    with options(ctx, {"debug.stamps": 1}):
        out, _ = ctx.intersect(ls, tomb=tomb)
        out.free()
        buf = (C.c_uint64 * (2048 * 8))()
        ctx._ck(ctx.lib.ii2_debug_read(ctx.h, buf, 2048 * 8))
    return int(np.count_nonzero(np.frombuffer(buf, dtype=np.uint64).reshape(-1, 8).sum(axis=1)))


def form_is(ref, l):
    seg, i = ref
    f = seg.dense_form(i)
    assert f is not None, i
    assert (f["origin"], f["n_words"]) == (dc.form_origin(l), dc.form_bytes(l) // 4)
    assert np.array_equal(f["words"], dc.form_words(l))
    return f


def no_form(ref):
    seg, i = ref
    return seg.dense_form(i, words=False) is None


def run_family(ctx, lists, ls, third, tombs=(), seen_through=None, words_ls=None, union_path=True, swapped=(), unmirrored=None, modes=MODES):
    """Every mode of the family on one pair.
      lists          (x, y, the third list) as numpy arrays, x and y in the order the query names them
      ls, third      [(segment, list)] of x and y, and the (segment, list) of the third list
      tombs          [(removed ids, the library's tombstones of them)]: the modes that take tombstones run once without and once
                     with each, mode by mode, so that what a mode says of the forms holds for all of its calls
      seen_through   [(ref of x, ref of y)]: every handle the forms must show through (default: ls itself)
      words_ls       the refs the `words` mode asks through, where they differ from ls (a view's parent)
      union_path     False: the pair is no case of the streaming OR (stream_pacer says so): any other path
      swapped        names of modes that also run with the pair named in the other order
      unmirrored     as call() takes it
    The pair's store must hold no form of x or y yet.  -> {mode name: [path deltas]}"""
    x, y, t = lists
    B, A = dc.roles(x, y)
    seen = seen_through or [tuple(ls)]
    seen = [(rx, ry) if B is x else (ry, rx) for rx, ry in seen]        # -> (ref of B, ref of A)
    out = ctx.empty(x.size + y.size + 64)
    took = {}
    try:
        for m in modes:
            arrays = [x, y, t] if m.lists == "three" else [x, y]
            refs = list(words_ls if m.name == "words" and words_ls else ls) + ([third] if m.lists == "three" else [])
            fn = ctx.union if m.lists == "union" else ctx.intersect
            runs = [(refs, removed, tomb) for removed, tomb in [(None, None)] + (list(tombs) if m.tombstones else [])]
            runs += [(refs[::-1], removed, tomb) for _, removed, tomb in runs if m.name in swapped]
            for refs, removed, tomb in runs:
                want = reference(arrays, removed, union=m.lists == "union")
                with options(ctx, m.options):
                    d = call(ctx, fn, refs, want, tomb, out, unmirrored)
                    took.setdefault(m.name, []).append(d)
                    if m.lists == "union" and not union_path:
                        assert d and not any(k.startswith("or.stream") for k in d), (m.name, d)
                    else:
                        assert d in m.paths, (m.name, removed is not None, d)
                    if m.rows is not None:
                        assert stamp_rows(ctx, refs, tomb) == m.rows(B, A), m.name
                for rb, ra in seen:
                    if m.forms == "none":
                        assert no_form(rb) and no_form(ra) and ra[0].dense_form_bytes() == 0 and rb[0].dense_form_bytes() == 0, m.name
                    elif m.forms == "A":
                        form_is(ra, A)
                        assert no_form(rb), m.name
                    elif m.forms == "both":
                        form_is(ra, A)
                        form_is(rb, B)
    finally:
        out.free()
    return took
