"""The table of kernel-path cases: for every path id the library counts (Context.paths(), include/ii2.h: ii2_ctx_paths) the
smallest input that reaches it, taken from the thresholds in csrc/setop.cpp, with the exact path delta that one call must show.

A case names its lists by index; a Layout spreads them over segments (one segment, two segments, one segment of 65537 lists)
and turns the indices into the (segment, list) pairs and list ranges the entry points take.  reference() is the plain numpy
answer in uint64.  tests/test_paths_cpu.py checks the table itself (coverage of every path id, references that are not
trivial), tests/test_gpu_paths.py runs it.

Thresholds the shapes come from (a DV1 block holds 256 postings, so a list of c postings owns ceil(c / 256) blocks):
  AND  small: <= 2048 postings in <= 128 blocks.  dense: 2 - 4 lists, driver (fewest blocks) >= 1024 blocks at <= 1100 docs per
       block.  split driver blocks (sub): 2+ lists and a driver of >= 8192 docs per block, or a one-block driver against a longest
       list of >= 64 blocks.  wide: 64 lists.  pair: two lists, no sparse driver.
  OR   small: <= 8192 postings in <= 128 blocks.  rank: <= 8 lists, <= 2^20 postings.  stream: 2 - 4 lists, longest >= 1024 blocks
       at <= 1100 docs per block.  tiles: >= 64 blocks, at most 2048 docs of the common range per posting.  else the merge passes.
  OR of ranges: more than 64 non-empty lists (or union.many = 1) go block by block, window by window.
No expectation depends on the CU count: where a chooser looks at it, the case forces the choice with the option.

Not reachable with segments the encoder writes, so not in the table: the 128 / 129 block boundary of the small kernels.  The
encoder fills every block of a list but the last, so n <= 64 lists of P postings own at most 64 + P / 256 blocks - 72 for the
AND's 2048 postings, 96 for the OR's 8192 - and the posting limit always bites first."""
import functools

import numpy as np

BIG_LISTS = 65537                 # more than ii2_seg::SPAN_MIRROR_MAX lists: such a segment mirrors no doc spans on the host
ALWAYS_MARK = 1 << 40             # intersect.ranges_mark: every filter pass marks (0: every pass probes)
BLOCK = 256
# the options the cases set, with the library's defaults (what the test restores)
DEFAULTS = {"intersect.and2": 1, "intersect.dense_bpw": 0, "intersect.map_docs": 0, "intersect.submax": 0, "intersect.wgs": 0,
            "union.rank": 1, "union.many": 0, "union.many_window_log2": 30, "intersect.ranges_mark": 64, "andnot.small": 1,
            "batch.tiny": 1, "batch.small": 1, "batch.groups": 1}
LAYOUTS = ("one", "two", "big")


def pick(rng, n, lo, hi):
    """n distinct ids of [lo, hi), ascending."""
    span = hi - lo
    assert 0 < n <= span
    if span <= 8_000_000:
        v = rng.permutation(span)[:n].astype(np.int64)
    else:
        v = np.unique(rng.integers(0, span, int(n * 1.25) + 64, dtype=np.int64))
        v = v[rng.permutation(v.size)[:n]]
        assert v.size == n
    return np.sort(v + lo).astype(np.uint32)


def with_ids(a, ids):
    return np.union1d(a, np.asarray(ids, np.uint32)).astype(np.uint32)


def sized(a, n, keep=()):
    """a cut to exactly n ids, those of `keep` among them."""
    keep = np.unique(np.asarray(keep, np.uint32))
    rest = np.setdiff1d(a, keep)
    k = n - keep.size
    assert 0 <= k <= rest.size
    rest = rest[np.unique(np.linspace(0, rest.size - 1, k).astype(np.int64))] if k else rest[:0]      # spread over a's whole range
    assert rest.size == k
    return np.union1d(rest, keep).astype(np.uint32)


# ---- builders (seeded; cached: cases that differ in their options share their lists) -------------------------------------
@functools.lru_cache(maxsize=None)
def uniform(seed, sizes, universe, lo=0):
    rng = np.random.default_rng(seed)
    return tuple(pick(rng, n, lo, lo + universe) for n in sizes)


@functools.lru_cache(maxsize=None)
def with_core(seed, sizes, universe, n_core):
    """Lists that share n_core ids (an AND of many random lists would be empty)."""
    rng = np.random.default_rng(seed)
    core = pick(rng, n_core, 0, universe)
    return tuple(sized(with_ids(pick(rng, n, 0, universe), core), n, core) for n in sizes)


@functools.lru_cache(maxsize=None)
def rare_term(seed, n_driver, universe=200_000, long_blocks=64):
    """A driver of n_driver postings against a list of exactly long_blocks blocks that lives in [1000, universe - 1000): the
    driver holds a candidate below the long list's first doc, one above its last, and every other one of its ids is a hit."""
    rng = np.random.default_rng(seed)
    long = pick(rng, long_blocks * BLOCK, 1000, universe - 1000)
    if n_driver == 1:
        return (long[4321:4322].copy(), long)
    hits = long[rng.permutation(long.size)[: n_driver // 2]]
    drv = with_ids(hits, [5, universe - 5])
    miss = np.setdiff1d(pick(rng, 4 * n_driver, 0, universe), long)
    drv = sized(with_ids(drv, miss), n_driver, with_ids(hits, [5, universe - 5]))
    assert drv.size == n_driver
    return (drv, long)


@functools.lru_cache(maxsize=None)
def wide_sub(seed):
    """64 lists: one block, 62 x three blocks, one of 64 blocks - the one-block driver against a long list."""
    rng = np.random.default_rng(seed)
    U = 200_000
    core = pick(rng, 40, 0, U)
    sizes = [200] + [700] * 62 + [64 * BLOCK]
    return tuple(sized(with_ids(pick(rng, n, 0, U), core), n, core) for n in sizes)


@functools.lru_cache(maxsize=None)
def windows(seed):
    """65 lists of 100 ids in [64, 64 + 5 * 2048): five windows of 2048 docs exactly."""
    rng = np.random.default_rng(seed)
    lo, hi = 64, 64 + 5 * 2048
    lists = [pick(rng, 100, lo, hi) for _ in range(65)]
    lists[0] = sized(with_ids(lists[0], [lo, hi - 1]), 100, [lo, hi - 1])
    return tuple(lists)


@functools.lru_cache(maxsize=None)
def whole_id_space(seed, n_lists, n):
    rng = np.random.default_rng(seed)
    lists = [pick(rng, n, 0, 1 << 32) for _ in range(n_lists)]
    lists[0] = sized(with_ids(lists[0], [0]), n, [0])
    lists[-1] = sized(with_ids(lists[-1], [0xFFFFFFFF]), n, [0xFFFFFFFF])
    return tuple(lists)


@functools.lru_cache(maxsize=None)
def stream(seed, m):
    """A pacer of exactly 1024 blocks at ~977 docs per block, then m - 1 lists of 50 000 ids in the same range."""
    return uniform(seed, (1024 * BLOCK,) + (50_000,) * (m - 1), 1_000_000)


def concat(*parts):
    return tuple(a for p in parts for a in p)


def batch_lists(seed):
    return concat(uniform(seed, (300, 300), 2000), uniform(seed + 1, (1500,) * 4, 100_000), uniform(seed + 2, (20_000, 20_000), 400_000))


def gbatch_lists(seed):
    return concat(uniform(seed, (200,) * 5, 1500), uniform(seed + 1, (1200,) * 5, 8000), uniform(seed + 2, (5000,) * 5, 30_000))


# ---- the cases ------------------------------------------------------------------------------------------------------------
class Case:
    """name; lists: () -> tuple of uint32 arrays; call: (entry point, arguments over list indices) -
         ("intersect", [i, ...])   ("union", [i, ...])   ("union_ranges", [(a, b), ...])
         ("intersect_ranges", [[(a, b), ...], ...])   ("andnot", groups, exclude)
         ("batch", [("and" | "or", [(a, b), ...]), ...])   ("gbatch", [(groups, exclude), ...])
       options: {option name: value} set around the call; expect: the exact delta of Context.paths() (paths not named: 0);
       tomb: the call takes tombstones (removed_ids()); cap: "exact" = the output buffer holds the result and no id more;
       big: None, or what the same call shows in addition when its lists live in a segment of BIG_LISTS lists;
       degenerate: None, or why the reference of this case cannot be smaller than its smallest operand."""

    def __init__(self, name, lists, call, expect, options=None, tomb=False, cap=None, big=None, degenerate=None):
        self.name, self.lists, self.call, self.expect = name, lists, call, dict(expect)
        self.options, self.tomb, self.cap, self.big, self.degenerate = dict(options or {}), tomb, cap, big, degenerate

    def expect_in(self, layout, repeat=False):
        e = dict(self.expect)
        if layout == "big":
            for k, v in self.big.items():
                if not (repeat and k == "span.fetch"):            # (the spans fetched by the first call are cached)
                    e[k] = e.get(k, 0) + v
        return e

    def layouts(self):
        return [l for l in LAYOUTS if l != "big" or self.big is not None]

    def __repr__(self):
        return self.name


def _both(name, lists, call, expect, **kw):
    """The case without and with tombstones."""
    return [Case(name, lists, call, expect, **kw), Case(name + "_tomb", lists, call, expect, tomb=True, **kw)]


def _cases():
    c = []
    PROBE, MARK = {"intersect.ranges_mark": 0}, {"intersect.ranges_mark": ALWAYS_MARK}
    # -- AND: the one-workgroup kernel and its posting limit
    c += _both("and_small_300", lambda: uniform(1, (300, 300), 2000), ("intersect", [0, 1]), {"and.small": 1}, big={})
    c += [Case("and_small_2048_postings", lambda: uniform(2, (1024, 1024), 6000), ("intersect", [0, 1]), {"and.small": 1}),
          Case("and_small_2049_postings_not_taken", lambda: uniform(3, (1024, 1025), 20_000), ("intersect", [0, 1]), {"and.tiles_pair": 1})]
    # -- AND: the dense forms at exactly 1024 driver blocks, ~977 docs per block
    dense = lambda k, blocks=1024: (lambda: uniform(4, (blocks * BLOCK,) * k, 1_000_000))
    c += [Case("and_and2_fused_1024_blocks", dense(2), ("intersect", [0, 1]), {"and.and2_fused": 1}, big={"span.fetch": 2}),
          Case("and_and2_split", dense(2), ("intersect", [0, 1]), {"and.and2_split": 1}, options={"intersect.and2": 2}),
          Case("and_dense2_and2_off", dense(2), ("intersect", [0, 1]), {"and.dense2": 1}, options={"intersect.and2": 0}),
          Case("and_dense2_bpw_32", dense(2), ("intersect", [0, 1]), {"and.dense2": 1}, options={"intersect.dense_bpw": 32}),
          Case("and_dense3", dense(3), ("intersect", [0, 1, 2]), {"and.dense3": 1}, tomb=True),
          Case("and_dense4", dense(4), ("intersect", [0, 1, 2, 3]), {"and.dense4": 1}),
          Case("and_dense_1023_blocks_not_taken", dense(2, 1023), ("intersect", [0, 1]), {"and.tiles_pair": 1}),
          Case("and_dense_5_lists_not_taken", dense(5), ("intersect", [0, 1, 2, 3, 4]), {"and.tiles": 1})]
    # -- AND: the tile kernel's instantiations
    pair = lambda: uniform(5, (20_000, 20_000), 400_000)                  # ~5000 docs per driver block
    c += _both("and_tiles_pair", pair, ("intersect", [0, 1]), {"and.tiles_pair": 1}, big={"span.fetch": 1})
    c += [Case("and_tiles_pair_every_tile_gallops", pair, ("intersect", [0, 1]), {"and.tiles_pair": 1}, options={"intersect.map_docs": 1}),
          Case("and_tiles_three_lists", lambda: uniform(5, (20_000,) * 3, 400_000), ("intersect", [0, 1, 2]), {"and.tiles": 1}),
          Case("and_tiles_sparse_driver_unsplit", lambda: uniform(6, (700, 20_000), 400_000), ("intersect", [0, 1]), {"and.tiles": 1},
               options={"intersect.submax": 1}),
          Case("and_tiles_workgroups_loop", lambda: uniform(7, (300 * BLOCK,) * 2, 1_500_000), ("intersect", [0, 1]), {"and.tiles_pair": 1},
               options={"intersect.wgs": 1}),
          Case("and_tiles_8_lists_shift_code", lambda: with_core(8, (700,) * 8, 12_000, 40), ("intersect", list(range(8))), {"and.tiles": 1}),
          Case("and_tiles_9_lists_counting_code", lambda: with_core(8, (700,) * 9, 12_000, 40), ("intersect", list(range(9))), {"and.tiles": 1})]
    for submax in (2, 3, 7, 16):                                          # slices per driver block that do not divide 256
        c.append(Case(f"and_tiles_sub_{submax}_slices", lambda: rare_term(9, 255), ("intersect", [0, 1]), {"and.tiles_sub": 1},
                      options={"intersect.submax": submax}))
    for nd in (1, 256, 257):
        c.append(Case(f"and_tiles_sub_driver_of_{nd}", lambda nd=nd: rare_term(9, nd), ("intersect", [0, 1]), {"and.tiles_sub": 1},
                      options={"intersect.submax": 3},
                      degenerate="a driver of one posting: the result is that posting" if nd == 1 else None))
    wide = lambda: with_core(10, (700,) * 64, 12_000, 40)                 # 64 lists x 3 blocks, < 6000 docs per driver block
    c += _both("and_tiles_wide", wide, ("intersect", list(range(64))), {"and.tiles_wide": 1})
    # list 0 cut to one block: the longest list has 3 blocks, not 64 - the chooser does not split the driver block
    c += [Case("and_tiles_wide_one_block_driver_short_lists", lambda: with_core(10, (200,) + (700,) * 63, 12_000, 40),
               ("intersect", list(range(64))), {"and.tiles_wide": 1})]
    c += _both("and_tiles_wide_sub", lambda: wide_sub(11), ("intersect", list(range(64))), {"and.tiles_wide_sub": 1})
    c += [Case("and_tiles_wide_sub_sparse_driver", lambda: with_core(12, (700,) * 64, 200_000, 40), ("intersect", list(range(64))),
               {"and.tiles_wide_sub": 1})]
    # -- OR
    c += [Case("or_small_8192_postings", lambda: uniform(13, (2048,) * 4, 100_000), ("union", [0, 1, 2, 3]), {"or.small": 1}, tomb=True),
          Case("or_rank_8193_postings", lambda: uniform(14, (2048, 2048, 2048, 2049), 100_000), ("union", [0, 1, 2, 3]), {"or.rank": 1}),
          Case("or_rank_8_lists", lambda: uniform(15, (1100,) * 8, 100_000), ("union", list(range(8))), {"or.rank": 1}, tomb=True),
          Case("or_9_lists_not_rank", lambda: uniform(15, (1000,) * 9, 100_000), ("union", list(range(9))), {"or.merge": 1}),
          Case("or_rank_off", lambda: uniform(16, (2100,) * 4, 100_000), ("union", [0, 1, 2, 3]), {"or.merge": 1}, options={"union.rank": 0})]
    for m in (2, 3, 4):
        c.append(Case(f"or_stream{m}", lambda m=m: stream(17, m), ("union", list(range(m))), {f"or.stream{m}": 1},
                      options={"union.rank": 0}, tomb=m == 3))
    c += _both("or_tiles_10_lists", lambda: uniform(18, (2000,) * 10, 100_000), ("union", list(range(10))), {"or.tiles": 1})
    c += _both("or_tiles_wide", wide, ("union", list(range(64))), {"or.tiles_wide": 1})
    c += [Case("or_merge_whole_id_space", lambda: whole_id_space(19, 9, 1000), ("union", list(range(9))), {"or.merge": 1}, tomb=True),
          Case("or_merge_too_sparse_for_tiles", lambda: whole_id_space(20, 9, 2000), ("union", list(range(9))), {"or.merge": 1})]
    # -- OR of list ranges
    few = lambda: uniform(21, (300, 900, 2000), 100_000)
    many = lambda: uniform(22, (100,) * 65, 1_000_000)
    c += [Case("ranges_few_lists_take_the_or_chooser", few, ("union_ranges", [(0, 3)]), {"or.small": 1}, big={}),
          Case("or_many_forced", few, ("union_ranges", [(0, 3)]), {"or.many": 1, "or.many_window": 1}, options={"union.many": 1},
               big={"span.bounds": 1})]
    c += _both("or_many_65_lists", many, ("union_ranges", [(0, 65)]), {"or.many": 1, "or.many_window": 1}, big={"span.bounds": 1})
    c += [Case("or_many_five_windows", lambda: windows(23), ("union_ranges", [(0, 65)]), {"or.many": 1, "or.many_window": 5},
               options={"union.many_window_log2": 11}, big={"span.bounds": 1}),
          Case("or_many_count_first", lambda: windows(23), ("union_ranges", [(0, 65)]), {"or.many": 1, "or.many_count_first": 1, "or.many_window": 10},
               options={"union.many_window_log2": 11}, cap="exact", tomb=True, big={"span.bounds": 1})]
    # -- AND of ORs
    g3 = lambda: uniform(24, (500,) * 6, 4000)
    groups3 = [[(0, 2)], [(2, 4)], [(4, 6)]]
    g4 = lambda: uniform(25, (400,) * 12, 4000)
    groups4 = [[(0, 3)], [(3, 6)], [(6, 9)], [(9, 12)]]
    c += [Case("ir_handoff", lambda: uniform(1, (300, 300), 2000), ("intersect_ranges", [[(0, 1)], [(1, 2)]]), {"ir.handoff": 1, "and.small": 1}, big={}),
          Case("ir_one_group_is_a_union", g3, ("intersect_ranges", [[(0, 2), (2, 4)]]), {"or.small": 1}, big={})]
    c += _both("ir_probe", g3, ("intersect_ranges", groups3), {"ir.groups": 1, "or.small": 1, "ir.probe": 2}, options=PROBE, big={"span.bounds": 3})
    c += _both("ir_mark", g3, ("intersect_ranges", groups3), {"ir.groups": 1, "or.small": 1, "ir.mark": 2}, options=MARK, big={"span.bounds": 3})
    c += [Case("ir_probe_4_groups_of_3", g4, ("intersect_ranges", groups4), {"ir.groups": 1, "or.small": 1, "ir.probe": 3}, options=PROBE,
               big={"span.bounds": 4}),
          Case("ir_mark_4_groups_of_3", g4, ("intersect_ranges", groups4), {"ir.groups": 1, "or.small": 1, "ir.mark": 3}, options=MARK,
               big={"span.bounds": 4})]
    # -- NOT
    an = lambda: uniform(26, (300,) * 6, 3000)
    an_call = ("andnot", [[(0, 2)], [(2, 4)]], [[(4, 6)]])
    heavy = lambda: uniform(27, (1200,) * 6, 12_000)                      # 7200 postings x 6 lists: above the default work bound
    general = lambda f, d: {"andnot.general": 1, "ir.groups": 1, "or.small": 1, f: 1, d: 1}
    c += _both("andnot_small", an, an_call, {"andnot.small": 1}, big={})
    c += [Case("andnot_small_above_the_work_bound", heavy, an_call, general("ir.probe", "ir.probe_drop"), options=PROBE, big={"span.bounds": 2}),
          Case("andnot_small_2_lifts_the_work_bound", heavy, an_call, {"andnot.small": 1}, options={"andnot.small": 2}, big={})]
    c += _both("andnot_general_probe", an, an_call, general("ir.probe", "ir.probe_drop"), options=dict(PROBE, **{"andnot.small": 0}),
               big={"span.bounds": 2})
    c += _both("andnot_general_mark", an, an_call, general("ir.mark", "ir.mark_drop"), options=dict(MARK, **{"andnot.small": 0}),
               big={"span.bounds": 2})
    # -- batches: a tiny query, a small one and one too large for the batch kernel
    bq = [("and", [(0, 2)]), ("or", [(2, 6)]), ("and", [(6, 8)])]
    bl = lambda: batch_lists(28)
    c += _both("batch_mixed", bl, ("batch", bq), {"batch.tiny": 1, "batch.small": 1, "batch.single": 1, "batch.pack": 1, "and.tiles_pair": 1},
               big={"span.fetch": 1})
    c += [Case("batch_tiny_off", bl, ("batch", bq), {"batch.small": 1, "batch.single": 1, "batch.pack": 1, "and.tiles_pair": 1},
               options={"batch.tiny": 0}, big={"span.fetch": 1}),
          Case("batch_small_off", bl, ("batch", bq), {"batch.single": 3, "batch.pack": 1, "and.small": 1, "or.small": 1, "and.tiles_pair": 1},
               options={"batch.small": 0}, big={"span.fetch": 1})]
    gq = [([[(0, 2)], [(2, 4)]], [[(4, 5)]]), ([[(5, 7)], [(7, 9)]], [[(9, 10)]]), ([[(10, 12)], [(12, 14)]], [[(14, 15)]])]
    gl = lambda: gbatch_lists(31)
    large = {"andnot.general": 1, "ir.groups": 1, "or.rank": 1, "ir.probe": 1, "ir.probe_drop": 1}
    c += _both("gbatch_mixed", gl, ("gbatch", gq), dict(large, **{"gbatch.tiny": 1, "gbatch.small": 1, "gbatch.single": 1, "gbatch.pack": 1}),
               options=PROBE, big={"span.bounds": 2})
    c += [Case("gbatch_tiny_off", gl, ("gbatch", gq), dict(large, **{"gbatch.small": 1, "gbatch.single": 1, "gbatch.pack": 1}),
               options=dict(PROBE, **{"batch.tiny": 0}), big={"span.bounds": 2}),
          Case("gbatch_groups_off", gl, ("gbatch", gq), dict(large, **{"gbatch.single": 3, "gbatch.pack": 1, "andnot.small": 2}),
               options=dict(PROBE, **{"batch.groups": 0}), big={"span.bounds": 2})]
    names = [x.name for x in c]
    assert len(set(names)) == len(names), "case names are unique"
    return c


CASES = _cases()

# paths that no call through the ABI can reach (name -> why); the CPU test allows three at the most
UNREACHABLE = {}


# ---- layouts -------------------------------------------------------------------------------------------------------------
class Layout:
    """Where the lists of a case live: segments[s] = the lists of segment s; list i is list at[i][1] of segment at[i][0]."""

    def __init__(self, kind, lists):
        self.kind = kind
        n = len(lists)
        if kind == "two":
            self.segments = [list(lists[0::2]), list(lists[1::2])]
            self.at = [(i % 2, i // 2) for i in range(n)]
        else:
            self.segments = [list(lists)]
            self.at = [(0, i) for i in range(n)]
        self.n_lists = [BIG_LISTS] if kind == "big" else [len(s) for s in self.segments]

    def flat(self, s):
        """(post_off u64 [n_lists + 1], values u32) of segment s as ii2_seg_encode takes them (the big layout: the lists, then
        empty ones)."""
        seg = self.segments[s]
        off = np.zeros(self.n_lists[s] + 1, np.uint64)
        sizes = np.array([a.size for a in seg], np.uint64)
        off[1: len(seg) + 1] = np.cumsum(sizes)
        off[len(seg) + 1:] = off[len(seg)]
        return off, (np.concatenate(seg) if seg else np.empty(0, np.uint32))

    def pairs(self, idx):
        return [self.at[i] for i in idx]

    def ranges(self, rs):
        """The list ranges [(a, b), ...] as ranges of the segments: [(segment, first, end), ...]."""
        out = []
        for a, b in rs:
            if self.kind == "two":
                out += [(s, lo, hi) for s, lo, hi in ((0, (a + 1) // 2, (b + 1) // 2), (1, a // 2, b // 2)) if hi > lo]
            else:
                out.append((0, a, b))
        return out


# ---- the reference ---------------------------------------------------------------------------------------------------------
def _or(lists, rs):
    out = np.empty(0, np.uint64)
    for a, b in rs:
        for l in lists[a:b]:
            out = np.union1d(out, l.astype(np.uint64))
    return out


def _and_of_ors(lists, groups, exclude=()):
    out = None
    for g in groups:
        u = _or(lists, g)
        out = u if out is None else np.intersect1d(out, u)
    for g in exclude:
        out = np.setdiff1d(out, _or(lists, g))
    return out


def operands(case, lists):
    """Per query of the call: ("and" | "or", the arrays it combines - an AND's required groups as their unions)."""
    kind, *args = case.call
    one = lambda i: lists[i].astype(np.uint64)
    if kind == "intersect":
        return [("and", [one(i) for i in args[0]])]
    if kind == "union":
        return [("or", [one(i) for i in args[0]])]
    if kind == "union_ranges":
        return [("or", [one(i) for a, b in args[0] for i in range(a, b)])]
    if kind == "intersect_ranges":
        return [("and", [_or(lists, g) for g in args[0]])] if len(args[0]) > 1 else [("or", [one(i) for a, b in args[0][0] for i in range(a, b)])]
    if kind == "andnot":
        return [("and", [_or(lists, g) for g in args[0]])]
    if kind == "batch":
        return [(op, [one(i) for a, b in rs for i in range(a, b)]) for op, rs in args[0]]
    if kind == "gbatch":
        return [("and", [_or(lists, g) for g in groups]) for groups, _ in args[0]]
    raise ValueError(kind)


def reference(case, lists, removed=None):
    """The results of the call's queries (one but for the batches), uint64, without or minus the removed ids."""
    kind, *args = case.call
    if kind == "intersect":
        res = [functools.reduce(np.intersect1d, [lists[i].astype(np.uint64) for i in args[0]])]
    elif kind == "union":
        res = [functools.reduce(np.union1d, [lists[i].astype(np.uint64) for i in args[0]])]
    elif kind == "union_ranges":
        res = [_or(lists, args[0])]
    elif kind == "intersect_ranges":
        res = [_and_of_ors(lists, args[0])]
    elif kind == "andnot":
        res = [_and_of_ors(lists, args[0], args[1])]
    elif kind == "batch":
        # (an "and" takes every list of its ranges as one operand)
        res = [_and_of_ors(lists, [[(i, i + 1)] for a, b in rs for i in range(a, b)]) if op == "and" else _or(lists, rs) for op, rs in args[0]]
    elif kind == "gbatch":
        res = [_and_of_ors(lists, groups, exclude) for groups, exclude in args[0]]
    else:
        raise ValueError(kind)
    if removed is not None:
        res = [np.setdiff1d(r, removed.astype(np.uint64)) for r in res]
    return res


def removed_ids(case, lists):
    """The tombstones of a case: every third id of each result, and as many ids again that are in none."""
    res = reference(case, lists)
    hit = np.unique(np.concatenate([r[::3] for r in res]))
    everything = np.unique(np.concatenate([l.astype(np.uint64) for l in lists]))
    miss = np.setdiff1d(everything, np.concatenate(res))[:: max(1, everything.size // max(hit.size, 1))]
    return np.union1d(hit, miss).astype(np.uint32)
