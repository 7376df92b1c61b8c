"""The table of merge cases: for every decision of the segment merge's plan and every recovery of its tile kernel the smallest
input that reaches it, with the tile count the plan must arrive at and the exact delta of Context.merge_events() one call must
show (include/ii2.h: ii2_merge_events).

plan() restates the arithmetic of the plan kernels (merge.hip: k_mp_terms / k_mp_terms_few, k_merge_heads, k_merge_tile_desc) in
plain numpy, simulate() the recovery inside k_merge_tiles: which batches overflow a bucket and are redone term by term, which doc
ranges are bisected and why, and how the leaves of a bisection are merged.  Both work on the lists alone; neither knows what the
library answers.  tests/test_merge_cases_cpu.py checks the table itself (every event and every plan branch reached, both sides of
every threshold differ in the tile count, hand-counted events of the fallback cases, references that are not trivial),
tests/test_gpu_merge_cases.py runs it.

The thresholds, read once (a DV1 block holds 256 postings):
  MERGE_CAP, MERGE_NT_MAX, MERGE_BM_WORDS, MERGE_BM_DOCS         csrc/internal.h:619-622
  small_max, batch_q, wmin, range_target, bitmap sparsity          csrc/ops.cpp:54-59 (merge_core)
  k >= 32: k_merge_tile_runs_shared, else k_merge_tile_runs_few    csrc/ops.cpp:121 (cut_st), csrc/merge.hip: launch_merge_tile_runs
  n_terms < 65536: k_mp_terms_few, else k_mp_terms                 csrc/merge.hip:1560 (launch_merge_plan_terms)
  small / large, bitmap / range, splitters, extra tiles            csrc/merge.hip:83-103 (k_mp_terms), 154-174 (k_mp_terms_few)
  batch heads                                                      csrc/merge.hip: k_merge_heads
  BKT_LIMIT, the bucket maps, the bisection, its bitmap leaves     csrc/merge.hip:42, k_merge_tiles ("bucket maps", line 1014: BM)

Not reachable, so not in the table: a batch of MERGE_NT_MAX = 256 terms.  A batch is the small terms whose exclusive weight
prefixes share one multiple of batch_q, every term weighs at least wmin = 14, so a batch holds at most ceil(2304 / 14) = 165 terms:
the case of 257 one-posting terms pins that number instead."""
import functools

import numpy as np

BLOCK = 256
MERGE_CAP = 3584
MERGE_NT_MAX = 256
MERGE_BM_DOCS = 2 * MERGE_CAP * 32                     # 229376
SMALL_MAX = MERGE_CAP * 5 // 14                        # 1280
BATCH_Q = MERGE_CAP - SMALL_MAX                        # 2304
WMIN = (MERGE_CAP + MERGE_NT_MAX - 1) // MERGE_NT_MAX  # 14
RANGE_TARGET = MERGE_CAP // 20 * 19                    # 3401
SPARSITY = 80
BKT_LIMIT = 15
FEW_TERMS = 65536
SHARED_RUNS_K = 32
TOP = 0xFFFFFFFF
EVENTS = ("batch_redo", "range_overfull", "range_bucket_overflow", "leaf_bitmap", "leaf_sorted")
BRANCHES = ("small", "large", "empty_term", "bitmap", "range", "block_cuts", "uniform_splitters", "extra_tile", "one_tile_range",
            "head_first", "head_after_large", "head_weight", "terms_few", "terms_many", "runs_few", "runs_shared")
# the options the cases set, with the library's defaults (what the test restores)
DEFAULTS = {"merge.direct": 1, "merge.large_tile": 0}
# events no case reaches deterministically: {name: reason}; at most one may be listed
UNREACHABLE = {}


# ---- segments: k term-aligned CSR pairs (off u64[T + 1], vals u32) --------------------------------------------------------
def csr(lists):
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    vals = np.concatenate([np.asarray(l, np.uint32) for l in lists] + [np.empty(0, np.uint32)]).astype(np.uint32)
    return off, vals


def lists_of(segs, t):
    return [v[int(o[t]):int(o[t + 1])] for o, v in segs]


def ap(n, lo, step):
    """n ids from lo on, step apart."""
    return (lo + step * np.arange(n, dtype=np.int64)).astype(np.uint32)


# ---- the plan -------------------------------------------------------------------------------------------------------------
class Plan:
    pass


def plan(segs, range_target=RANGE_TARGET):
    """What the plan kernels decide for k aligned segments: per term n, mn, mx, the longest list and its blocks, small / bitmap /
    range, the tiles of a large term, the batch heads, and n_tiles = heads + tiles of the large terms."""
    k, T = len(segs), len(segs[0][0]) - 1
    sizes = np.stack([np.diff(o.astype(np.int64)) for o, _ in segs])                      # [k, T]
    first = np.full((k, T), TOP, np.int64)
    last = np.zeros((k, T), np.int64)
    for s, (o, v) in enumerate(segs):
        ne = sizes[s] > 0
        first[s, ne] = v[o[:-1][ne].astype(np.int64)]
        last[s, ne] = v[o[1:][ne].astype(np.int64) - 1]
    p = Plan()
    p.k, p.T, p.range_target = k, T, range_target
    p.n = sizes.sum(0)
    p.mn, p.mx = first.min(0), last.max(0)
    p.mn[p.n == 0] = 0
    p.mx = np.maximum(p.mx, p.mn)
    nb = (sizes + BLOCK - 1) // BLOCK
    p.best_nb = nb.max(0) if T else np.zeros(0, np.int64)
    p.best = nb.argmax(0) if T else np.zeros(0, np.int64)                                  # the first of the longest lists
    p.large = p.n > SMALL_MAX
    p.weight = np.where(p.large, 0, np.maximum(p.n, WMIN))                                 # (empty terms weigh wmin too)
    p.tiles = np.zeros(T, np.int64)
    p.bitmap = np.zeros(T, bool)
    p.uniform = np.zeros(T, bool)
    p.extra = np.zeros(T, np.int64)
    for t in np.flatnonzero(p.large):
        n, nbt = int(p.n[t]), int(p.best_nb[t])
        span = int(p.mx[t]) - (int(p.mn[t]) & ~31) + 1
        if span <= n * SPARSITY:
            p.bitmap[t] = True
            p.tiles[t] = (span + MERGE_BM_DOCS - 1) // MERGE_BM_DOCS
            continue
        tiles = (n + range_target - 1) // range_target
        if nbt < 2 * tiles:
            p.uniform[t] = True
        else:
            for _ in range(2):                                                              # "up to two tiles more"
                most = (nbt + tiles - 1) // tiles
                if n * most <= range_target * nbt:
                    break
                tiles += 1
                p.extra[t] += 1
        p.tiles[t] = tiles
    wpre = np.concatenate([[0], np.cumsum(p.weight)])[:-1] if T else np.zeros(0, np.int64)
    prev_large = np.concatenate([[True], p.large[:-1]]) if T else np.zeros(0, bool)        # (term 0 counts as "after a large term")
    crossed = np.concatenate([[False], wpre[1:] // BATCH_Q != wpre[:-1] // BATCH_Q]) if T else np.zeros(0, bool)
    p.head = ~p.large & (prev_large | crossed)
    p.n_tiles = int(p.head.sum() + p.tiles.sum())
    # the batches: [first term, last term] of every run of small terms a head opens
    p.batches = []
    for t in range(T):
        if p.head[t]:
            p.batches.append([t, t])
        elif not p.large[t]:
            p.batches[-1][1] = t
    b = set()
    if np.any(~p.large & (p.n > 0)): b.add("small")
    if np.any(p.n == 0): b.add("empty_term")
    if np.any(p.large): b.add("large")
    if np.any(p.bitmap): b.add("bitmap")
    rng_t = p.large & ~p.bitmap
    if np.any(rng_t): b.add("range")
    if np.any(rng_t & p.uniform & (p.tiles > 1)): b.add("uniform_splitters")
    if np.any(rng_t & ~p.uniform & (p.tiles > 1)): b.add("block_cuts")
    if np.any(rng_t & (p.tiles == 1)): b.add("one_tile_range")
    if np.any(p.extra > 0): b.add("extra_tile")
    if T and p.head[0]: b.add("head_first")
    if np.any(p.head[1:] & p.large[:-1]): b.add("head_after_large")
    if np.any(p.head[1:] & ~p.large[:-1]): b.add("head_weight")
    b.add("terms_few" if T < FEW_TERMS else "terms_many")
    if p.n_tiles: b.add("runs_shared" if k >= SHARED_RUNS_K else "runs_few")
    p.branches = b
    return p


def tile_ranges(p, segs, t):
    """[(dlo, dhi) or None] of the tiles of range term t (k_merge_tile_desc): None = an empty doc range."""
    m, mn, mx = int(p.tiles[t]), int(p.mn[t]), int(p.mx[t])
    if m == 1:
        return [(0, TOP)]
    if p.uniform[t]:
        cut = [0] + [mn + (j * (mx - mn + 1)) // m for j in range(1, m)] + [1 << 32]
    else:
        firsts = lists_of(segs, t)[int(p.best[t])][::BLOCK].astype(np.int64)
        cut = [0] + [int(firsts[(j * firsts.size) // m]) for j in range(1, m)] + [1 << 32]
    return [(cut[j], cut[j + 1] - 1) if cut[j + 1] > cut[j] else None for j in range(m)]


# ---- the recovery inside the tile kernel ------------------------------------------------------------------------------------
def _f32(x):
    return np.float32(x)


def _overflows(buckets):
    """A bucket takes a 17th posting (its slot number would be BKT_LIMIT + 1)."""
    return buckets.size > 0 and int(np.bincount(buckets).max()) > BKT_LIMIT + 1


def _range_buckets(v, lo, hi, tmn, tmx):
    """The bucket of every id of a doc range of one term: MERGE_CAP buckets over the range's part of the term's docs, in float."""
    u_mn, mxr = max(lo, tmn), min(hi, tmx)
    scale = _f32(MERGE_CAP) / (_f32(max(mxr, u_mn) - u_mn) + _f32(1))
    bq = ((v.astype(np.int64) - u_mn).astype(np.float32) * scale).astype(np.int64)
    return np.minimum(bq, MERGE_CAP - 1)


def _blocks_of_range(firsts, b_lo, b_hi, dlo, dhi):
    """merge.hip blocks_of_range: from the last block that starts at or before dlo to the last one that starts at or before dhi."""
    if b_hi <= b_lo or dlo > dhi:
        return b_lo, b_lo
    a = b_lo + int(np.searchsorted(firsts[b_lo:b_hi], dlo, "right"))
    b1 = b_hi if dhi == TOP else a + int(np.searchsorted(firsts[a:b_hi], dhi, "right"))
    return (a - 1 if a > b_lo else b_lo), b1


def _bisect(ev, lists, runs, lo, hi, tmn, tmx):
    """One root doc range of one term: lists = its k id arrays, runs = [(first block, end block)] of every list for the root.
    Counts the events of the root and of everything it is bisected into."""
    firsts = [l[::BLOCK].astype(np.int64) for l in lists]
    stack = [(lo, hi, True)]
    while stack:
        lo, hi, root = stack.pop()
        if root:
            nblk = sum(b1 - b0 for b0, b1 in runs)
        else:
            nblk = sum(b1 - b0 for b0, b1 in (_blocks_of_range(f, r0, r1, lo, hi) for f, (r0, r1) in zip(firsts, runs)))
        if nblk == 0:
            continue
        if not root and hi - (lo & ~31) < MERGE_BM_DOCS:
            ev["leaf_bitmap"] += 1
            continue
        v = np.concatenate([l[(l >= lo) & (l <= hi)] for l in lists])
        if v.size > MERGE_CAP:
            ev["range_overfull"] += 1
        elif _overflows(_range_buckets(v, lo, hi, tmn, tmx)):
            ev["range_bucket_overflow"] += 1
        else:
            if not root:
                ev["leaf_sorted"] += 1
            continue
        mid = lo + ((hi - lo) >> 1)
        stack += [(mid + 1, hi, False), (lo, mid, False)]


def _cut_block(l, x):
    """Blocks in front of the cut before the first posting >= x (k_merge_tile_runs*), and whether the cut is inside a block."""
    pos = int(np.searchsorted(l, x, "left"))
    nb = (l.size + BLOCK - 1) // BLOCK
    if pos == l.size:
        return nb, False
    return pos // BLOCK, pos % BLOCK != 0


def simulate(segs, p):
    """{event: count} of one merge of the segments under plan p."""
    ev = dict.fromkeys(EVENTS, 0)
    # -- batches: term t of a batch of n postings owns floor(n_t * MERGE_CAP / n) buckets over [mn_t, mx_t]
    small = ~p.large
    bid = np.cumsum(p.head) - 1                                                             # batch of every small term
    nbat = len(p.batches)
    if nbat:
        n_b = np.bincount(bid[small], weights=p.n[small], minlength=nbat).astype(np.int64)
        nbk = np.zeros(p.T, np.int64)
        nbk[small] = p.n[small] * MERGE_CAP // np.maximum(n_b[bid[small]], 1)
        cum = np.concatenate([[0], np.cumsum(nbk)])
        tb = cum[:-1] - cum[[a for a, _ in p.batches]][np.maximum(bid, 0)]                 # first bucket of every term inside its batch
        den = (p.mx - p.mn).astype(np.float32) + _f32(1)
        scale = np.where(nbk > 0, nbk.astype(np.float32) / den, _f32(0)).astype(np.float32)
        keys = []
        for o, v in segs:
            term = np.repeat(np.arange(p.T), np.diff(o.astype(np.int64)))
            keep = small[term]
            term, v = term[keep], v[keep].astype(np.int64)
            bq = ((v - p.mn[term]).astype(np.float32) * scale[term]).astype(np.int64)
            keys.append(bid[term] * MERGE_CAP + tb[term] + np.minimum(bq, nbk[term] - 1))
        keys = np.concatenate(keys)
        over = np.unique(keys[np.isin(keys, np.flatnonzero(np.bincount(keys) > BKT_LIMIT + 1))] // MERGE_CAP) if keys.size else []
        for b in over:
            ev["batch_redo"] += 1
            for t in range(p.batches[b][0], p.batches[b][1] + 1):                          # term by term: whole lists, all docs
                lists = lists_of(segs, t)
                _bisect(ev, lists, [(0, (l.size + BLOCK - 1) // BLOCK) for l in lists], 0, TOP, int(p.mn[t]), int(p.mx[t]))
    # -- range tiles of the large terms (a bitmap tile never leaves its path)
    for t in np.flatnonzero(p.large & ~p.bitmap):
        lists = lists_of(segs, t)
        for r in tile_ranges(p, segs, t):
            if r is None:
                continue
            lo, hi = r
            runs = []
            for l in lists:
                bs = 0 if lo == 0 else _cut_block(l, lo)[0]
                if hi == TOP:
                    be = (l.size + BLOCK - 1) // BLOCK
                else:
                    blk, inside = _cut_block(l, hi + 1)
                    be = blk + (1 if inside else 0)
                runs.append((bs, max(be, bs)))
            _bisect(ev, lists, runs, lo, hi, int(p.mn[t]), int(p.mx[t]))
    return {k: v for k, v in ev.items() if v}


# ---- the cases --------------------------------------------------------------------------------------------------------------
class Case:
    """name; segs: () -> the k segments (CSR pairs); removed: () -> ids to tombstone (the case also runs without); options:
    {option: value} set around the call; union: the case is ONE term whose k lists are also unioned through ii2_union (the
    merge passes: 'or.merge'); encoding: also compare ii2_merge_segments_to_seg byte for byte with the DV1 encoding of the
    reference; pair: name of the case on the other side of the same threshold (their tile counts must differ), or a (name, "same")
    pair whose results and tile counts must agree."""

    def __init__(self, name, segs, removed, options=None, union=False, encoding=False, pair=None, same=None):
        self.name, self._segs, self._removed = name, segs, removed
        self.options, self.union, self.encoding, self.pair, self.same = dict(options or {}), union, encoding, pair, same

    @functools.lru_cache(maxsize=None)
    def segs(self):
        return self._segs()

    def removed(self):
        return np.unique(np.asarray(self._removed(self.segs()), np.uint32))

    @functools.lru_cache(maxsize=None)
    def plan(self):
        return plan(self.segs(), min(self.options.get("merge.large_tile", 0), MERGE_CAP) or RANGE_TARGET)

    @functools.lru_cache(maxsize=None)
    def events(self):
        return simulate(self.segs(), self.plan())

    def __repr__(self):
        return self.name


def reference(segs, removed=None):
    """The merge in plain numpy, uint64: per term the sorted union of the k lists minus the removed ids.  (off u64[T + 1], ids)"""
    T = len(segs[0][0]) - 1
    rem = np.asarray(removed if removed is not None else [], np.uint64)
    out, off = [], [0]
    for t in range(T):
        u = np.unique(np.concatenate([l.astype(np.uint64) for l in lists_of(segs, t)]))
        if rem.size:
            u = u[~np.isin(u, rem)]
        out.append(u)
        off.append(off[-1] + u.size)
    return np.array(off, np.uint64), np.concatenate(out + [np.empty(0, np.uint64)])


def _every_nth(n, start=3):
    """Tombstones: every n-th id of the merged lists."""
    def f(segs):
        allv = np.unique(np.concatenate([v for _, v in segs]))
        return allv[start::n]
    return f


def _terms(*per_term):
    """k segments from per-term tuples of k lists."""
    k = len(per_term[0])
    return [csr([term[s] for term in per_term]) for s in range(k)]


E = np.empty(0, np.uint32)


def _small_large(n_mid):
    """A term of n_mid postings (two lists, 1000 docs apart: far too sparse for the bitmap) between two small terms."""
    a = n_mid // 2
    return lambda: _terms((ap(10, 5, 7), ap(10, 6, 7)), (ap(a, 100, 1000), ap(n_mid - a, 600, 1000)), (ap(9, 50, 3), ap(9, 51, 3)))


def _one_range_term(sizes):
    """One range term: every list spread evenly over the same 4M docs."""
    return lambda: _terms(tuple(ap(n, 17 + 11 * s, 4_000_000 // n) for s, n in enumerate(sizes)))


def _span_term(n, mn, mx):
    """One term of n postings in two lists whose docs run from mn to mx exactly."""
    def f():
        ids = np.unique(np.linspace(mn, mx, n).astype(np.int64))
        assert ids.size == n and ids[0] == mn and ids[-1] == mx
        return _terms((ids[0::2].astype(np.uint32), ids[1::2].astype(np.uint32)))
    return f


def _one_block_lists(k=64, n=200):
    """k one-block lists spread evenly over 4M docs: four range tiles, splitters uniform in doc space."""
    return lambda: _terms(tuple(ap(n, 1000 + 311 * s, 20_000) for s in range(k)))


def _one_posting_terms(T):
    return lambda: _terms(*[(np.array([100 + 3 * t], np.uint32), np.array([100 + 3 * t + (t & 1)], np.uint32)) for t in range(T)])


def _weights(sizes):
    """Small terms of the given sizes (two lists each; the second repeats a few ids of the first in a third segment)."""
    def f():
        terms = []
        for t, n in enumerate(sizes):
            a = n // 2
            terms.append((ap(a, 10 + t, 50), ap(n - a, 35 + t, 50)))
        return _terms(*terms)
    return f


def _empties():
    """Empty terms first, last and between; a term that only some segments hold."""
    def f():
        a, b, c = ap(10, 5, 9), ap(12, 7, 9), ap(8, 500, 2)
        return _terms((E, E, E), (a, E, b), (E, E, E), (E, c, E), (b, a, c), (E, E, E))
    return f


def _interrupted():
    """A bitmap term and a range term interrupt a run of small ones."""
    def f():
        s = lambda t: (ap(20, 10 + t, 5), ap(20, 12 + t, 5))
        dense = (ap(1500, 64, 2), ap(1500, 65, 2))
        sparse = (ap(700, 9, 5000), ap(700, 11, 5000))
        return _terms(s(0), s(1), dense, s(2), sparse, s(3), s(4))
    return f


@functools.lru_cache(maxsize=None)
def _dictionary(T):
    """k = 20 segments over T terms (the 16 sub-lanes of k_mp_terms_few take two rounds): most terms hold one to three postings
    in a few segments, many none; three large terms whose longest list is tied between two segments (3 and 19, 5 and 17, 0 and
    16: the first must win) - and term T - 1 empty when T = 65536, so that both term counts merge the same lists."""
    rng = np.random.default_rng(65535)
    T0, k = FEW_TERMS - 1, 20
    big = {100: (3, 19), 30_000: (5, 17), 65_000: (0, 16)}
    segs = []
    for s in range(k):
        sizes = np.where(rng.random(T0) < 0.12, rng.integers(1, 4, T0), 0)
        for t, pair in big.items():
            sizes[t] = 1900 if s in pair else (300 if s == 9 else 0)
        if T > T0:
            sizes = np.concatenate([sizes, [0]])
        term = np.repeat(np.arange(sizes.size), sizes)
        j = np.arange(term.size) - np.repeat(np.cumsum(sizes) - sizes, sizes)                # index inside the list
        step = np.where(np.isin(term, list(big)), 997, 5)
        vals = (term * 7919) % 1_000_003 + step * j + (s % 4) * np.where(step == 5, 1, 331)
        segs.append((np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64), vals.astype(np.uint32)))
    return segs


def _cut_lists(k):
    """One range term of k three-block lists over 4M docs, ids shared between neighbouring lists."""
    def f():
        rng = np.random.default_rng(31)
        base = np.sort(rng.choice(4_000_000, 64 * 300, replace=False)).astype(np.uint32)
        lists = []
        for s in range(k):
            own = base[s::64]
            nxt = base[(s + 1) % 64::64][::3]
            lists.append(np.unique(np.concatenate([own, nxt, ap(200, 7 + 97 * s, 19_001)])).astype(np.uint32))
            assert 2 * BLOCK < lists[-1].size <= 3 * BLOCK
        return _terms(tuple(lists))
    return f


FOLD_IDS = ap(40, 5000, 3000)            # the list that k segments share: 40 ids 3000 docs apart
SPARSE_IDS = ap(500, 77, 100_003)        # ... as a sparse large term: 500 ids over 50M docs


def _fold_small(k):
    """The same list in k segments as a small term inside a batch of ordinary terms, an empty term on each side."""
    def f():
        o = lambda t, s: ap(30, 1000 * t + s, 11) if s < 3 else E
        terms = [tuple(o(t, s) for s in range(k)) for t in (1, 2)] + [(E,) * k, (FOLD_IDS,) * k, (E,) * k] + \
                [tuple(o(t, s) for s in range(k)) for t in (3, 4)]
        return _terms(*terms)
    return f


def _fold_large(k):
    """... as the one term of k segments; the first two also hold a few ids of their own (the result is none of the inputs)."""
    own = lambda s: np.union1d(SPARSE_IDS, ap(10, 1_050_000 + s, 4_000_001)).astype(np.uint32)
    return lambda: _terms((own(0), own(1)) + (SPARSE_IDS,) * (k - 2))


def clustered_geometry():
    """The clustered case's numbers: 64 one-block lists whose ids lie in the first quarter of the term's doc span, one outlier at
    its end.  mn = 9, span = 1.6M docs: four tiles of 400 000 docs (uniform splitters); the first holds every id but the outlier,
    more than MERGE_CAP: it is bisected once, and both halves are narrower than MERGE_BM_DOCS - bitmap leaves with bounds that
    are no multiples of 32."""
    mn, span = 9, 1_600_000
    t0_hi = mn + span // 4 - 1                      # tile 0 = [0, t0_hi]
    mid = t0_hi >> 1                                # leaves [0, mid] and [mid + 1, t0_hi]
    return mn, mn + span - 1, t0_hi, mid


def _clustered():
    def f():
        mn, mx, t0_hi, mid = clustered_geometry()
        lists = [ap(199, 1000 + 31 * s, 2000) for s in range(64)]
        assert max(int(l[-1]) for l in lists) < t0_hi - 64
        w_mid, w_end = mid & ~31, t0_hi & ~31                                                # the words the leaves' bounds fall into
        lists[0] = np.union1d(lists[0], [mx]).astype(np.uint32)                              # the outlier
        lists[3] = np.union1d(lists[3], [mn, w_mid, mid, w_end]).astype(np.uint32)         # first doc; last word of leaf 1; last word of leaf 2
        lists[5] = np.union1d(lists[5], [mid + 1, w_mid + 31, t0_hi, t0_hi + 1, w_end + 31]).astype(np.uint32)  # first word of leaf 2; first word of tile 1
        assert all(l.size <= BLOCK for l in lists)
        return _terms(tuple(lists))
    return f


def _clustered_removed(segs):
    """One tombstone in the first and one in the last word of leaf 1, one in the first word of leaf 2 (the same word), and the
    largest one inside leaf 2: the tombstone bitmap ends there, every id behind it survives."""
    mn, mx, t0_hi, mid = clustered_geometry()
    inside = lists_of(segs, 0)[7]
    inside = int(inside[(inside > mid + 5000) & (inside < t0_hi - 5000)][3])
    return [mn, mid & ~31, mid + 1, inside]


def _top_cluster():
    """A term over the whole id space, 20 ids inside the last 2^20 docs below 2^32: the float bucket map rounds their distance
    from the first doc up to 2^32, the bucket number to MERGE_CAP - one past the last bucket, which the clamp must catch."""
    def f():
        a = ap(700, 0, 6_000_000)
        b = np.union1d(ap(700, 1, 6_000_000), (TOP - 50_000 * np.arange(20, dtype=np.int64))).astype(np.uint32)
        return _terms((a, b))
    return f


def _cases():
    none = lambda segs: []
    nth = _every_nth(7)
    c = []
    # -- plan thresholds
    c += [Case("small_at_small_max", _small_large(SMALL_MAX), nth, pair="large_at_small_max_plus_1"),
          Case("large_at_small_max_plus_1", _small_large(SMALL_MAX + 1), nth),
          Case("range_at_target", _one_range_term((1700, RANGE_TARGET - 1700)), nth, pair="range_at_target_plus_1"),
          Case("range_at_target_plus_1", _one_range_term((1700, RANGE_TARGET + 1 - 1700)), nth),
          Case("seven_blocks_take_a_third_tile", _one_range_term((1700,) * 4), nth, pair="eight_blocks_stay_at_two_tiles"),
          Case("eight_blocks_stay_at_two_tiles", _one_range_term((2048, 1600, 1600, 1552)), nth),
          Case("bitmap_at_span_80n", _span_term(3000, 1000, 992 + SPARSITY * 3000 - 1), nth, pair="range_at_span_80n_plus_1"),
          Case("range_at_span_80n_plus_1", _span_term(3000, 1000, 992 + SPARSITY * 3000), nth),
          Case("bitmap_span_one_tile", _span_term(3000, 1000, 992 + MERGE_BM_DOCS - 1), nth, pair="bitmap_span_one_bit_more"),
          Case("bitmap_span_one_bit_more", _span_term(3000, 1000, 992 + MERGE_BM_DOCS), nth),
          Case("uniform_splitters_64_one_block_lists", _one_block_lists(), nth),
          Case("one_posting_terms_257", _one_posting_terms(257), _every_nth(5)),
          Case("weight_prefix_at_batch_q", _weights((BATCH_Q // 2, BATCH_Q // 2, 10)), nth, pair="weight_prefix_below_batch_q"),
          Case("weight_prefix_below_batch_q", _weights((BATCH_Q // 2, BATCH_Q // 2 - 1, 10)), nth),
          Case("empty_terms_first_last_between", _empties(), _every_nth(4), encoding=True),
          Case("large_terms_interrupt_small_ones", _interrupted(), nth, encoding=True),
          Case("terms_65535_few_kernel", lambda: _dictionary(FEW_TERMS - 1), _every_nth(11), same="terms_65536_thread_per_term"),
          Case("terms_65536_thread_per_term", lambda: _dictionary(FEW_TERMS), _every_nth(11)),
          Case("k31_cuts_inside_blocks", _cut_lists(31), nth, options={"merge.large_tile": 1000}),
          Case("k32_cuts_inside_blocks", _cut_lists(32), nth, options={"merge.large_tile": 1000})]
    # -- fallbacks
    c += [Case("fold_16_small_no_event", _fold_small(16), lambda s: FOLD_IDS[::5]),
          Case("fold_17_small_batch_redo", _fold_small(17), lambda s: FOLD_IDS[::5], encoding=True),
          Case("fold_16_large_no_event", _fold_large(16), lambda s: SPARSE_IDS[::6]),
          Case("fold_17_large_every_tile_overflows", _fold_large(17), lambda s: SPARSE_IDS[::6], union=True),
          Case("clustered_overfull_bitmap_leaves", _clustered(), _clustered_removed, encoding=True),
          Case("top_of_id_space_cluster", _top_cluster(), lambda s: [TOP, TOP - 50_000, 6_000_000])]
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
