"""Pure numpy: the list pools, random AND-of-ORs / NOT queries and expectations that the ii2_query_batch_groups tests share.
Nothing here touches the GPU, so the mix of query classes a seed produces is checked on the CPU (test_query_batch_groups_cpu.py)
and relied on by the GPU test (test_gpu_query_batch_groups.py).

A pool is [[array, ...], ...]: the lists of three segments and of a view of the first one (VIEW_SRC: ii2_seg_select source
indices, -1 an empty slot).  A query is (groups, exclude), each a list of groups, a group a list of ranges (pool entry, first,
end)."""
import numpy as np

MAX_LISTS, SMALL_POSTINGS, SMALL_BLOCKS, TINY_POSTINGS, TINY_BLOCKS = 64, 8192, 128, 2048, 32
_RUN = list(range(10, 30))
VIEW_SRC = [-1] + _RUN[:7] + [-1, -1] + _RUN[7:] + [-1]

# (universe, tombstones, seed) of the random batches; the seeds are picked so that every batch holds the mix of classes that
# check_mix asks for
RANDOM_BATCHES = [(50, False, 5105), (5_000, True, 5102), (1_000_000, False, 5103), ((1 << 32) - 1, True, 5104)]
N_QUERIES = 300


def core_of(rng, universe):
    if universe > 1_000_000:
        return np.array([0, 7, 1 << 31, 0xFFFFFFFE, 0xFFFFFFFF], np.uint32)       # ids 0 and 0xFFFFFFFF present
    return np.unique(rng.integers(0, universe, 12, dtype=np.uint64)).astype(np.uint32)


def make_lists(rng, universe, n_lists=90, core=None):
    """the pool of test_gpu_query_batch.py: three segments of lists of 0 .. 20 000 ids, 60 % of them sharing `core`, and a view"""
    def one():
        kind = rng.random()
        if kind < 0.06:
            n = 0
        elif kind < 0.55:
            n = int(rng.integers(1, 60))
        elif kind < 0.85:
            n = int(rng.integers(60, 600))
        elif kind < 0.96:
            n = int(rng.integers(600, 3000))
        else:
            n = int(rng.integers(8193, 20000))                                   # past the batch kernel's capacity on its own
        n = min(n, universe)
        l = np.unique(rng.integers(0, universe, n, dtype=np.uint64)).astype(np.uint32) if n else np.empty(0, np.uint32)
        if core is not None and n and rng.random() < 0.6:
            l = np.union1d(l, core).astype(np.uint32)
        return l

    pool = [[one() for _ in range(k)] for k in (n_lists, n_lists // 2, n_lists // 3)]
    pool.append([pool[0][j] if j >= 0 else np.empty(0, np.uint32) for j in VIEW_SRC])
    return pool


def _group(rng, pool, k, recent):
    """k lists in ranges of 1 .. 4 consecutive lists; now and then a list the batch has used before, or the same list twice"""
    ranges, have = [], 0
    while have < k:
        if recent and rng.random() < 0.2:
            s, a = recent[int(rng.integers(0, len(recent)))]
            ln = 1
        else:
            s = int(rng.integers(0, len(pool)))
            ln = min(int(rng.choice([1, 1, 1, 2, 4])), k - have, len(pool[s]))
            a = int(rng.integers(0, len(pool[s]) - ln + 1))
        ranges.append((s, a, a + ln))
        recent.append((s, a))
        have += ln
        if rng.random() < 0.15 and have < k:
            ranges.append((s, a, a + 1))
            have += 1
    return ranges


def random_queries(rng, pool, n_queries):
    """1 - 5 required groups of 1 - 20 lists and 0 - 3 excluded groups each; lists repeated within and across queries, some both
    required and excluded; now and then a query without groups, a required group without postings or an empty range"""
    empties = [(s, j) for s, ls in enumerate(pool) for j, l in enumerate(ls) if l.size == 0]
    recent, queries = [], []
    for _ in range(n_queries):
        u = rng.random()
        if u < 0.02:
            queries.append(([], []))                                             # no group
            continue
        n_req = int(rng.choice([1, 1, 2, 2, 3, 4, 5]))
        shape = rng.random()                                                     # few short groups, medium ones, long ones
        sizes = [1, 1, 2, 3] if shape < 0.4 else [2, 4, 6, 9] if shape < 0.7 else [8, 12, 16, 20, 20]
        groups = [_group(rng, pool, int(rng.choice(sizes)), recent) for _ in range(n_req)]
        if u < 0.06:
            s, j = empties[int(rng.integers(0, len(empties)))]
            groups[int(rng.integers(0, n_req))] = [(s, j, j + 1), (0, 3, 3)]     # a required group without postings
        exclude = [_group(rng, pool, int(rng.choice([1, 1, 2, 5, 20])), recent) for _ in range(int(rng.choice([0, 0, 1, 1, 2, 3])))]
        if exclude and rng.random() < 0.3:
            exclude[0].append(groups[0][0])                                      # a list both required and excluded
        if rng.random() < 0.1:
            groups[0].append((0, 3, 3))                                          # an empty range
        queries.append((groups, exclude))
    return queries


def lists_of(pool, ranges):
    return [pool[s][j] for s, a, b in ranges for j in range(a, b)]


def want(pool, groups, exclude, removed=None):
    """the ids in at least one list of every group of `groups` and in no list of any group of `exclude`, minus `removed`"""
    if not groups:
        return np.empty(0, np.uint32)
    w = None
    for g in groups:
        ls = lists_of(pool, g)
        u = np.unique(np.concatenate(ls)) if ls else np.empty(0, np.uint32)
        w = u if w is None else np.intersect1d(w, u, assume_unique=True)
    for g in exclude:
        for l in lists_of(pool, g):
            w = np.setdiff1d(w, l, assume_unique=True)
    if removed is not None:
        w = np.setdiff1d(w, removed, assume_unique=True)
    return w.astype(np.uint32)


def query_class(pool, groups, exclude):
    """"empty" | "tiny" | "small" | "large" from the numpy sizes alone, by the rule of include/ii2.h: a query without a group,
    with a required group without postings or with required doc spans that do not overlap is empty; the others count their
    non-empty required lists (a list as often as it is named) and the non-empty excluded lists whose doc span meets the required
    groups' common span: up to 64 lists, 2048 postings in 32 blocks tiny, 8192 postings in 128 blocks small, beyond large"""
    if not groups:
        return "empty"
    lo, hi, mine = 0, 0xFFFFFFFF, []
    for g in groups:
        ls = [l for l in lists_of(pool, g) if l.size]
        if not ls:
            return "empty"
        lo, hi = max(lo, min(int(l[0]) for l in ls)), min(hi, max(int(l[-1]) for l in ls))
        mine += ls
    if lo > hi:
        return "empty"
    mine += [l for g in exclude for l in lists_of(pool, g) if l.size and int(l[0]) <= hi and int(l[-1]) >= lo]
    post, blocks = sum(l.size for l in mine), sum((l.size + 255) // 256 for l in mine)
    if len(mine) > MAX_LISTS or post > SMALL_POSTINGS or blocks > SMALL_BLOCKS:
        return "large"
    return "tiny" if post <= TINY_POSTINGS and blocks <= TINY_BLOCKS else "small"


# ---- the capacity table: queries at, and one past, every limit of the one-workgroup kernels --------------------------------
# A pool of one segment per entry: 33 lists of 256 postings (one full block each), 33 lists of 64 postings, two one-posting
# lists, 80 short lists, and a one-posting list far outside every other span.
CAPACITY_LISTS = [
    [np.arange(i, 256 * 64 + i, 64, dtype=np.uint32) for i in range(33)],
    [np.arange(i, 64 * 100 + i, 100, dtype=np.uint32) for i in range(33)],
    [np.array([77], np.uint32), np.array([64], np.uint32)],
    [np.arange(i % 7, 2000, 17 + i % 5, dtype=np.uint32) for i in range(80)],
    [np.array([1_000_000], np.uint32)],
]
CAPACITY_QUERIES = [
    # the excluded lists are counted in: 20 + 12 lists, 2048 postings in 32 blocks - exactly the 256-thread form's capacity
    ([[(1, 0, 10)], [(1, 10, 20)]], [[(1, 20, 32)]]),
    ([[(1, 0, 10)], [(1, 10, 20)]], [[(1, 20, 33)]]),           # 33 blocks: one past it -> the 1024-thread form
    ([[(1, 0, 32)]], []),                                       # 32 blocks in one group
    ([[(1, 0, 33)]], []),
    ([[(0, 0, 4)], [(0, 2, 6)]], []),                           # 2048 postings in 8 full blocks
    ([[(0, 0, 4)], [(0, 2, 6)]], [[(2, 0, 1)]]),                # 2049 postings
    ([[(0, 0, 16)], [(0, 8, 16)]], [[(0, 16, 24)]]),            # 8192 postings in 32 blocks: exactly the 1024-thread form's capacity
    ([[(0, 0, 16)], [(0, 8, 16)]], [[(0, 16, 24)], [(2, 1, 2)]]),   # 8193 postings: a large query
    ([[(0, 0, 16)], [(0, 8, 16), (2, 1, 2)]], [[(0, 16, 24)]]),     # ... with the extra posting on the required side
    ([[(0, 0, 33)]], []),
    ([[(3, 0, 30)], [(3, 30, 50)]], [[(3, 50, 64)]]),           # 64 lists
    ([[(3, 0, 30)], [(3, 30, 50)]], [[(3, 50, 65)]]),           # 65 lists: a large query
    ([[(3, 0, 30), (3, 64, 65)], [(3, 30, 50)]], [[(3, 50, 64)]]),
    ([[(3, 0, 64)]], []),
    ([[(3, 0, 65)]], []),
    ([[(3, 0, 40), (3, 20, 80), (1, 0, 33)]], [[(3, 1, 2)]]),
    # 64 lists that count plus the far list.  Excluded, its span misses the required groups' common span: it does not count and
    # the query stays small.  Required in a group of its own, the required spans do not overlap: the query is empty.
    ([[(3, 0, 30)], [(3, 30, 50)]], [[(3, 50, 64)], [(4, 0, 1)]]),
    ([[(3, 0, 30)], [(3, 30, 50)], [(4, 0, 1)]], [[(3, 50, 64)]]),
]
CAPACITY_CLASSES = ["tiny", "small", "tiny", "small", "tiny", "small", "small", "large", "large", "large", "small", "large", "large",
                    "small", "large", "large", "small", "empty"]


def random_batch(universe, with_tomb, seed):
    """(pool, queries, removed or None, expectations) of one entry of RANDOM_BATCHES"""
    rng = np.random.default_rng(seed)
    core = core_of(rng, universe)
    pool = make_lists(rng, universe, core=core)
    removed = None
    if with_tomb:
        removed = np.unique(np.concatenate([rng.integers(0, universe, 300, dtype=np.uint64).astype(np.uint32), core[:2]]))
    queries = random_queries(rng, pool, N_QUERIES)
    return pool, queries, removed, [want(pool, g, x, removed) for g, x in queries]


def check_mix(pool, queries, wants, removed):
    """what the issue asks of every generated batch; returns the counts"""
    classes = [query_class(pool, g, x) for g, x in queries]
    n = {k: classes.count(k) for k in ("empty", "tiny", "small", "large")}
    nonempty = sum(w.size > 0 for w in wants)
    removed_some = sum(want(pool, g, [], removed).size > w.size for (g, x), w in zip(queries, wants))
    assert n["tiny"] >= 30 and n["small"] >= 30 and n["large"] >= 10 and n["empty"] >= 10, n
    assert nonempty * 4 >= len(queries), nonempty
    assert removed_some * 10 >= len(queries), removed_some
    return n, nonempty, removed_some
