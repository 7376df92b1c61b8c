"""The case table of the histograms (ii2_histogram_ranges, ii2_histogram_ids): edge sets, the ids worth asking about, a plain
statement of what a block's doc bounds are to an axis (ii2_hist_block), and the expected counts from numpy.  No device needed."""
import numpy as np

TOP = 1 << 32
SKIP, WHOLE, SPLIT, WIDE = 0, 1, 2, 3
STRIP = 64               # buckets a SPLIT block meets at most

# name -> n_buckets + 1 edges
EDGE_SETS = {
    "one bucket": [100, 5000],
    "everything": [0, TOP],
    "width 1": list(range(1000, 1101)),
    "4096 buckets": [7 + 1021 * b for b in range(4097)],
    "inside": [50_000, 50_001, 60_000, 4_000_000_000, TOP - 1],
    "uneven": [0, 6, 10, 301, TOP],
    "top": [TOP - 3, TOP - 2, TOP - 1, TOP],
}

# (edges, return code) - II2_EINVAL = -1, II2_ERANGE = -5
BAD_EDGES = [
    ([5, 5], -1),                                  # equal neighbours
    ([0, 10, 10, 20], -1),
    ([10, 5], -1),                                 # descending
    ([0, 10, 9], -1),
    ([0, TOP + 1], -1),                            # above 2^32
    ([TOP, TOP + 1], -1),
    ([7], -1),                                     # no bucket
    (list(range(4098)), -5),                       # 4097 buckets
]


def probe_ids(edges):
    """ids at every edge, edge +- 1, 0 and 2^32 - 1"""
    ids = {0, TOP - 1}
    for e in edges:
        ids.update(x for x in (e - 1, e, e + 1) if 0 <= x < TOP)
    return sorted(ids)


def buckets(edges, ids):
    """numpy's answer: the bucket of every id, -1 outside the axis"""
    e = np.asarray(edges, np.int64)
    ids = np.asarray(ids, np.int64)
    b = np.searchsorted(e[:-1], ids, "right") - 1
    b[(ids < e[0]) | (ids >= e[-1])] = -1
    return b


def block(edges, first_doc, up):
    """(kind, b_lo, b_hi) of a block with the doc bounds [first_doc, up], stated plainly: the buckets that hold an id of the bounds"""
    lo_ax, hi_ax = edges[0], edges[-1] - 1
    if up < first_doc or first_doc > hi_ax or up < lo_ax:
        return SKIP, 0, 0
    a, z = max(first_doc, lo_ax), min(up, hi_ax)
    met = [b for b in range(len(edges) - 1) if edges[b] <= z and edges[b + 1] - 1 >= a]
    leaves = first_doc < lo_ax or up > hi_ax
    if len(met) == 1 and not leaves:
        return WHOLE, met[0], met[0]
    return (SPLIT if len(met) <= STRIP else WIDE), met[0], met[-1]


# (edge set, first_doc, up): what ii2_hist_block is asked
W1 = EDGE_SETS["width 1"]
U = EDGE_SETS["uneven"]
I = EDGE_SETS["inside"]
BLOCKS = [
    (U, 1, 5), (U, 0, 5), (U, 7, 8), (U, 301, TOP - 1),                          # inside one bucket
    (U, 1, 6), (U, 6, 9), (U, 6, 10), (U, 5, 6), (U, 9, 10), (U, 300, 301),      # up == edge - 1, up == edge
    (W1, 1000, 1001), (W1, 1000, 1063), (W1, 1000, 1064), (W1, 1036, 1099),      # 2, 64, 65, 64 buckets
    (W1, 1035, 1099), (W1, 1000, 1099),
    (W1, 990, 1005), (W1, 1090, 1200), (W1, 0, TOP - 1), (W1, 999, 1000), (W1, 1099, 1100),      # half outside
    (W1, 0, 999), (W1, 1100, 1100), (W1, 1100, TOP - 1), (I, 0, 49_999), (I, TOP - 1, TOP - 1),  # wholly outside
    (I, 50_000, 50_000), (I, 50_001, 50_001), (I, TOP - 2, TOP - 2), (W1, 1000, 1000), (W1, 999, 999),      # first_doc == up
    (I, 49_999, 50_000), (I, 50_000, 50_001), (I, 60_000, TOP - 2), (I, 60_000, TOP - 1),
    (EDGE_SETS["one bucket"], 100, 4999), (EDGE_SETS["one bucket"], 99, 4999), (EDGE_SETS["one bucket"], 100, 5000),
    (EDGE_SETS["everything"], 0, TOP - 1), (EDGE_SETS["top"], TOP - 3, TOP - 1), (EDGE_SETS["top"], TOP - 4, TOP - 1),
    (EDGE_SETS["4096 buckets"], 7, 7 + 1021 * 64 - 1), (EDGE_SETS["4096 buckets"], 7, 7 + 1021 * 64), (EDGE_SETS["4096 buckets"], 0, TOP - 1),
]


def truth(lists, ids, edges, removed=()):
    """counts[k, b]: the ids of list k in bucket b that lie in `ids` (None: every doc) and not in `removed`"""
    nb = len(edges) - 1
    out = np.zeros((len(lists), nb), np.uint64)
    for k, l in enumerate(lists):
        l = np.asarray(l, np.uint32)
        hit = np.ones(l.size, bool) if ids is None else np.isin(l, np.asarray(ids, np.uint32))
        hit &= ~np.isin(l, np.asarray(removed, np.uint32))
        b = buckets(edges, l[hit])
        out[k] = np.bincount(b[b >= 0], minlength=nb)
    return out


def uniform(lo, hi, n):
    """n buckets of (almost) equal width over [lo, hi)"""
    e = [lo + (hi - lo) * b // n for b in range(n + 1)]
    assert all(x < y for x, y in zip(e, e[1:]))
    return e
