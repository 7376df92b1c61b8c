"""The case table of ii2_explain_batch, shared by tests/test_explain_batch_cpu.py (its own consistency and the planner, no GPU) and
tests/test_gpu_explain_batch.py (the device against it).  Every expectation comes from plain Python: a set per list; bit g of row i
of query q is any(ids[i] in L for L in group g of q); an id that is repeated inside a page keeps its mask in its first row and has
zeros after; query q's rows start at word mask_off[q] = sum over the queries before it of ids x ceil(groups / 64).

A batch: `segments` - per segment its posting lists (`views`: segment v is ii2_seg_select(segment base, src), and segments[v]
holds the lists the view shows); `queries` - per query (groups, ids), groups = per group its ranges (segment, first list, end list).
The shapes are the smallest at which the planner or the kernel can go wrong: the size classes' edges, the list and id limits, the
mask words' seams, block seams, the id space's ends, repeated ids."""
from dataclasses import dataclass, field

import numpy as np

MAX_LISTS = 64
BATCH_IDS = 1024                         # II2_EXPLAIN_BATCH_IDS
TINY_POSTINGS, TINY_BLOCKS = 2048, 32
SMALL_POSTINGS, SMALL_BLOCKS = 8192, 128
EMPTY, TINY, SMALL, SINGLE = range(4)
OPTIONS = ((1, 1), (1, 0), (0, 1), (0, 0))          # (batch.explain, batch.tiny)


def form(n_lists, n_postings, n_blocks, n_ids, explain=1, tiny=1):
    """the planner restated: what runs a query of n_lists non-empty lists"""
    if n_ids == 0 or n_blocks == 0:
        return EMPTY
    if not explain or n_ids > BATCH_IDS or n_lists > MAX_LISTS or n_postings > SMALL_POSTINGS or n_blocks > SMALL_BLOCKS:
        return SINGLE
    return TINY if tiny and n_postings <= TINY_POSTINGS and n_blocks <= TINY_BLOCKS else SMALL


def rows(group_lists, ids):
    """[n_ids][n_words] ints: group_lists[g] = the posting lists of group g"""
    sets = [[set(int(x) for x in l) for l in lists] for lists in group_lists]
    n_words = (len(group_lists) + 63) // 64
    out, seen = [], set()
    for x in (int(x) for x in ids):
        row = [0] * n_words
        if x not in seen:
            seen.add(x)
            for g, lists in enumerate(sets):
                if any(x in s for s in lists):
                    row[g >> 6] |= 1 << (g & 63)
        out.append(row)
    return out


@dataclass
class Batch:
    name: str
    segments: list                      # [segment][list] -> ascending uint32 ids
    queries: list                       # [query] -> (groups, ids)
    views: dict = field(default_factory=dict)       # segment -> (base segment, src list numbers, -1 = an empty slot)

    def group_lists(self, q):
        return [[self.segments[s][j] for s, a, b in g for j in range(a, b)] for g in self.queries[q][0]]

    def n_words(self, q):
        return (len(self.queries[q][0]) + 63) // 64

    def n_ids(self, q):
        return len(self.queries[q][1])

    def ids_off(self):
        return np.cumsum([0] + [self.n_ids(q) for q in range(len(self.queries))]).astype(np.uint64)

    def all_ids(self):
        return np.concatenate([np.asarray(ids, np.uint32) for _, ids in self.queries] + [np.empty(0, np.uint32)])

    def mask_off(self):
        return np.cumsum([0] + [self.n_ids(q) * self.n_words(q) for q in range(len(self.queries))]).astype(np.uint64)

    def expect(self):
        """the packed masks, uint64 [mask_off[-1]]"""
        words = [w for q in range(len(self.queries)) for row in rows(self.group_lists(q), self.queries[q][1]) for w in row]
        return np.array(words, np.uint64) if words else np.empty(0, np.uint64)

    def shape(self, q):
        """(non-empty lists, their postings, their blocks, ids) of query q, a list counted once per range that names it"""
        ls = [l for lists in self.group_lists(q) for l in lists if len(l)]
        return len(ls), sum(len(l) for l in ls), sum((len(l) + 255) // 256 for l in ls), self.n_ids(q)

    def forms(self, explain=1, tiny=1):
        return [form(*self.shape(q), explain, tiny) for q in range(len(self.queries))]

    def stats(self, explain=1, tiny=1):
        f = self.forms(explain, tiny)
        want = self.expect()
        return {"n_tiny": f.count(TINY), "n_small": f.count(SMALL), "n_single": f.count(SINGLE), "n_empty": f.count(EMPTY),
                "n_rows": int(self.ids_off()[-1]), "n_words": int(self.mask_off()[-1]), "n_hits": popcount(want)}


def popcount(words):
    return int(sum(bin(int(w)).count("1") for w in np.asarray(words, np.uint64).ravel()))


def _u32(x):
    return np.asarray(x, np.uint32)


def _su(rng, n, universe):
    return np.sort(rng.choice(universe, size=n, replace=False)).astype(np.uint32)


def _page(rng, lists, n_hit, n_miss, universe):
    """a shuffled page: n_hit ids drawn from the lists, n_miss from the universe at large (some of those lie in no list)"""
    pool = np.unique(np.concatenate(lists))
    ids = np.union1d(rng.choice(pool, size=min(n_hit, pool.size), replace=False), _su(rng, n_miss, universe))
    return rng.permutation(ids).astype(np.uint32)


def _size_lists(rng):
    """one segment whose ranges give every size-class edge: 32 x 64, 1 x 65, 33 x 62, 32 x 256, 1 x 257 postings"""
    U = 60_000
    return ([_su(rng, 64, U) for _ in range(32)] + [_su(rng, 65, U)] + [_su(rng, 62, U) for _ in range(33)]
            + [_su(rng, 256, U) for _ in range(32)] + [_su(rng, 257, U)])


def cases():
    out = []
    # ---- the size classes' edges: 2048 postings / 32 blocks and one over (TINY -> SMALL), 8192 and one over (SMALL -> SINGLE) ----
    rng = np.random.default_rng(9001)
    S = _size_lists(rng)
    U = 60_000
    at_tiny = [[(0, 0, 8)], [(0, 8, 16)], [(0, 16, 24)], [(0, 24, 32)]]                     # 32 x 64 = 2048 postings in 32 blocks
    over_tiny_post = [[(0, 1, 32)], [(0, 32, 33)]]                                          # 31 x 64 + 65 = 2049 in 32 blocks
    over_tiny_blk = [[(0, 33, 50)], [(0, 50, 66)]]                                          # 33 x 62 = 2046 in 33 blocks
    at_small = [[(0, 66, 80)], [(0, 80, 90)], [(0, 90, 98)]]                                # 32 x 256 = 8192 in 32 blocks
    over_small = [[(0, 67, 98)], [(0, 98, 99)]]                                             # 31 x 256 + 257 = 8193 in 33 blocks
    b = Batch("size_class_edges", [S], [(at_tiny, _page(rng, S[0:32], 12, 8, U)), (over_tiny_post, _page(rng, S[1:33], 12, 8, U)),
                                        (over_tiny_blk, _page(rng, S[33:66], 12, 8, U)), (at_small, _page(rng, S[66:98], 30, 8, U)),
                                        (over_small, _page(rng, S[67:99], 30, 8, U))])
    assert [b.shape(q)[:3] for q in range(5)] == [(32, 2048, 32), (32, 2049, 32), (33, 2046, 33), (32, 8192, 32), (32, 8193, 33)]
    out.append(b)
    # ---- one mixed batch: TINY, SMALL, SINGLE and EMPTY queries interleaved (the same segment) ----
    many_ids = rng.permutation(_su(rng, BATCH_IDS + 1, U)).astype(np.uint32)
    b = Batch("mixed", [S], [(at_tiny, _page(rng, S[0:32], 9, 3, U)), (at_tiny, _u32([])), (over_small, _page(rng, S[67:99], 20, 5, U)),
                             (at_small, _page(rng, S[66:98], 25, 5, U)), ([], _u32([5, 6, 7])), (over_tiny_blk, _page(rng, S[33:66], 7, 3, U)),
                             ([[(0, 0, 2)]], many_ids), ([[(0, 3, 3)], []], _u32([1, 2])), (over_tiny_post, _page(rng, S[1:33], 9, 3, U))])
    assert b.forms(1, 1) == [TINY, EMPTY, SINGLE, SMALL, EMPTY, SMALL, SINGLE, EMPTY, SMALL]
    out.append(b)
    # ---- 64 and 65 non-empty lists (empty ones in between do not count) ----
    rng = np.random.default_rng(9002)
    L = [_su(rng, int(rng.integers(1, 9)), 3000) for _ in range(70)]
    L[10] = L[40] = np.empty(0, np.uint32)
    g64 = [[(0, 0, 30)], [(0, 30, 50)], [(0, 50, 66)]]                                      # 66 lists, 2 of them empty
    g65 = [[(0, 0, 30)], [(0, 30, 50)], [(0, 50, 67)]]
    b = Batch("list_limit", [L], [(g64, _page(rng, L[:66], 15, 5, 3000)), (g65, _page(rng, L[:67], 15, 5, 3000))])
    assert [b.shape(q)[0] for q in range(2)] == [64, 65]
    out.append(b)
    # ---- II2_EXPLAIN_BATCH_IDS ids (the LDS table half full, its first id again in the last row) and one more ----
    rng = np.random.default_rng(9003)
    L = [_su(rng, 300, 5000) for _ in range(6)]
    groups = [[(0, 0, 2)], [(0, 2, 3)], [(0, 3, 6)]]
    ids = rng.permutation(_su(rng, BATCH_IDS + 1, 5000)).astype(np.uint32)
    full = ids[:BATCH_IDS].copy()
    full[-1] = full[0] = L[0][7]
    out.append(Batch("id_limit", [L], [(groups, full), (groups, ids)]))
    # ---- the mask words' seams: 130 groups of which only 0, 63, 64 and 129 own lists; one id in all four ----
    rng = np.random.default_rng(9004)
    L = [np.union1d(_su(rng, 40, 2000), [1234]).astype(np.uint32) for _ in range(4)]
    groups = [[] for _ in range(130)]
    for j, g in enumerate((0, 63, 64, 129)):
        groups[g] = [(0, j, j + 1)]
    groups[5] = [(0, 2, 2)]                                                                 # (an empty range)
    ids = rng.permutation(np.union1d(_page(rng, L, 30, 10, 2000), [1234])).astype(np.uint32)
    out.append(Batch("word_seams", [L], [(groups, ids), (groups[:64], ids[::-1].copy()), (groups[:65], ids)]))
    # ---- blocks and groups: multi-block lists with a partial last block hit at a block's last posting and at the next one's
    # first, an id in several lists of one group, ids 0 and 2^32 - 1, ids in no list ----
    rng = np.random.default_rng(9005)
    long_a = np.union1d(_su(rng, 598, 1 << 20) + 1, [0, 0xFFFFFFFF]).astype(np.uint32)       # 600 postings: blocks of 256, 256, 88
    long_b = (_su(rng, 700, 1 << 20) + 1).astype(np.uint32)                                  # 700: 256, 256, 188
    shared = _u32([long_a[255], long_a[256], long_b[511], long_b[512]])
    short = np.union1d(_su(rng, 50, 1 << 20) + 1, shared[:2]).astype(np.uint32)
    L = [long_a, long_b, short, _u32([0]), _u32([0xFFFFFFFF])]
    ids = _u32([long_a[256], 0xFFFFFFFF, long_b[511], 3, long_a[255], long_b[512], 0, long_a[598], long_b[699], long_a[511] + 1, long_b[0], 0xFFFFFFFE])
    assert not np.isin(_u32([3, long_a[511] + 1, 0xFFFFFFFE]), np.concatenate(L)).any()
    groups = [[(0, 0, 1), (0, 2, 3)], [(0, 1, 2)], [(0, 2, 5)], [(0, 2, 3), (0, 2, 3), (0, 3, 5)]]
    b = Batch("blocks_and_groups", [L], [(groups, ids)])
    assert b.shape(0)[1] <= TINY_POSTINGS and b.shape(0)[2] == 14 and len(long_a) == 600
    out.append(b)
    # ---- repeated ids: next to each other, at the two ends of a page; the same ids under other groups in the next query ----
    rng = np.random.default_rng(9006)
    L = [_su(rng, n, 4000) for n in (300, 500, 120, 900)]
    base = _page(rng, L, 20, 6, 4000)
    hit = L[1][17]
    ids = np.concatenate([[hit], base[base != hit][:10], [base[11], base[11]], base[base != hit][12:20], [hit]]).astype(np.uint32)
    ga = [[(0, 0, 1)], [(0, 1, 2)], [(0, 2, 4)]]
    gb = [[(0, 0, 2)], [(0, 3, 4)]]
    b = Batch("repeats_and_neighbours", [L], [(ga, ids), (gb, ids), (ga, ids[::-1].copy()), (gb[:1], _u32([hit] * 5))])
    assert ids[0] == ids[-1] and ids[11] == ids[12]
    out.append(b)
    # ---- nothing to run: a query without groups, one without ids, one whose groups own no block - between two that do run ----
    rng = np.random.default_rng(9007)
    L = [_su(rng, 80, 1000), np.empty(0, np.uint32), _su(rng, 30, 1000)]
    g = [[(0, 0, 1)], [(0, 2, 3)]]
    page = _page(rng, L, 10, 5, 1000)
    out.append(Batch("nothing_to_run", [L], [(g, page), ([], page[:4].copy()), (g, _u32([])), ([[(0, 1, 2)], [], [(0, 2, 2)]], page[:6].copy()),
                                             (g, page[::-1].copy())]))
    # ---- segments and views: a group over two segments and a view with empty slots ----
    rng = np.random.default_rng(9008)
    A = [_su(rng, int(rng.integers(1, 400)), 9000) for _ in range(10)]
    B = [_su(rng, int(rng.integers(1, 700)), 9000) for _ in range(4)]
    src = [0, -1, 1, 2, -1, 3, 4, -1]                                                       # (a view skips only empty slots)
    V = [A[j] if j >= 0 else np.empty(0, np.uint32) for j in src]
    q0 = [[(0, 0, 3), (1, 0, 1)], [(2, 0, 4)], [(2, 4, 8), (1, 2, 4)]]
    q1 = [[(2, 0, 8)], [(0, 3, 10)], [(1, 1, 2), (1, 1, 2)]]
    out.append(Batch("segments_and_views", [A, B, V], [(q0, _page(rng, A + B, 40, 10, 9000)), (q1, _page(rng, A + B, 40, 10, 9000))],
                     views={2: (0, src)}))
    return out
