"""The case table of ii2_explain_ranges, shared by tests/test_explain_cpu.py (its own consistency, no GPU) and
tests/test_gpu_explain_ranges.py (the device against it).  Every expectation comes from numpy alone: bit g of row i is
any(ids[i] in L for L in group g); an id that is repeated keeps its mask in its first row and has zeros after.

A case: `segments` - per segment its posting lists; `groups` - per group its ranges (segment, first list, end list); `ids` - the
rows, in any order.  The shapes are the smallest at which the kernels can go wrong: wave and workgroup edges of the row kernels,
ids that share a bitmap word, probe chains of the 64-slot table (chosen with the hash the kernels run), the edges of the mask
words."""
from dataclasses import dataclass, field

import numpy as np

MUL = 0x9E3779B1


def slot(id, log2_slots):
    """ii2_explain_slot restated: the top log2_slots bits of the low 32 bits of id * MUL"""
    return ((int(id) * MUL) & 0xFFFFFFFF) >> (32 - log2_slots)


def table_log2(n_ids):
    """log2 of the table's slots: the smallest power of two >= 2 * n_ids, at least 64"""
    l = 6
    while (1 << l) < 2 * n_ids:
        l += 1
    return l


def colliding(target, log2_slots, count, lo, hi, slot_fn=slot):
    """the first `count` ids of [lo, hi), ascending, whose probe starts at slot `target` of a table of 1 << log2_slots slots"""
    cand = np.arange(lo, hi, dtype=np.uint64)
    cand = cand[((cand * MUL) & 0xFFFFFFFF) >> (32 - log2_slots) == target][:count]
    assert cand.size == count and all(slot_fn(int(x), log2_slots) == target for x in cand)
    return cand.astype(np.uint32)


def truth(group_lists, ids):
    """masks[n_ids, n_words] (uint64): group_lists[g] = the posting lists of group g"""
    ids = np.asarray(ids, np.uint32)
    n_words = (len(group_lists) + 63) // 64
    masks = np.zeros((ids.size, n_words), np.uint64)
    _, first_row = np.unique(ids, return_index=True)
    is_first = np.zeros(ids.size, bool)
    is_first[first_row] = True
    for g, lists in enumerate(group_lists):
        member = np.zeros(ids.size, bool)
        for l in lists:
            member |= np.isin(ids, np.asarray(l, np.uint32))
        masks[member & is_first, g >> 6] |= np.uint64(1 << (g & 63))
    return masks


def popcount(masks):
    return int(sum(bin(int(w)).count("1") for w in np.asarray(masks, np.uint64).ravel()))


@dataclass
class Case:
    name: str
    segments: list                      # [segment][list] -> ascending uint32 ids
    groups: list                        # [group] -> [(segment, first list, end list), ...]
    ids: np.ndarray
    windows: int = 1                    # doc windows at the default window of 2^30 docs (0: nothing is marked)
    note: dict = field(default_factory=dict)

    def group_lists(self):
        return [[self.segments[s][j] for s, a, b in g for j in range(a, b)] for g in self.groups]

    def expect(self):
        return truth(self.group_lists(), self.ids)

    @property
    def n_words(self):
        return (len(self.groups) + 63) // 64

    @property
    def n_lists(self):
        return sum(b - a for g in self.groups for _, a, b in g)

    @property
    def n_blocks(self):
        return sum((len(l) + 255) // 256 for lists in self.group_lists() for l in lists)


def _u32(x):
    return np.asarray(x, np.uint32)


def _sorted_unique(rng, n, universe):
    return np.sort(rng.choice(universe, size=n, replace=False)).astype(np.uint32)


def _ordered(ids, order, rng):
    if order == "ascending":
        return ids.copy()
    if order == "descending":
        return ids[::-1].copy()
    return rng.permutation(ids).astype(np.uint32)


ROW_SIZES = (1, 63, 64, 65, 257)
ORDERS = ("ascending", "descending", "shuffled")
WORD_GROUPS = (1, 63, 64, 65, 130)


def cases(slot_fn=slot):
    out = []
    # ---- rows: wave and workgroup edges of prepare and mark, the same set in three orders ----
    rng = np.random.default_rng(7001)
    U = 5000
    row_lists = [_sorted_unique(rng, n, U) for n in (1, 40, 255, 256, 257, 700, 1300, 2000, 30, 513, 90, 1024)]
    row_groups = [[(0, 0, 2)], [(0, 2, 5)], [(0, 5, 6)], [(0, 6, 8)], [(0, 8, 11)], [(0, 11, 12)]]
    for n in ROW_SIZES:
        base = _sorted_unique(rng, n, U)
        if n == 1:
            base = row_lists[5][100:101].copy()                          # a single id that does hit
        for order in ORDERS:
            out.append(Case(f"rows_{n}_{order}", [row_lists], row_groups, _ordered(base, order, np.random.default_rng(n))))
    # ---- bitmap: several ids in one bitmap word; ids 0 and 2^32 - 1 in the lists and among the ids (a doc span of 2^32) ----
    word = _u32([64, 65, 66, 70, 77, 94, 95])
    lists = [_u32([0, 64, 66, 95, 0xFFFFFFFF]), _u32([65, 66, 94]), _u32([0xFFFFFFFE, 0xFFFFFFFF]), _u32([0, 7, 96])]
    out.append(Case("bitmap_shared_word", [lists], [[(0, 0, 1)], [(0, 1, 2)], [(0, 3, 4)]], _u32([95, 64, 70, 66, 65, 94, 77])))
    out.append(Case("bitmap_id_space_edges", [lists], [[(0, 0, 1)], [(0, 1, 2)], [(0, 2, 3)], [(0, 3, 4)]],
                    np.concatenate([_u32([0xFFFFFFFF]), word, _u32([0, 0xFFFFFFFE, 7])]), windows=4))
    # ---- the hash table: 64 slots, chains chosen with the kernels' hash ----
    chain = colliding(10, 6, 21, 0, 1 << 16, slot_fn)
    others = _u32([x for x in range(3000, 3400) if slot_fn(x, 6) not in range(10, 31)][:8])
    lists = [chain[::2].copy(), chain[1::2].copy(), np.sort(np.concatenate([chain[:5], others[:4]])).astype(np.uint32), np.sort(others)]
    groups = [[(0, 0, 1)], [(0, 1, 2)], [(0, 2, 3)], [(0, 3, 4)]]
    out.append(Case("hash_chain_of_20", [lists], groups, np.concatenate([chain[:20][::-1], others])))
    # ... the 21st id of the chain lies in the lists and not among the ids: its probe would walk all 20 before the empty slot
    out.append(Case("hash_absent_after_full_chain", [lists], groups, chain[:20].copy(), note={"absent": int(chain[20])}))
    wrap = colliding(62, 6, 6, 0, 1 << 16, slot_fn)
    low = colliding(0, 6, 2, 0, 1 << 16, slot_fn)                          # ... whose own slot the wrapped chain has taken
    lists = [wrap[:4].copy(), np.sort(np.concatenate([wrap[3:], low])).astype(np.uint32), low[1:].copy()]
    out.append(Case("hash_chain_wraps", [lists], [[(0, 0, 1)], [(0, 1, 2)], [(0, 2, 3)]], np.concatenate([wrap, low])))
    # ---- repeated ids: a triple and two pairs among 100 ids ----
    rng = np.random.default_rng(7002)
    lists = [_sorted_unique(rng, n, 3000) for n in (900, 1500, 400, 2200)]
    hit = _u32([lists[0][5], lists[1][700], lists[3][11]])                   # the repeated ones do hit
    ids = rng.permutation(np.setdiff1d(_sorted_unique(rng, 120, 3000), hit)[:96]).astype(np.uint32)
    ids[[3, 20, 70]] = hit                                                  # their first rows ...
    ids = np.insert(ids, [10, 50, 50, 90], [ids[3], ids[20], ids[20], ids[70]]).astype(np.uint32)      # ... and the later ones
    assert ids.size == 100 and np.unique(ids).size == 96
    out.append(Case("repeated_ids", [lists], [[(0, 0, 1)], [(0, 1, 3)], [(0, 3, 4)], [(0, 0, 4)]], ids))
    # ---- mask words: n_groups at the words' edges, a doc in groups 63 and 64 at once ----
    rng = np.random.default_rng(7003)
    lists = [_sorted_unique(rng, int(rng.integers(1, 300)), 2000) for _ in range(130)]
    both = np.uint32(1234)
    for g in (0, 62, 63, 64, 65, 127, 128, 129):
        lists[g] = np.union1d(lists[g], [both]).astype(np.uint32)
    ids = rng.permutation(np.union1d(_sorted_unique(rng, 70, 2000), [both])).astype(np.uint32)
    for n in WORD_GROUPS:
        out.append(Case(f"words_{n}_groups", [lists], [[(0, g, g + 1)] for g in range(n)], ids))
    # ---- lists: a group over 3 segments, one list in two groups, a list twice in a group, empty groups / ranges / lists ----
    rng = np.random.default_rng(7004)
    mk = lambda k: [_sorted_unique(rng, int(rng.integers(1, 900)), 20_000) for _ in range(k)]
    A, B, Cs = mk(6), mk(5), mk(4)
    B[2] = np.empty(0, np.uint32)
    Cs[0] = np.empty(0, np.uint32)
    groups = [[(0, 0, 2), (1, 0, 1), (2, 1, 3)],                             # three segments
              [(0, 2, 3)], [(0, 2, 3), (1, 4, 5)],                           # list 2 of A in two groups
              [(1, 1, 2), (1, 1, 2), (1, 0, 2)],                             # a list twice in one group, and once more in an overlapping range
              [],                                                           # a group without a range
              [(0, 4, 4), (1, 3, 3)],                                        # ... of empty ranges only
              [(1, 2, 3), (2, 0, 1)],                                        # ... of empty lists only
              [(2, 0, 4), (0, 5, 5), (0, 5, 6)]]
    ids = rng.permutation(np.union1d(_sorted_unique(rng, 300, 20_000), np.concatenate([A[2][:20], B[1][:20], Cs[3][:5]]))).astype(np.uint32)
    out.append(Case("lists_and_groups", [A, B, Cs], groups, ids))
    out.append(Case("no_group_owns_a_block", [A, B, Cs], [[], [(1, 2, 3)], [(0, 1, 1)]], ids[:40].copy(), windows=0))
    # ---- the ids' span misses the lists': zero rows, nothing decoded ----
    span = [[_u32(np.arange(1000, 2000, 3))]]
    out.append(Case("span_miss", span, [[(0, 0, 1)]], _u32([5000, 2001, 70000]), windows=0))
    out.append(Case("ids_around_the_span", span, [[(0, 0, 1)]], _u32([5000, 2001, 999, 70000, 1001])))      # (1001 lies inside and in no list)
    # ---- a 2000-posting list (8 blocks) of which the ids hit only blocks 0 and 7 ----
    long_list = (np.arange(2000, dtype=np.uint32) * 400 + 17).astype(np.uint32)           # a block spans 102400 docs: 50 chunks of 2048
    ids = _u32([long_list[1999], long_list[3], 18, long_list[1900], long_list[200] + 1])
    assert np.all(np.isin(ids, long_list)[[0, 1, 3]]) and not np.isin(ids, long_list)[[2, 4]].any()
    out.append(Case("long_list_blocks_0_and_7", [[long_list]], [[(0, 0, 1)]], ids))
    return out
