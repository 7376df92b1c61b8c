"""CPU: the merge table of tests/merge_cases.py is sound before it reaches a GPU - the library names its events, every event and
every plan branch is reached by a case, both sides of every threshold differ in the tile count the model arrives at, the
fallback cases show the events counted by hand from merge.hip, and no case's reference is trivial."""
import numpy as np
import pytest

from inverted_index_2_amd import _lib
from inverted_index_2_amd.engine import merge_event_names
from oracle import oracle as orc
from tests import merge_cases as mc


def test_event_names_are_the_tables_and_end_with_null():
    lib = _lib.load()
    names = merge_event_names()
    assert tuple(names) == mc.EVENTS
    assert lib.ii2_merge_event_name(len(names)) is None and lib.ii2_merge_event_name(0xFFFFFFFF) is None
    assert lib.ii2_merge_event_name(0) == b"batch_redo"
    assert lib.ii2_merge_events(None, None, 0) == -1       # II2_EINVAL: the counters belong to a context


def test_thresholds_are_the_ones_the_cases_were_sized_for():
    assert (mc.MERGE_CAP, mc.SMALL_MAX, mc.BATCH_Q, mc.WMIN, mc.RANGE_TARGET, mc.MERGE_BM_DOCS) == (3584, 1280, 2304, 14, 3401, 229376)


def test_every_event_has_a_case():
    reached = set()
    for case in mc.CASES:
        reached |= set(case.events())
    assert reached <= set(mc.EVENTS)
    assert len(mc.UNREACHABLE) <= 1 and set(mc.UNREACHABLE) <= set(mc.EVENTS) and all(mc.UNREACHABLE.values())
    assert not (reached & set(mc.UNREACHABLE)), "an event listed as unreachable has a case"
    assert set(mc.EVENTS) - reached - set(mc.UNREACHABLE) == set()


def test_every_plan_branch_has_a_case():
    reached = set()
    for case in mc.CASES:
        reached |= case.plan().branches
    assert reached == set(mc.BRANCHES), sorted(set(mc.BRANCHES) ^ reached)


def test_both_sides_of_every_threshold_differ_in_tiles():
    pairs = [(c, mc.BY_NAME[c.pair]) for c in mc.CASES if c.pair]
    assert len(pairs) >= 6
    for a, b in pairs:
        assert a.plan().n_tiles != b.plan().n_tiles, (a.name, b.name)
        assert a.options == b.options
    for a in mc.CASES:
        if a.same:
            assert a.plan().n_tiles == mc.BY_NAME[a.same].plan().n_tiles, a.name


def test_tile_counts_counted_by_hand():
    """The numbers the issue states, from the constants and not from the model's code."""
    n = lambda name: mc.BY_NAME[name].plan().n_tiles
    assert (n("small_at_small_max"), n("large_at_small_max_plus_1")) == (1, 3)
    assert (n("range_at_target"), n("range_at_target_plus_1")) == (1, 2)
    assert (n("seven_blocks_take_a_third_tile"), n("eight_blocks_stay_at_two_tiles")) == (3, 2)
    assert (n("bitmap_at_span_80n"), n("range_at_span_80n_plus_1")) == (2, 1)
    assert (n("bitmap_span_one_tile"), n("bitmap_span_one_bit_more")) == (1, 2)
    assert n("uniform_splitters_64_one_block_lists") == 4
    assert (n("weight_prefix_at_batch_q"), n("weight_prefix_below_batch_q")) == (2, 1)
    assert n("empty_terms_first_last_between") == 1
    assert n("large_terms_interrupt_small_ones") == 3 + 1 + 1               # three batches, one bitmap tile (3000 docs), one range tile (1400 postings)
    # 257 terms of weight wmin = 14: the exclusive prefix reaches batch_q = 2304 at term 165 - a batch never holds MERGE_NT_MAX terms
    p = mc.BY_NAME["one_posting_terms_257"].plan()
    assert p.batches == [[0, 164], [165, 256]] and p.n_tiles == 2
    assert max(b - a + 1 for c in mc.CASES for a, b in c.plan().batches) <= (mc.BATCH_Q + mc.WMIN - 1) // mc.WMIN < mc.MERGE_NT_MAX
    # the cases about the two cut kernels: many tiles, every list cut inside its blocks
    for name, k in (("k31_cuts_inside_blocks", 31), ("k32_cuts_inside_blocks", 32)):
        p = mc.BY_NAME[name].plan()
        assert p.k == k and p.uniform[0] and p.n_tiles == -(-int(p.n[0]) // 1000) >= 19
    # the dictionary cases: both plan kernels, the same lists; the tied longest lists resolve to the first
    few, many = mc.BY_NAME["terms_65535_few_kernel"].plan(), mc.BY_NAME["terms_65536_thread_per_term"].plan()
    assert few.T == mc.FEW_TERMS - 1 and many.T == mc.FEW_TERMS and few.k == 20
    assert [int(few.best[t]) for t in (100, 30_000, 65_000)] == [3, 5, 0] and int(few.large.sum()) == 3
    assert many.n[-1] == 0 and np.array_equal(few.n, many.n[:-1])


def test_events_counted_by_hand():
    ev = lambda name: mc.BY_NAME[name].events()
    for case in mc.CASES:                                                   # the plan cases stay on the ordinary path
        if not case.name.startswith(("fold_17", "clustered", "top_of")):
            assert case.events() == {}, case.name
    # 40 ids below 2^17 + 2^14, each 17 times: the batch is redone; the term's root range and its lower halves down to 2^18 docs
    # overflow (15 ranges: 2^32 ... 2^18), every upper half still meets the list's one block and sorts nothing (14), and the two
    # halves of [0, 2^18) are bitmap leaves
    assert ev("fold_17_small_batch_redo") == {"batch_redo": 1, "range_bucket_overflow": 15, "leaf_sorted": 14, "leaf_bitmap": 2}
    # every id 17 times: each of the three tiles overflows, and so does every range of the bisection that holds an id
    e = ev("fold_17_large_every_tile_overflows")
    assert set(e) == {"range_bucket_overflow", "leaf_bitmap", "leaf_sorted"} and e["range_bucket_overflow"] >= 3 + 100
    assert mc.BY_NAME["fold_17_large_every_tile_overflows"].plan().n_tiles == 3
    # tile 0 holds 12 700 postings: bisected once, both halves fit the bitmap
    assert ev("clustered_overfull_bitmap_leaves") == {"range_overfull": 1, "leaf_bitmap": 2}
    mn, mx, t0_hi, mid = mc.clustered_geometry()
    p = mc.BY_NAME["clustered_overfull_bitmap_leaves"].plan()
    assert mc.tile_ranges(p, mc.BY_NAME["clustered_overfull_bitmap_leaves"].segs(), 0)[0] == (0, t0_hi) and (int(p.mn[0]), int(p.mx[0])) == (mn, mx)
    assert mn % 32 and (mid + 1) % 32 and (mid + 1) % 32 != 31 and (t0_hi + 1) % 32 and t0_hi - ((mid + 1) & ~31) < mc.MERGE_BM_DOCS
    rem = mc.BY_NAME["clustered_overfull_bitmap_leaves"].removed()
    assert mid + 1 < rem.max() < t0_hi - 64 and rem.min() == mn
    # the root's last bucket takes the 20 clustered ids; the halves spread them over two buckets
    assert ev("top_of_id_space_cluster") == {"range_bucket_overflow": 1, "leaf_sorted": 2}


def test_float_bucket_map_rounds_at_the_top_of_the_id_space():
    v = np.array([mc.TOP, mc.TOP - 100, mc.TOP - 950_000], np.uint32)
    raw = (v.astype(np.float32) * (np.float32(mc.MERGE_CAP) / np.float32(2.0 ** 32))).astype(np.int64)
    assert raw.tolist() == [mc.MERGE_CAP, mc.MERGE_CAP, mc.MERGE_CAP - 1]                  # one past the last bucket without the clamp
    assert mc._range_buckets(v, 0, mc.TOP, 0, mc.TOP).tolist() == [mc.MERGE_CAP - 1] * 3


@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_reference_is_not_trivial(case):
    segs = case.segs()
    T = len(segs[0][0]) - 1
    for o, v in segs:
        assert o.dtype == np.uint64 and v.dtype == np.uint32 and o.size == T + 1 and int(o[-1]) == v.size
        inner = np.ones(v.size, bool)
        inner[o[1:-1][o[1:-1] < v.size].astype(np.int64)] = False                            # (list starts)
        assert np.all((np.diff(v.astype(np.int64)) > 0) | ~inner[1:])                        # every list ascends
    offs, vals = [o for o, _ in segs], [v for _, v in segs]
    w_off, w_vals, w_terms = orc.merge_segments(offs, vals, ())
    assert w_vals.size > 0 and w_terms > 0
    for o, v in segs:
        assert not (np.array_equal(o, w_off) and np.array_equal(v, w_vals)), "the result is one of the inputs"
    removed = case.removed()
    assert removed.size
    t_off, t_vals, _ = orc.merge_segments(offs, vals, removed)
    assert 0 < t_vals.size < w_vals.size
    if T <= 300:                                                                             # the oracle against plain numpy, uint64
        r_off, r_vals = mc.reference(segs, removed)
        assert np.array_equal(t_off, r_off) and np.array_equal(t_vals.astype(np.uint64), r_vals)
    if case.union:
        assert T == 1 and np.unique(np.concatenate(vals)).size < sum(v.size for v in vals)
