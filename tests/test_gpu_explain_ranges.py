"""GPU: ii2_explain_ranges - per id of an array in any order, the groups it lies in - against numpy alone (tests/explain_cases.py:
bit g of row i is any(ids[i] in L for L in group g); a repeated id keeps its mask in its first row).  Masks and stats are
compared exactly.  The sizes are the smallest at which the kernels can go wrong."""
import ctypes as C

import numpy as np
import pytest
import torch

from inverted_index_2_amd import Context, _lib, explain_slot
from tests import explain_cases as ec
from tests.gpu_util import ctx, one_block_lists_past_a_wave, path_delta, sorted_unique  # noqa: F401

pytestmark = pytest.mark.gpu

PATTERN = 0xA5A5A5A5DEADBEEF
CASES = ec.cases()                                 # (built without the library: nothing is loaded while the tests are collected)
BY_NAME = {c.name: c for c in CASES}


class Option:
    def __init__(self, ctx, name, value, default):
        self.ctx, self.name, self.value, self.default = ctx, name, value, default

    def __enter__(self):
        self.ctx.set_option(self.name, self.value)

    def __exit__(self, *exc):
        self.ctx.set_option(self.name, self.default)


def explain(ctx, groups, ids):
    """(masks[n_ids, n_words], ExplainStats) of one call; the words behind the masks must stay as they were"""
    ids = np.asarray(ids, np.uint32)
    n_out = ids.size * ((len(groups) + 63) // 64)
    d_ids = ctx.empty(max(ids.size, 1)).upload(ids)
    out = ctx.empty(n_out + 8, np.uint64).upload(np.full(n_out + 8, PATTERN, np.uint64))
    out.count = n_out                              # (what the entry point takes as the capacity)
    with path_delta(ctx) as d:
        masks, st = ctx.explain_ranges(groups, d_ids, ids.size, stats=True, out=out)
    assert d == {}                                 # not a set operation: no kernel path
    out.count = n_out + 8
    got = out.download()
    assert np.all(got[n_out:] == PATTERN), "words written behind the masks"
    assert masks.shape == (ids.size, (len(groups) + 63) // 64)
    return got[:n_out].reshape(masks.shape), st


def run_case(ctx, case):
    segs = [ctx.encode_lists(lists) for lists in case.segments]
    groups = [[(segs[s], a, b) for s, a, b in g] for g in case.groups]
    return explain(ctx, groups, case.ids)


def check_stats(st, case, want, windows=None):
    assert (st.n_ids, st.n_lists, st.n_blocks, st.n_words) == (case.ids.size, case.n_lists, case.n_blocks, case.n_words)
    assert st.n_hits == ec.popcount(want)
    assert st.n_windows == (case.windows if windows is None else windows)
    assert st.log2_slots == (ec.table_log2(case.ids.size) if case.n_blocks else 0)
    assert st.n_decoded <= st.n_blocks * max(st.n_windows, 1) and (st.n_windows or st.n_decoded == 0)


def test_colliding_ids_are_those_the_library_hash_chooses():
    for a, b in zip(CASES, ec.cases(explain_slot)):
        assert a.name == b.name and np.array_equal(a.ids, b.ids) and all(np.array_equal(x, y) for x, y in zip(a.segments[0], b.segments[0]))
    chain = BY_NAME["hash_chain_of_20"]
    assert sum(explain_slot(int(x), 6) == 10 for x in chain.ids) == 20
    assert [explain_slot(int(x), 6) for x in BY_NAME["hash_chain_wraps"].ids] == [62] * 6 + [0] * 2
    assert explain_slot(BY_NAME["hash_absent_after_full_chain"].note["absent"], 6) == 10


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case(ctx, case):
    want = case.expect()
    got, st = run_case(ctx, case)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    check_stats(st, case, want)


@pytest.mark.parametrize("n", ec.ROW_SIZES)
def test_row_order_does_not_matter(ctx, n):
    rows = []
    for order in ec.ORDERS:
        case = BY_NAME[f"rows_{n}_{order}"]
        got, _ = run_case(ctx, case)
        rows.append({int(i): tuple(m.tolist()) for i, m in zip(case.ids, got)})
        assert len(rows[-1]) == n
    assert rows[0] == rows[1] == rows[2]


def test_repeated_ids_are_deterministic(ctx):
    case = BY_NAME["repeated_ids"]
    want = case.expect()
    runs = [run_case(ctx, case)[0] for _ in range(3)]
    for got in runs:
        assert np.array_equal(got, want)
    later = np.ones(case.ids.size, bool)
    later[np.unique(case.ids, return_index=True)[1]] = False
    assert later.sum() == 4 and not runs[0][later].any() and all(runs[0][i].any() for i in (3, 20, 70))


def test_summary_skip(ctx):
    case = BY_NAME["long_list_blocks_0_and_7"]
    want = case.expect()
    decoded = {}
    for skip in (1, 0):
        with Option(ctx, "count.summary_skip", skip, 1):
            got, st = run_case(ctx, case)
            assert np.array_equal(got, want), skip
            check_stats(st, case, want)
            decoded[skip] = st.n_decoded
    assert case.n_blocks == 8 and decoded[0] == 8                      # every block lies in the ids' span
    assert 2 <= decoded[1] < decoded[0] and decoded[1] == 2            # blocks 0 and 7 hold the ids' chunks, 1 .. 6 meet none


def test_view(ctx):
    rng = np.random.default_rng(7101)
    S = [sorted_unique(rng, int(rng.integers(1, 1500)), 30_000) for _ in range(12)]
    src = [0, -1, 1, 2, -1, -1, 3] + list(range(4, 12)) + [-1]
    base = ctx.encode_lists(S)
    view = ctx.select(base, src)                                       # a view with empty slots
    V = [S[j] if j >= 0 else np.empty(0, np.uint32) for j in src]
    ranges = [[(0, 0, 4)], [(0, 4, 6)], [(0, 3, 9), (1, 0, 1)], [(0, 9, len(src))]]
    case = ec.Case("view", [V, S], ranges, rng.permutation(sorted_unique(rng, 500, 30_000)).astype(np.uint32))
    segs = [view, base]
    got, st = explain(ctx, [[(segs[s], a, b) for s, a, b in g] for g in case.groups], case.ids)
    want = case.expect()
    assert np.array_equal(got, want) and want.any()
    check_stats(st, case, want)


def test_windows(ctx):
    rng = np.random.default_rng(7102)
    lists = [sorted_unique(rng, int(rng.integers(1, 1500)), 10_000) + 777 for _ in range(40)]
    groups = [[(0, 5 * g, 5 * g + 5)] for g in range(8)]
    inside = sorted_unique(rng, 700, 9_000) + 1500
    ids = rng.permutation(np.concatenate([inside, [3, 500, 776, 12_000, 70_000]])).astype(np.uint32)      # some outside the lists' span
    case = ec.Case("windows", [lists], groups, ids)
    want = case.expect()
    outside = (ids < min(l[0] for l in lists)) | (ids > max(l[-1] for l in lists))
    assert outside.sum() == 5 and not want[outside].any() and want[~outside].any()
    got, st = run_case(ctx, case)
    assert np.array_equal(got, want)
    check_stats(st, case, want, windows=1)
    lo = max(min(int(l[0]) for l in lists), int(ids.min()))
    hi = min(max(int(l[-1]) for l in lists), int(ids.max()))
    n_win = (hi - (lo & ~2047)) // 2048 + 1
    assert n_win >= 3
    for skip in (1, 0):
        with Option(ctx, "union.many_window_log2", 11, 30), Option(ctx, "count.summary_skip", skip, 1):
            got, st = run_case(ctx, case)
            assert np.array_equal(got, want), skip
            check_stats(st, case, want, windows=n_win)


def test_explains_a_ranked_page(ctx):
    rng = np.random.default_rng(7103)
    lists = [sorted_unique(rng, int(n), 8000) for n in rng.integers(100, 900, 9)]     # (46 docs score 3, the rest of the page 2)
    seg = ctx.encode_lists(lists)
    groups = [[(seg, 0, 2)], [(seg, 2, 3)], [(seg, 3, 6)], [(seg, 6, 7)], [(seg, 7, 9)]]
    d_ids, d_scores, n = ctx.topk_ranges(groups, 50)
    assert n == 50
    page, scores = d_ids.download(n), d_scores.download(n)
    assert np.any(np.diff(page.astype(np.int64)) < 0)                   # score-descending: the ids do not ascend
    masks, st = ctx.explain_ranges(groups, d_ids, n, stats=True)
    got = masks.download(n * st.n_words).reshape(masks.shape)
    assert [bin(int(m)).count("1") for m in got[:, 0]] == scores.tolist()
    want = ec.truth([[lists[j] for j in range(a, b)] for ((_, a, b),) in groups], page)
    assert np.array_equal(got, want) and st.n_hits == int(scores.sum())


def test_a_wave_walks_several_blocks_across_range_ends(ctx):
    """More blocks than 2 x 32 waves per CU: every wave of k_ex_match walks three blocks, and range (group) ends fall inside its run."""
    rng = np.random.default_rng(7106)
    D = 1 << 22
    segments, ranges, per_wave = one_block_lists_past_a_wave(rng, D)
    flat = np.concatenate([segments[s][j] for s, a, b in ranges for j in range(a, b)])
    page = np.union1d(rng.choice(flat, 150, replace=False), sorted_unique(rng, 150, D)).astype(np.uint32)
    ids = rng.permutation(page).astype(np.uint32)
    k = int(np.flatnonzero(np.isin(ids, flat))[0])                                        # a repeated id that hits: its first row keeps the mask
    ids = np.insert(ids, [k + 30, k + 150], [ids[k], ids[k]]).astype(np.uint32)
    case = ec.Case("past_a_wave", segments, [[r] for r in ranges[:4]] + [ranges[4:]], ids)    # five groups, the last of two ranges
    want = case.expect()
    n_blocks = sum(b - a for _, a, b in ranges)
    assert per_wave >= 3 and case.n_blocks == n_blocks > 2 * 32 * torch.cuda.get_device_properties(0).multi_processor_count
    assert ec.popcount(want) >= 150 and want[k].any() and not want[[k + 30, k + 151]].any() and np.all(ids[[k + 30, k + 151]] == ids[k])
    for skip in (0, 1):
        with Option(ctx, "count.summary_skip", skip, 1):
            got, st = run_case(ctx, case)
            assert np.array_equal(got, want), skip
            check_stats(st, case, want)


def raw(ctx, group_first, ranges, d_ids, n_ids, d_masks, cap, stats=None, n_groups=None):
    """the return code of one ii2_explain_ranges call: group_first an array or None (NULL), d_ids / d_masks DeviceArrays or None"""
    n = len(ranges)
    segs = (C.c_void_p * max(n, 1))(*[s.h if s is not None else None for s, _, _ in ranges])
    first = (C.c_uint64 * max(n, 1))(*[a for _, a, _ in ranges])
    end = (C.c_uint64 * max(n, 1))(*[b for _, _, b in ranges])
    gf = (C.c_uint64 * len(group_first))(*group_first) if group_first is not None else None
    if n_groups is None:
        n_groups = len(group_first) - 1
    return ctx.lib.ii2_explain_ranges(ctx.h, n_groups, gf, segs, first, end, d_ids.data_ptr() if d_ids is not None else None, n_ids,
                                      d_masks.data_ptr() if d_masks is not None else None, cap, C.byref(stats) if stats is not None else None)


def test_protocol(ctx):
    rng = np.random.default_rng(7104)
    lists = [sorted_unique(rng, 500, 50_000) for _ in range(10)]
    seg = ctx.encode_lists(lists)
    ids = rng.permutation(sorted_unique(rng, 300, 50_000)).astype(np.uint32)
    d_ids = ctx.empty(ids.size).upload(ids)
    good_gf, good = [0, 1, 3], [(seg, 0, 4), (seg, 4, 5), (seg, 2, 10)]
    want = ec.truth([lists[0:4], lists[4:5] + lists[2:10]], ids)
    d_masks = ctx.empty(ids.size, np.uint64)
    stats = _lib.ExplainStats()

    def untouched():
        return np.all(d_masks.download() == PATTERN) and stats.n_ids == 77 and stats.n_words == 0

    assert raw(ctx, good_gf, good, d_ids, ids.size, d_masks, ids.size, stats) == 0          # (the call's buffers are grown)
    assert np.array_equal(d_masks.download().reshape(-1, 1), want) and stats.n_ids == ids.size and stats.n_hits == ec.popcount(want)
    d_masks.upload(np.full(ids.size, PATTERN, np.uint64))
    stats = _lib.ExplainStats()
    stats.n_ids = 77
    for gf, ranges in (([0, 1], [(seg, 5, 4)]), ([0, 1], [(seg, 0, 11)]), ([0, 2], [(seg, 0, 3), (None, 0, 1)]),      # bad ranges, no segment
                       ([0, 2, 1], good), ([1, 2, 3], good), (None, good)):                                          # group_first
        n_groups = 2 if gf is None else None
        assert raw(ctx, gf, ranges, d_ids, ids.size, d_masks, ids.size, stats, n_groups) == -1, (gf, ranges)
        assert untouched()
    assert raw(ctx, good_gf, good, None, ids.size, d_masks, ids.size, stats) == -1          # ids is NULL
    assert raw(ctx, good_gf, good, d_ids, ids.size, None, ids.size, stats) == -1            # masks is NULL
    assert raw(ctx, good_gf, good, d_ids, ids.size, d_masks, ids.size - 1, stats) == -4     # one word short
    assert untouched()
    # more ids than a call takes: II2_ERANGE before the pointer is looked at (it holds 300 ids)
    assert raw(ctx, good_gf, good, d_ids, _lib.II2_EXPLAIN_MAX_IDS + 1, d_masks, 1 << 40, stats) == -5
    assert untouched()
    # nothing to do: no id, or no group - nothing launched or written, the device pointers may be NULL
    with path_delta(ctx) as d:
        assert raw(ctx, good_gf, good, None, 0, None, 0, stats) == 0
        assert (stats.n_ids, stats.n_words, stats.n_lists, stats.n_windows, stats.log2_slots) == (0, 1, 13, 0, 0)
        assert raw(ctx, [0], [], None, ids.size, None, 0, stats) == 0
        assert (stats.n_ids, stats.n_words, stats.n_lists, stats.n_hits) == (ids.size, 0, 0, 0)
        assert raw(ctx, None, [], d_ids, ids.size, d_masks, ids.size, None, n_groups=0) == 0
    assert d == {} and np.all(d_masks.download() == PATTERN)
    # stats may be NULL; the context goes on working
    assert raw(ctx, good_gf, good, d_ids, ids.size, d_masks, ids.size, None) == 0
    assert np.array_equal(d_masks.download().reshape(-1, 1), want)


def test_scratch_stays_clean_and_contexts_agree(ctx):
    rng = np.random.default_rng(7105)
    D = 400_000
    lists = [sorted_unique(rng, int(rng.integers(1, 3000)), D) for _ in range(80)]
    ids = rng.permutation(sorted_unique(rng, 20_000, D)).astype(np.uint32)
    groups = [[(0, 8 * g, 8 * g + 8)] for g in range(5)]
    want = ec.Case("scratch", [lists], groups, ids).expect()
    other = Context(0)
    try:
        for c in (ctx, other):
            seg = c.encode_lists(lists)
            got, st = explain(c, [[(seg, a, b) for _, a, b in g] for g in groups], ids)
            assert np.array_equal(got, want) and st.n_hits == ec.popcount(want)
            with path_delta(c) as d:
                out, n = c.union_ranges([(seg, 0, 80)])                    # more than 64 lists: the same bitmap - nothing of the ids may be left in it
            assert d.get("or.many") == 1, d
            assert np.array_equal(out.download(n), np.unique(np.concatenate(lists)))
            dset = np.sort(ids[:5000])
            counts, _ = c.count_ranges([(seg, 0, 80)], c.empty(dset.size).upload(dset), dset.size)
            assert np.array_equal(counts, [np.count_nonzero(np.isin(l, dset)) for l in lists])
            got, _ = explain(c, [[(seg, a, b) for _, a, b in g] for g in groups], ids)       # ... and nothing of those two
            assert np.array_equal(got, want)
    finally:
        other.close()
