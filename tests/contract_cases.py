"""The two contracts every query entry point keeps, as tables to run the path cases under (tests/path_cases.py: for every kernel
path the smallest input that reaches it, with its numpy reference).

Tombstones.  ii2_tomb_create sizes the bitmap by the largest removed id - n_words = (max >> 5) + 1 words, every doc past them is
"not removed" -, pads it with 4 to 7 zero words and follows it with a summary of one bit per 16 docs (32 such bits: 512 docs a
summary word).  Every kernel reads that bitmap with code of its own, and removed ids spread over the lists' whole range never show
a reader that is wrong at the bitmap's END.  A layout here is a function (R, E) -> removed ids, R being the sorted union of the
call's results without tombstones and E every id of every list; each puts the bitmap's last word, or its summary, where a reader
can go wrong (LAYOUTS).  The reference of a (case, layout) pair is path_cases.reference(case, lists, removed).  The readers the path
table does not reach take the layouts with R and E of their own: the two-list AND instances, ii2_merge_segments, ii2_count_ranges,
ii2_histogram_ranges (R: the ids of the set, or of the lists, that hit; reference: hist_cases.truth), ii2_histogram_ids (R = E = the
set), ii2_atleast_ranges and the ranked calls.

Capacity.  A result that does not fit `cap` is II2_ECAPACITY (include/ii2.h); capacities(n) are the values of `cap` a result of n
ids runs at: exactly enough, one too few, none.

Pure numpy.  tests/test_contract_cases_cpu.py proves that every (case, layout) pair does what LAYOUTS says of it,
tests/test_gpu_path_contracts.py runs the pairs and the capacities on the device."""
import numpy as np

from tests import path_cases as pc

GROUP_SHIFT = 4               # docs per summary bit: 1 << 4 (csrc/internal.h: TOMB_SUM_SHIFT)
SUMMARY_SHIFT = 9             # docs per summary word: 32 bits x 16 docs
TOP = 0xFFFFFFFF

# name -> what the layout aims at
LAYOUTS = {
    "empty": "no removed id: a tombstone object that is not NULL with n_words == 0",
    "one_hit_last": "{h}, h the middle hit: the bitmap's last word holds one bit, a hit; the hits above h's word lie past the bitmap",
    "one_hit_last_other_parity": "one hit about a third into R whose word index has the other parity than h's: the last word is once "
                                 "the first and once the second word of a reader that loads the words in pairs",
    "last_word_full": "all 32 ids of h's word and every third hit below it: a reader that clamps to the last word without zeroing "
                      "wipes out everything above",
    "summary_neighbours": "for every 4th hit the other docs of its 16-doc group that are no hits, and every (4 i + 2)th hit itself: "
                          "the summary says 'maybe' where the bitmap says 'no', and hits are removed in the same summary words",
    "all_hits": "R: count 0, nothing written",
    "far_beyond": "every third hit and one id 2^20 past every list (at most 2^32 - 1): the bitmap reaches far past every list",
}
ENDS_INSIDE = ("one_hit_last", "one_hit_last_other_parity", "last_word_full")      # the bitmap ends in the middle of the results
# the cases of the path table that exist only with tombstones (every other case has a "_tomb" twin or runs without)
TOMB_ONLY = ("and_dense3", "or_small_8192_postings", "or_rank_8_lists", "or_stream3", "or_merge_whole_id_space", "or_many_count_first")
# the cases no layout runs on: fewer than two result ids (the CPU test proves that these are all of them)
DEGENERATE = ("and_tiles_sub_driver_of_1",)
# the cases where summary_neighbours leaves no removed hit in one 512-doc summary word with a survivor: some forty hits, thousands
# of docs apart - no layout could.  Neither takes the merge passes, the only reader of the summary.
NO_SHARED_SUMMARY_WORD = ("and_tiles_three_lists", "and_tiles_wide_sub_sparse_driver")
# the cases of tests/merge_cases.py that ii2_merge_segments runs under the layouts (R = the merged ids): a bitmap tile, a range tile
# and small terms only, which count no event; both kinds of leaves of a bisection after a batch is redone; bitmap leaves whose
# bounds are no multiples of 32
MERGE_CASES = ("bitmap_at_span_80n", "range_at_target", "small_at_small_max", "fold_17_small_batch_redo", "clustered_overfull_bitmap_leaves")


def distinct_path_cases():
    """path_cases.CASES without the "_tomb" twins: every case runs under the layouts whatever its own tomb flag says."""
    names = {c.name for c in pc.CASES}
    out = [c for c in pc.CASES if not (c.name.endswith("_tomb") and c.name[:-len("_tomb")] in names)]
    assert all(c.tomb == (c.name in TOMB_ONLY) for c in out)
    return out


PATH_CASES = distinct_path_cases()


def hits(results):
    """R: the sorted union of a call's results (one array per query), uint64"""
    return np.unique(np.concatenate([np.asarray(r, np.uint64) for r in results] + [np.empty(0, np.uint64)]))


def every_id(lists):
    """E: every id of every list, sorted, uint64"""
    return np.unique(np.concatenate([np.asarray(l, np.uint64) for l in lists] + [np.empty(0, np.uint64)]))


def sets_of(case, lists):
    """(R, E) of a path case"""
    return hits(pc.reference(case, lists)), every_id(lists)


def middle(R):
    return int(R[R.size // 2])


def other_parity_hit(R):
    """the hit nearest to a third into R whose word index has the other parity than the middle hit's; None when there is none"""
    odd = (R >> np.uint64(5)) & np.uint64(1)
    idx = np.flatnonzero(odd != ((middle(R) >> 5) & 1))
    if not idx.size:
        return None
    return int(R[idx[np.argmin(np.abs(idx - R.size // 3))]])


def removed_for(layout, R, E):
    """the removed ids of a layout, ascending uint32 - or None when R cannot carry it (fewer than two hits; every hit in words of
    one parity)"""
    R, E = np.asarray(R, np.uint64), np.asarray(E, np.uint64)
    if R.size < 2:
        return None
    if layout == "empty":
        ids = []
    elif layout == "one_hit_last":
        ids = [middle(R)]
    elif layout == "one_hit_last_other_parity":
        x = other_parity_hit(R)
        if x is None:
            return None
        ids = [x]
    elif layout == "last_word_full":
        first = middle(R) & ~31
        ids = np.concatenate([np.arange(first, first + 32, dtype=np.uint64), R[R < first][::3]])
    elif layout == "summary_neighbours":
        group = (R[::4] >> np.uint64(GROUP_SHIFT)) << np.uint64(GROUP_SHIFT)
        near = (group[:, None] + np.arange(1 << GROUP_SHIFT, dtype=np.uint64)[None, :]).ravel()
        ids = np.concatenate([np.setdiff1d(near, R), R[2::4]])
    elif layout == "all_hits":
        ids = R
    elif layout == "far_beyond":
        ids = np.concatenate([R[::3], [min(int(E[-1]) + (1 << 20), TOP)]]).astype(np.uint64)
    else:
        raise ValueError(layout)
    ids = np.unique(np.asarray(ids, np.uint64))
    assert not ids.size or int(ids[-1]) <= TOP
    return ids.astype(np.uint32)


def n_words(removed):
    """words of the bitmap ii2_tomb_create makes for these ids"""
    return (int(np.max(removed)) >> 5) + 1 if len(removed) else 0


def last_word(removed):
    """the bitmap's last word: bit d & 31 is set when doc d of that word is removed (0 for no removed id)"""
    r = np.asarray(removed, np.uint64)
    if not r.size:
        return 0
    bits = np.zeros(32, np.uint8)
    bits[(r[(r >> np.uint64(5)) == np.uint64(n_words(r) - 1)] & np.uint64(31)).astype(np.int64)] = 1
    return int(np.packbits(bits, bitorder="little").view("<u4")[0])


def capacities(n):
    """the capacities a result of n ids runs at: exactly enough, one too few, none"""
    return list(dict.fromkeys([n] + ([n - 1] if n > 0 else []) + [0]))
