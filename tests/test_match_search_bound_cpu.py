"""CPU: the output bound the host mirror gives one name of PrefixSearch / MatchSearch before it unions the name's list ranges
(host/host_index.cpp: union_bound, through the test entry ii2h_union_bound).  A prefix has one range per segment; a substring
search has one range per RUN, any number of them in one segment, and they hold no more postings than the segment does: every
distinct segment counts once.  Counting it once per run would push a pattern with many runs in a large segment past the batch
call's limit of 2^32 ids and into an allocation of runs x postings."""
from inverted_index_2_amd.host import union_bound

CALL_IDS = 0xFFFFFFFF


def test_one_range_per_segment_is_the_sum():
    assert union_bound([0, 1, 2], [10, 20, 30]) == 60
    assert union_bound([2, 0], [10, 20, 30]) == 40                     # a segment without a range does not count
    assert union_bound([], [10]) == 0 and union_bound([0], [0]) == 0


def test_many_runs_in_one_segment_count_it_once():
    assert union_bound([0] * 95, [100_000_000]) == 100_000_000         # 95 runs of a glob in a segment of 10^8 postings
    assert union_bound([0] * 100_000, [100_000_000]) < CALL_IDS        # 10^5 runs of a substring: still one batch query
    assert union_bound([0, 0, 1, 0, 1, 1, 0], [7, 5]) == 12


def test_runs_of_several_segments_in_any_order():
    seg = [s for _ in range(1000) for s in (3, 1, 2)]                  # interleaved, as chunks of dictionaries may leave them
    assert union_bound(seg, [1 << 40, 11, 13, 17]) == 41
    assert union_bound(sorted(seg), [1 << 40, 11, 13, 17]) == 41
    assert union_bound([0, 1, 0, 1], [1 << 33, 1 << 33]) == 1 << 34    # above 2^32 it is still the plain sum: no wrap
