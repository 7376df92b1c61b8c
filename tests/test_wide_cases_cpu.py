"""CPU: every case of tests/wide_cases.py reaches the regime it names, by arithmetic.  The window comes from the library itself
(ii2_atleast_plan and ii2_topkw_plan are host only); the launch shape from the constants wide_cases mirrors, with the 256 compute
units of an MI355X: workgroups and whether the last is ragged, summary words, grid-stride steps, the count table against the scan
tile, the windows, the late groups, the groups skipped per window.  And the references are worth comparing with: every class a case
names is populated, every k that is meant to cut inside a class does, the removed and excluded ids would otherwise be returned, and a
case holds at most a few thousand postings.  A case that misses its regime fails here instead of passing quietly on the GPU."""
import ctypes as C
import os

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import atleast_cases as ac
from tests import topk_cases as tc
from tests import topkw_cases as wc
from tests import wide_cases as wd
from tests.wide_cases import SW

OK = 0
DEFAULT_WLOG2 = 30               # union.many_window_log2 as a context starts with it (include/ii2.h)


def _lib_built():
    from inverted_index_2_amd import host
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(host.HOST_LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def atleast_plan(n_counted, m):
    """(n_planes, window_docs, first_late) of the counting form"""
    planes, win, late = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert _lib_built().ii2_atleast_plan(n_counted, m, DEFAULT_WLOG2, C.byref(planes), C.byref(win), C.byref(late)) == OK
    return planes.value, win.value, late.value


def topk_window(case):
    """(n_planes, window_docs) of the ranked query: exact counters, B = bit_width(n')"""
    planes, win, _ = atleast_plan(case.n_counted, case.n_counted)
    return planes, win


def topkw_plan(t, min_score):
    """(total_weight, n_planes, window_docs, late flags) of the weighted query"""
    weights, postings = [t.weights[g] for g in t.counted], t.postings
    n = len(weights)
    late = (C.c_uint8 * n)()
    total, planes, win, n_late = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint32()
    assert _lib_built().ii2_topkw_plan(n, (C.c_uint32 * n)(*weights), (C.c_uint64 * n)(*postings), min_score, DEFAULT_WLOG2, C.byref(total),
                                       C.byref(planes), C.byref(win), late, C.byref(n_late)) == OK
    assert n_late.value == sum(late)
    return total.value, planes.value, win.value, list(late)


# ---- the mirrored constants are the sources' ---------------------------------------------------------------------------------------
def test_the_constants_are_the_sources():
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "inverted_index_2_amd", "csrc")
    src = {n: open(os.path.join(csrc, n)).read() for n in ("setop.cpp", "topk.hip", "atleast.hip", "scan.hip")}
    assert "p.n_sum = (uint32_t)((docs + 65535) / 65536);" in src["setop.cpp"] and wd.SW == 65536
    for f, n in (("topk.hip", 4), ("atleast.hip", 2)):
        assert src[f].count("for (uint32_t sw = blockIdx.x * 4u + (threadIdx.x >> 6); sw < p.n_sum; sw += n_waves)") == n and wd.WAVES == 4
        assert src[f].count("const uint32_t wi = (sw * 32u + chunk) * 64u + l;") == n and wd.CHUNK == 64 * 32
    assert "grid = (uint32_t)std::min<uint64_t>((p.n_sum + 3) / 4, (uint64_t)ctx->cu_count * 8u);" in src["setop.cpp"] and wd.GRID_CUS == 8
    assert "launch_top_hist(t, std::min<uint32_t>(grid, (uint32_t)ctx->cu_count * 2u)" in src["setop.cpp"] and wd.HIST_CUS == 2
    assert "SCAN_THREADS = 256;" in src["scan.hip"] and "SCAN_PER_THREAD = 16;" in src["scan.hip"] and wd.SCAN_TILE == 256 * 16
    # thr_window_docs at its real values: 2^30, 2^29, 2^28, 2^27 docs for B = 1, 2, 3 .. 4, 5 .. 8
    assert [atleast_plan(255, m)[:2] for m in (1, 2, 4, 8, 16, 32, 64, 255)] == [(1, 1 << 30), (2, 1 << 29), (3, 1 << 28), (4, 1 << 28), (5, 1 << 27), (6, 1 << 27), (7, 1 << 27), (8, 1 << 27)]


# ---- the launch shape ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", wd.CASES, ids=lambda c: c.name)
def test_the_case_reaches_its_launch_shape(c):
    r = c.regime
    planes, win = topk_window(c.case)
    assert (planes, win) == (r["n_planes"], 1 << r["window_log2"]) and planes == c.case.n_counted.bit_length()
    n_sum = wd.n_sum_of(c.case, win)
    grid = wd.grid_of(n_sum)
    print(c.name, "planes", planes, "window", win, "n_sum", n_sum, "workgroups", grid, "steps", wd.steps_of(n_sum))
    assert n_sum == r["n_sum"] and wd.n_windows_of(c.case, win) == r["n_windows"]
    assert grid == r["workgroups"] and grid > 1                                  # more than one workgroup, always
    assert (n_sum < grid * wd.WAVES) == r["ragged"] and wd.steps_of(n_sum) == r["steps"]
    assert win % SW == 0                                                         # (word_of holds inside every window)
    assert 0 <= wd.window_span(c.case)[1] - wd.window_span(c.case)[0] < (1 << 32)
    # the threshold runs: their own planes and window; the counting form is what the chooser takes under wide_cases.COUNTING
    for case, m in c.atleast:
        p, w, first_late = atleast_plan(case.n_counted, m)
        assert p == m.bit_length() and first_late == case.n_counted - m + 1
        assert ac.expected_form(case, **{k.split(".")[1]: v for k, v in wd.COUNTING.items()}) in (ac.COUNT,) or m > case.n_counted
        assert wd.grid_of(wd.n_sum_of(case, w), extra=1) > 1


def test_three_workgroups():
    c = wd.BY_NAME["three_workgroups"]
    base, hi = wd.window_span(c.case)
    lo = min(int(l[0]) for l in c.case.lists[:3])
    assert base == lo & ~31 and lo % 32 and base % (1 << 18) and hi - base + 1 == 9 * SW          # exactly nine summary words
    ids, scores = tc.scores_of(c.case)
    everything = np.unique(np.concatenate([c.case.ids(g) for g in c.case.groups]))
    for j in range(9):                                                            # a doc at the first and at the last id of every word
        assert (lo if j == 0 else base + j * SW) in everything and base + (j + 1) * SW - 1 in everything
    tie = ids[scores == 2]
    assert np.array_equal(tie, c.named["tie"]) and sorted(set(wd.word_of(c.case, tie).tolist())) == c.regime["tie_words"] == [0, 3, 4, 8]
    # word 3: the last wave of workgroup 0; word 4: the first of workgroup 1; word 8: the only busy wave of workgroup 2
    assert (3 // wd.WAVES, 3 % wd.WAVES, 4 // wd.WAVES, 4 % wd.WAVES, 8 // wd.WAVES, 8 % wd.WAVES) == (0, 3, 1, 0, 2, 0)
    assert np.array_equal(ids[scores == 3], c.named["top"]) and wd.word_of(c.case, c.named["top"]).tolist() == c.regime["top_words"]
    alone = int(c.named["alone"][0])
    assert alone in c.case.lists[3] and wd.word_of(c.case, [alone])[0] == c.regime["alone_word"]
    assert not np.any((everything.astype(np.int64) - base) // wd.CHUNK == (alone - base) // wd.CHUNK)
    # the cuts of the tie class: behind its word-3 members, inside word 8, one past its end
    got = {k: tc.reference(c.case, k)[0:2] for k in c.top.ks}
    assert got[6][1].tolist() == [3, 3, 2, 2, 2, 2] and wd.word_of(c.case, got[6][0][2:]).tolist() == [0, 0, 3, 3]
    assert got[10][1].tolist() == [3, 3] + [2] * 8 and wd.word_of(c.case, got[10][0][-3:]).tolist() == [4, 8, 8] and tie.size == 9
    assert got[12][1].tolist() == [3, 3] + [2] * 9 + [1]
    assert set(c.regime["cuts"]) <= set(c.top.ks)


def test_two_scan_tiles():
    c = wd.BY_NAME["two_scan_tiles"]
    _, win = topk_window(c.case)
    n_sum = wd.n_sum_of(c.case, win)
    assert c.case.n_counted == 40 and all(len(g) == 1 for g in c.case.groups) and n_sum == 128
    ids, scores = tc.scores_of(c.case)
    for s in range(1, 41):                                                        # every class, each in several words
        mine = ids[scores == s]
        assert mine.size >= 5 and np.unique(wd.word_of(c.case, mine)).size >= 5, s
        assert all(np.array_equal(np.isin(mine, c.case.lists[g]), np.full(mine.size, g < s)) for g in range(40)), s
    assert np.unique(wd.word_of(c.case, ids)).size == 128                          # every summary word holds a doc
    for tomb in (False, True):
        _, _, hist = tc.reference(c.case, 0, 1, tomb)
        for k, (cut_score, table) in c.regime["tables"].items():
            mx, cs, above, n_cut = tc.cut(hist, k)
            n_cls = mx - cs + 1
            print("two_scan_tiles tomb", tomb, "k", k, "cut", cs, "n_cls", n_cls, "table", n_cls * n_sum + 1)
            assert (cs, n_cls * n_sum + 1) == (cut_score, table), (tomb, k)
            assert cut_score == 1 or 0 < n_cut < int(hist[cs])                    # the cut is inside the class
    tables = sorted(t for _, t in c.regime["tables"].values())
    assert tables == [3969, 4097, 5121] and tables[0] < wd.SCAN_TILE < tables[1] == wd.SCAN_TILE + 1 and tables[2] > wd.SCAN_TILE + 1024


def test_hist_stride():
    c = wd.BY_NAME["hist_stride"]
    _, win = topk_window(c.case)
    n_sum = wd.n_sum_of(c.case, win)
    base, hi = wd.window_span(c.case)
    assert hi - base + 1 == (1 << 27) + 2 * SW and n_sum == 2050 > wd.GRID_CUS * wd.CUS
    hist_waves = wd.grid_of(n_sum, per_cu=wd.HIST_CUS) * wd.WAVES
    assert hist_waves == 2048 and wd.steps_of(n_sum, per_cu=wd.HIST_CUS) == c.regime["hist_steps"] == 2
    ids, scores = tc.scores_of(c.case)
    words = wd.word_of(c.case, ids)
    for a, b in c.regime["pairs"]:                                                # one wave of k_top_hist meets both words, each with every score
        assert b == a + hist_waves
        for j in (a, b):
            assert set(scores[words == j].tolist()) == {1, 2, 3}, j
    assert sorted(set(words.tolist())) == [0, 1, 2046, 2047, 2048, 2049]


def test_full_stride():
    c = wd.BY_NAME["full_stride"]
    planes, win = topk_window(c.case)
    n_sum = wd.n_sum_of(c.case, win)
    base, hi = wd.window_span(c.case)
    assert (planes, win) == (1, 1 << 30) and (1 << 30) - SW < hi - base + 1 < (1 << 30) and n_sum == 16384 > 32 * wd.CUS
    waves = wd.grid_of(n_sum) * wd.WAVES
    assert waves == 8192
    assert len(c.case.groups) == 1 and len(c.case.groups[0]) == 3
    a, b, d = (c.case.lists[i] for i in c.case.groups[0])
    assert np.intersect1d(a, b).size and np.intersect1d(b, d).size and np.intersect1d(a, d).size       # the three lists overlap
    ids, scores = tc.scores_of(c.case)
    words = wd.word_of(c.case, ids)
    for x, y in c.regime["pairs"]:
        assert y == x + waves
        for j in (x, y):                                                          # several docs per word, in several chunks
            mine = ids[words == j]
            assert mine.size >= 4 and np.unique((mine.astype(np.int64) - base) // wd.CHUNK).size >= 3, j
    for k, word in c.regime["cut_in_word"].items():
        got = tc.reference(c.case, k)[0]
        assert wd.word_of(c.case, got[-1:])[0] == word and wd.word_of(c.case, ids[ids > got[-1]][:1])[0] == word and k in c.top.ks
    assert [(t.weights, t.min_scores) for t in c.weighted] == [([1], [1])]
    thr, m = c.atleast[0]
    assert (len(thr.groups), m, atleast_plan(thr.n_counted, m)[:2]) == (5, 1, (1, 1 << 30)) and thr.exclude
    assert wd.n_sum_of(thr, 1 << 30) == 16384 and np.array_equal(np.unique(np.concatenate(thr.lists[:5])), np.unique(np.concatenate([a, b, d])))
    assert ac.expected_form(thr, handoff=1, small=0) == ac.COUNT                  # excluded ids that count: no hand-off to the OR anyway


def test_default_windows():
    c = wd.BY_NAME["default_windows"]
    planes, win = topk_window(c.case)
    assert (c.case.n_counted, planes, win) == (5, 3, 1 << 28) and wd.window_span(c.case) == (0, 0xFFFFFFFF)
    assert wd.n_windows_of(c.case, win) == 16
    everything = np.unique(np.concatenate([c.case.ids(g) for g in c.case.groups]))
    assert sum(1 for w in range(1, 16) if w * win - 1 in everything and w * win in everything) == 15      # docs on both sides of every seam
    ids, scores = tc.scores_of(c.case)
    tie = ids[scores == 2]
    assert np.array_equal(tie, c.named["tie"]) and (tie // win).tolist() == list(range(16))             # exactly one member per window
    assert int(scores.max()) == 4 and np.array_equal(ids[scores == 4], c.named["top"]) and np.all(c.named["top"] // win == 15)
    assert wd.skipped(c.case, win) == c.regime["skipped"]
    assert sorted(set((c.case.lists[5] // win).tolist())) == c.regime["excluded_windows"]
    # k = 1: the highest class, found in the last window, goes in front; the middle cut takes the tie class's members of windows 0 .. 7
    assert tc.reference(c.case, 1)[0].tolist() == [int(c.named["top"][0])]
    k = [k for k in c.regime["cuts"]][0]
    got_ids, got_scores, hist = tc.reference(c.case, k)
    assert tc.cut(hist, k)[1:] == (2, k - 8, 8) and got_ids[-8:].tolist() == tie[:8].tolist() and k in c.top.ks
    assert max(c.case.removed) < (1 << 29) and (everything > max(c.case.removed)).sum() > 40              # the bitmap ends below most ids


# ---- the weighted twins --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", wd.CASES, ids=lambda c: c.name)
def test_the_weighted_twins(c):
    if c.name == "full_stride":
        assert [t.tag for t in c.weighted] == ["one"]
    else:
        assert [t.tag for t in c.weighted] == ["odd", "pow2"]
        odd, pow2 = c.weighted
        assert all(w % 2 for w in odd.weights) and any(w > 1 for w in odd.weights) and all(w & (w - 1) == 0 for w in pow2.weights)
    for t in c.weighted:
        assert t.case is c.case and t.total_weight <= wc.MAX_SCORE and len(t.weights) == len(c.case.groups)
        late_seen = False
        for m in t.min_scores:
            total, planes, win, late = topkw_plan(t, m)
            assert (total, planes) == (t.total_weight, t.total_weight.bit_length()) and late == wc.late_rule([t.weights[g] for g in t.counted], t.postings, m)
            late_seen = late_seen or any(late)
            n_sum, n_win = wd.n_sum_of(c.case, win), wd.n_windows_of(c.case, win)
            print(t.name, "min_score", m, "planes", planes, "window", win, "n_sum", n_sum, "windows", n_win, "late", late)
            # the twin keeps the case's regime: as many summary words per window or, where more planes halve the window, more windows
            assert wd.grid_of(n_sum) > 1 and n_sum * n_win >= c.regime["n_sum"] * c.regime["n_windows"]
            if c.name in ("hist_stride", "full_stride"):
                assert n_sum == c.regime["n_sum"]
            _, _, hist = wc.reference(t.case, t.weights, 0, m)
            assert hist.any()
        assert late_seen == (c.name != "full_stride"), t.name
        assert 1 <= len(t.ks) <= 8 and 0 not in t.ks


# ---- the references are not trivial --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", wd.CASES, ids=lambda c: c.name)
def test_the_references_are_not_trivial(c):
    cases = {id(case): case for case in [c.case] + [case for case, _ in c.atleast]}.values()
    for case in cases:
        assert sum(int(l.size) for l in case.lists) <= 5000, case.name
        # every removed id but the stray ones and at least one excluded id would otherwise be returned
        plain = ac.reference(case, m=1, exclude=False)
        assert np.isin(np.asarray(case.removed, np.uint32), plain).sum() >= 2, case.name
        assert np.isin(np.concatenate([case.lists[i] for g in case.exclude for i in g] + [ac.EMPTY]), plain).any() == bool(case.exclude), case.name
        assert ac.reference(case, m=1, tomb=True).size < ac.reference(case, m=1).size <= plain.size
    for case, m in c.atleast:
        assert 0 < ac.reference(case, m=m, tomb=True).size < ac.reference(case, m=m).size or m == case.n_counted, (case.name, m)
        assert ac.reference(case, m=m).size, (case.name, m)
    t = c.top
    assert t.ks == sorted(set(t.ks)) and 0 not in t.ks
    kinds = set()
    for m in t.min_matches:
        for tomb in (False, True):
            _, _, hist = tc.reference(t.case, 0, m, tomb)
            assert hist.any()
            for k in t.ks:
                _, cs, above, n_cut = tc.cut(hist, k)
                kinds.add("tie" if int(hist[cs]) > n_cut else "beyond" if k > int(hist.sum()) else "whole")
        for k in t.ks:
            a, b = tc.reference(t.case, k, m), tc.reference(t.case, k, m, tomb=True)
            assert not np.array_equal(a[2], b[2])                                  # the tombstones change the histogram
    assert kinds >= {"tie", "beyond"} or c.name == "two_scan_tiles" and kinds >= {"tie", "whole"}, (c.name, kinds)
