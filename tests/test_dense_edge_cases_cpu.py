"""CPU: the table of the dense family at the edges of the id space (tests/dense_edge_cases.py) is sound - every shifted case still
is the case it was moved from, still goes to the dense kernels, really sits where its name says, and the numpy restatement of the
word kernel's window arithmetic is exact at these ids."""
import numpy as np
import pytest

from tests import and2_words_cases as wc
from tests import dense_edge_cases as de
from tests import dense_form_cases as dc

EDGES = pytest.mark.parametrize("edge", de.EDGES, ids=lambda e: e.name)


def test_the_table_holds_the_cases_and_the_edges_asked_for():
    names = {e.name for e in de.EDGES}
    for s in ("uniform", "alignment_last_bit31", "gap_in_b", "tombstones_whole_window", "stretches_removed", "one_word", "offset_1", "offset_3"):
        assert f"{s}@top" in names
    assert {"uniform@mid", "gap_in_b@mid", "offset_1@mid"} <= names
    assert de.UNIT == wc.WG_DOCS == 65536 and de.UNIT % 128 == 0 and de.UNIT % dc.CAPW == 0
    tombstoned = [e for e in de.EDGES if e.case.data()[2] is not None]
    assert {e.source for e in tombstoned} >= {"tombstones_whole_window", "stretches_removed", "offset_1", "offset_3"}
    assert all(len(e.data()[2]) == (2 if e.at == "top" else 1) for e in tombstoned)
    modes = {m.name: m for m in de.MODES}
    assert list(modes) == ["dense2", "dense2_bpw32", "split", "fused_marking", "fused_form", "fused_form_x2", "words", "dense3", "union"]
    assert all(m.tombstones for m in de.MODES[:8])
    assert all(set(m.options) <= set(de.DEFAULTS) for m in de.MODES)             # every option a mode sets has a default to go back to


@EDGES
def test_a_shifted_case_is_the_case_it_was_moved_from(edge):
    x0, y0, r0 = edge.case.data()
    x, y, sets, by = edge.data()
    assert by > 0 and by % de.UNIT == 0
    added = [de.TOP, de.TOP - 1] if edge.at == "top" else []
    assert np.array_equal(np.setdiff1d(x, added), de.moved(x0, by)[de.moved(x0, by) < de.TOP - 1])
    assert np.array_equal(np.setdiff1d(y, added), de.moved(y0, by)[de.moved(y0, by) < de.TOP - 1])
    assert (dc.roles(x, y)[0] is x) == (dc.roles(x0, y0)[0] is x0)               # the added docs change no list's role
    assert (r0 is None) == (not sets)
    if sets:
        assert np.array_equal(sets[0], de.moved(r0, by))
    assert edge.source_holds()                                                   # the source case's own predicate
    # alignment: the forms' origins, the window's first word modulo 4 and the workgroup boundaries are the source's
    assert all(dc.form_origin(l) - by == dc.form_origin(l0) for l, l0 in ((x, x0), (y, y0)))
    lo, lo0 = wc.window(x, y)[0], wc.window(x0, y0)[0]
    assert lo - lo0 == by >> 5 and lo % 4 == lo0 % 4 and (lo - lo0) % wc.W == 0


@EDGES
def test_both_lists_meet_the_dense_chooser(edge):
    x, y, sets, by = edge.data()
    for l in (x, y):
        assert dc.blocks(l) >= dc.MIN_BLOCKS and 0 < dc.docs_per_block(l) <= dc.MAX_DOCS_PER_BLOCK
    t = edge.third()
    assert de.dense_driver([x, y]) and de.dense_driver([x, y, t]) and dc.blocks(t) > min(dc.blocks(x), dc.blocks(y))
    assert de.stream_pacer([x, y]) == (edge.source != "one_word")                # (its lists lie one behind the other: no pacer)
    assert x.dtype == y.dtype == t.dtype == np.uint32
    assert all(np.all(np.diff(l.astype(np.int64)) > 0) for l in (x, y, t))


@EDGES
def test_the_window_arithmetic_is_exact_at_these_ids(edge):
    x, y, sets, by = edge.data()
    x0, y0, r0 = edge.source_coordinates()
    for removed in [None] + sets:
        want = de.reference([x, y], removed)
        lo, w = wc.result_words(x, y, removed)
        ids = wc.ids_of(lo, w)
        assert ids.dtype == np.uint32 and np.array_equal(ids, want)
        assert int(wc.per_workgroup(w).sum()) == want.size
    # word for word what the same lists give next to doc 0: nothing wrapped on the way up
    lo, w = wc.result_words(x, y, sets[0] if sets else None)
    lo0, w0 = wc.result_words(x0, y0, r0)
    assert lo - lo0 == by >> 5 and np.array_equal(w, w0)
    for l, l0 in ((x, x0), (y, y0)):
        f = dc.form_words(l)
        assert f.size == dc.form_bytes(l) // 4 and np.array_equal(f, dc.form_words(l0))
        assert np.array_equal(wc.ids_of(dc.form_origin(l) >> 5, f), l)           # the form's bits are the list
    if sets:
        n = wc.window(x, y)[1]
        t = wc.tomb_words(sets[0], lo, n)
        assert np.array_equal(t, wc.tomb_words(r0, lo0, n))
        inside = sets[0][(sets[0] >> 5 >= lo) & (sets[0] >> 5 < lo + n)]
        assert np.array_equal(wc.ids_of(lo, t), inside)


@EDGES
def test_the_case_sits_where_its_name_says(edge):
    x, y, sets, by = edge.data()
    B, A = dc.roles(x, y)
    want = de.reference([x, y])
    if edge.at == "mid":
        assert de.straddles(x) and de.straddles(y)
        assert want[0] < de.HALF < want[-1]                                      # hits on both sides
        assert abs(float(np.median(np.concatenate([x, y]))) - de.HALF) < 64 * de.UNIT
        for r in sets:
            assert r[0] < de.HALF and de.tomb_bitmap_words(r) < de.TOMB_WORDS_ALL
        return
    assert max(int(x[-1]), int(y[-1])) == de.TOP
    assert de.TOP - by - max(int(l[-1]) for l in edge.case.data()[:2]) < de.UNIT     # the largest shift that fits
    if edge.source in de.TOP_IN_ONE_LIST:
        assert int(B[-1]) == de.TOP and de.TOP not in want and wc.window(x, y)[1] == 1
    else:
        assert int(B[-1]) == int(A[-1]) == want[-1] == de.TOP                    # a hit ...
        for l in (B, A):                                                         # ... and the last bit of the last word of both forms
            assert dc.form_origin(l) + 32 * (dc.form_bytes(l) // 4) == 1 << 32 and dc.form_words(l)[-1] >> 31 == 1
        assert B[-2] == de.TOP - 1 and de.TOP - 1 not in A and de.TOP - 1 not in want
    if sets:
        first, second = sets
        assert de.tomb_bitmap_words(first) < sum(wc.window(x, y)) - 2 * wc.W     # words past the bitmap's end: the window's last workgroups
        assert de.tomb_bitmap_words(second) == de.TOMB_WORDS_ALL                 # the bitmap ends at word 2^27 - 1: none
        assert int(second[-1]) >> 5 == int(x[-1]) >> 5 == int(y[-1]) >> 5 if edge.source not in de.TOP_IN_ONE_LIST else True
        gone = np.setdiff1d(second, first)
        assert gone.size == 2 and gone[-1] == de.TOP - 1 and gone[0] == want[-2]                 # (the source case's last hit)
        assert de.reference([x, y], second).size == de.reference([x, y], first).size - 1 and de.reference([x, y], second)[-1] == de.TOP
