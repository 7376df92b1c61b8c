"""The case table of the word-by-word two-list AND (tests/and2_words_cases.py, tests/dense_form_cases.py) without a device: the
window arithmetic in plain numpy - the window's first word and length, a form's word offset into it, which words read as zero -
gives np.intersect1d on every case, every new case has the property it is named for, and every pair is one the dense path takes."""
import numpy as np
import pytest

from tests import and2_words_cases as wc
from tests import dense_form_cases as dc

ALL = [(c.name, c) for c in dc.CASES] + [(c.name, c) for c in wc.CASES]


@pytest.mark.parametrize("name,case", ALL, ids=[n for n, _ in ALL])
def test_the_window_arithmetic_gives_the_intersection(name, case):
    x, y, removed = case.data()
    want = wc.reference(x, y, removed)
    lo, words = wc.result_words(x, y, removed)
    assert np.array_equal(wc.ids_of(lo, words), want)
    assert int(wc.per_workgroup(words).sum()) == want.size
    assert wc.per_workgroup(words).size == wc.workgroups(x, y)
    if words.size:                                                   # nothing outside the window can be a hit
        assert int(want[0]) >> 5 >= lo and int(want[-1]) >> 5 < lo + words.size


@pytest.mark.parametrize("case", wc.CASES, ids=lambda c: c.name)
def test_new_case_has_its_property_and_takes_the_dense_path(case):
    x, y, removed = case.data()
    lo, words = wc.result_words(x, y, removed)
    assert case.check(x, y, removed, lo, words)
    B, A = dc.roles(x, y)
    assert B is x and dc.blocks(B) >= dc.MIN_BLOCKS and dc.docs_per_block(B) <= dc.MAX_DOCS_PER_BLOCK
    assert np.all(np.diff(x.astype(np.int64)) > 0) and np.all(np.diff(y.astype(np.int64)) > 0)


def test_zero_reads():
    """words from the window's end on do not exist; tombstone words past that bitmap's end read as zero"""
    x, y, removed = dc.BY_NAME["tombstones"].data()
    lo, n = wc.window(x, y)
    t = wc.tomb_words(removed, lo, n)
    nw = (int(removed[-1]) >> 5) + 1
    assert nw < n and not np.any(t[nw - lo:]) and np.any(t[:nw - lo])
    assert wc.tomb_words(None, lo, n).sum() == 0
    for case in ("b_wider", "a_wider"):                              # a form reaches beyond the window on both sides: its offset, its rest
        x, y, _ = dc.BY_NAME[case].data()
        lo, n = wc.window(x, y)
        offs = sorted(wc.form_offset(l, lo) for l in (x, y))
        assert offs[0] == 0 and offs[1] > 4 * dc.CAPW // 32
        wide = x if wc.form_offset(x, lo) else y
        assert dc.form_words(wide).size > wc.form_offset(wide, lo) + n + 4 * dc.CAPW // 32


def test_the_rule_keeps_the_table_on_the_present_kernels():
    """the default threshold (iii) is CUs x workgroups per CU x 16 blocks - 16 384 blocks on an MI355X - and no B of either
    table reaches it, while the `uniform` pair passes an injected 1024"""
    for _, case in ALL:
        x, y, _ = case.data()
        assert dc.blocks(dc.roles(x, y)[0]) < 256 * 64, case.name
    x, y, _ = dc.BY_NAME["uniform"].data()
    B, A = dc.roles(x, y)
    assert dc.blocks(B) >= 1024 and dc.criterion_b(A) and dc.criterion_b(B)
    assert wc.workgroups(x, y) == 13 != (dc.blocks(B) + dc.WG_BLOCKS - 1) // dc.WG_BLOCKS == 17
    x, y, _ = dc.BY_NAME["criterion"].data()
    B, A = dc.roles(x, y)
    assert not dc.criterion_b(A)
