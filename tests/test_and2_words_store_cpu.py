"""The case table of the word kernel's id stores (tests/and2_words_store_cases.py) without a device: every case has the property
it is named for - on the numpy reference -, the window arithmetic gives np.intersect1d on it, the pair is one the dense path
takes, and the capacities of the capacity case lie inside the window's result."""
import numpy as np
import pytest

from tests import and2_words_cases as wc
from tests import and2_words_store_cases as sc
from tests import dense_form_cases as dc


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_case_has_its_property_and_takes_the_dense_path(case):
    x, y, removed = case.data()
    want = wc.reference(x, y, removed)
    lo, words = wc.result_words(x, y, removed)
    assert np.array_equal(wc.ids_of(lo, words), want)
    assert int(sc.chunk_counts(words).sum()) == want.size
    assert case.check(x, y, removed, lo, words)
    B, A = dc.roles(x, y)
    assert B is x and dc.blocks(B) >= dc.MIN_BLOCKS and dc.docs_per_block(B) <= dc.MAX_DOCS_PER_BLOCK
    assert np.all(np.diff(x.astype(np.int64)) > 0) and np.all(np.diff(y.astype(np.int64)) > 0)


def test_round_layout():
    assert sc.round_layout(0, 1536) == (0, 1536, 0)
    assert sc.round_layout(1, 1536) == (3, 1532, 1)
    assert sc.round_layout(6, 1536) == (2, 1532, 2)
    assert sc.round_layout(7, 2) == (1, 0, 1)
    assert sc.round_layout(5, 2) == (2, 0, 0)
    assert sc.S == 1536 and sc.CHUNK_DOCS == 8192


def test_the_capacity_positions_are_inside_the_window():
    x, y, _ = sc.BY_NAME["capacity"].data()
    want = wc.reference(x, y)
    pos, (p, h, nb, t) = sc.capacity_positions(x, y)
    assert sorted(pos) == ["body", "head", "tail"]
    assert all(0 < v < want.size - 1 for v in pos.values())
    assert p == 2 + sc.CAP_WAVE * sc.WAVE_DOCS and h and nb and t


def test_the_removed_ids_are_in_a_head_and_in_a_body():
    x, y, removed = sc.BY_NAME["residues_removed"].data()
    _, w = wc.result_words(x, y)
    st = sc.chunk_starts(w)
    want = wc.reference(x, y)
    place = np.searchsorted(want, removed)
    assert np.array_equal(want[place], removed)
    starts = [int(st[2 * k + 1, 0, 0]) for k in range(sc.RESIDUES)]
    for head_id, body_id in place.reshape(-1, 2):
        p = max(s for s in starts if s <= head_id)
        h, nb, _ = sc.round_layout(p, sc.S)
        assert p <= head_id < p + h <= body_id < p + h + nb
