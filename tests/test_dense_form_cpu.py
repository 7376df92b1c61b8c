"""CPU: the case table of the dense form (tests/dense_form_cases.py) says what it claims - every pair reaches the thresholds of
the one-launch two-list AND, criterion (b) holds or fails as the case says, every property a case was built for is there, and
the references are not trivial.  No device."""
import numpy as np
import pytest

from tests import dense_form_cases as dc


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_case_reaches_the_dense_two_list_path(case):
    x, y, _ = case.data()
    B, A = dc.roles(x, y)
    for l in (B, A):
        assert l.dtype == np.uint32 and np.all(np.diff(l.astype(np.int64)) > 0)
    assert dc.blocks(B) < dc.blocks(A)                                  # no tie: the roles do not hang on the order of the lists
    assert dc.blocks(B) >= dc.MIN_BLOCKS and 0 < dc.docs_per_block(B) <= dc.MAX_DOCS_PER_BLOCK
    assert dc.blocks(B) > 16 * dc.WG_BLOCKS                             # 17 workgroups at the least


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_criterion_b_is_what_the_case_says(case):
    x, y, _ = case.data()
    _, A = dc.roles(x, y)
    assert dc.criterion_b(A) == case.form, (dc.form_bytes(A), dc.payload_bytes(A))
    if not case.form:                                                   # ... and not by a hair: one posting per 5 docs is at 5 / 8
        assert 2 * dc.form_bytes(A) > 1.15 * dc.payload_bytes(A)
    else:
        assert 2 * dc.form_bytes(A) < 0.9 * dc.payload_bytes(A)


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_case_has_the_properties_it_was_built_for(case):
    x, y, removed = case.data()
    B, A = dc.roles(x, y)
    assert (removed is not None) == case.removed
    for name, pred in case.checks.items():
        assert pred(B, A, removed), name


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_references_are_not_trivial(case):
    x, y, removed = case.data()
    B, A = dc.roles(x, y)
    want = dc.reference(case)
    assert 1000 < want.size < B.size
    if removed is not None:
        assert want.size < np.intersect1d(x, y, assume_unique=True).size - 100
    words = dc.form_words(A)
    assert words.size * 4 == dc.form_bytes(A)
    assert int(sum(bin(int(w)).count("1") for w in words[:64])) == np.count_nonzero(A < dc.form_origin(A) + 64 * 32)
    assert words[0] != 0 and words[-1] != 0                             # the first and the last doc
    # bit by bit, the slow way, on a sample
    o = dc.form_origin(A)
    rng = np.random.default_rng(0)
    docs = rng.integers(o, int(A[-1]) + 1, 2000)
    inA = np.isin(docs, A)
    got = (words[(docs - o) >> 5] >> ((docs - o) & 31).astype(np.uint32)) & 1
    assert np.array_equal(got.astype(bool), inA)


def test_swapped_case_is_the_same_pair_in_the_other_order():
    x, y, _ = dc.BY_NAME["uniform"].data()
    ys, xs, _ = dc.BY_NAME["uniform_swapped"].data()
    assert np.array_equal(x, xs) and np.array_equal(y, ys)
    assert dc.blocks(x) < dc.blocks(y)                                  # "uniform" names B first, the swapped case A first
