"""No GPU: the host-only parts of ii2_explain_ranges - ii2_explain_slot against its restatement, the prototypes, the stats
struct - and the case table of tests/explain_cases.py checked against itself."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib, explain_slot
from inverted_index_2_amd.engine import II2Error
from tests import explain_cases as ec

EDGE_IDS = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF]


def test_slot_matches_its_restatement():
    ids = EDGE_IDS + [int(x) for x in np.random.default_rng(11).integers(0, 1 << 32, 1000, dtype=np.uint64)]
    for log2_slots in (6, 7, 24, 25):
        for i in ids:
            got = explain_slot(i, log2_slots)
            assert got == ((i * 0x9E3779B1) & 0xFFFFFFFF) >> (32 - log2_slots) == ec.slot(i, log2_slots), (i, log2_slots)
            assert 0 <= got < (1 << log2_slots)


def test_slot_rejects_bad_arguments():
    lib = _lib.load()
    out = C.c_uint32(77)
    for log2_slots in (0, 32, 33, 0xFFFFFFFF):
        assert lib.ii2_explain_slot(5, log2_slots, C.byref(out)) == -1 and out.value == 77
        with pytest.raises(II2Error):
            explain_slot(5, log2_slots)
    assert lib.ii2_explain_slot(5, 6, None) == -1
    assert lib.ii2_explain_slot(5, 1, C.byref(out)) == 0 and out.value in (0, 1)
    assert lib.ii2_explain_slot(5, 31, C.byref(out)) == 0 and out.value == ec.slot(5, 31)


def test_prototypes_and_stats_struct():
    restype, args = _lib.PROTOTYPES["ii2_explain_ranges"]
    assert restype is C.c_int and len(args) == 11 and args[-1]._type_ is _lib.ExplainStats
    restype, args = _lib.PROTOTYPES["ii2_explain_slot"]
    assert restype is C.c_int and len(args) == 3
    assert C.sizeof(_lib.ExplainStats) == 56
    assert [f[0] for f in _lib.ExplainStats._fields_] == ["n_ids", "n_lists", "n_blocks", "n_decoded", "n_hits", "n_windows", "n_words", "log2_slots", "pad"]
    assert _lib.II2_EXPLAIN_MAX_IDS == 1 << 24


def test_table_log2():
    assert [ec.table_log2(n) for n in (0, 1, 32, 33, 64, 65, 257, 1 << 24)] == [6, 6, 6, 7, 7, 8, 10, 25]


CASES = ec.cases()


def test_case_names_are_distinct_and_cover_the_areas():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for n in ec.ROW_SIZES:
        for order in ec.ORDERS:
            assert f"rows_{n}_{order}" in names
    for n in ec.WORD_GROUPS:
        assert f"words_{n}_groups" in names
    # the table built with the library's hash is the same table
    for a, b in zip(CASES, ec.cases(explain_slot)):
        assert a.name == b.name and np.array_equal(a.ids, b.ids)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_is_consistent(case):
    for lists in case.segments:
        for l in lists:
            assert l.dtype == np.uint32 and np.all(np.diff(l.astype(np.int64)) > 0)
    for g in case.groups:
        for s, a, b in g:
            assert 0 <= a <= b <= len(case.segments[s])
    want = case.expect()
    assert want.shape == (case.ids.size, case.n_words) and want.dtype == np.uint64
    # every mask bit at or above n_groups is 0
    high = len(case.groups) & 63
    if high:
        assert not np.any(want[:, -1] >> np.uint64(high))
    # a repeated id: its first row may hold bits, every later row is zero
    seen = set()
    for i, x in enumerate(case.ids.tolist()):
        if x in seen:
            assert not want[i].any()
        seen.add(x)
    # bit g of row i against the definition, by plain loops
    sets = [set(np.concatenate(ls).tolist()) if ls else set() for ls in ([l for l in gl if l.size] for gl in case.group_lists())]
    first = {}
    for i, x in enumerate(case.ids.tolist()):
        first.setdefault(x, i)
    for i, x in enumerate(case.ids.tolist()):
        for g, members in enumerate(sets):
            bit = (int(want[i, g >> 6]) >> (g & 63)) & 1
            assert bit == int(x in members and first[x] == i), (i, g)
    if case.windows == 0:
        assert not want.any()


def test_the_hash_cases_do_collide():
    by = {c.name: c for c in CASES}
    chain = by["hash_chain_of_20"]
    assert ec.table_log2(chain.ids.size) == 6
    assert sum(ec.slot(x, 6) == 10 for x in chain.ids) == 20
    absent = by["hash_absent_after_full_chain"]
    a = absent.note["absent"]
    assert ec.slot(a, 6) == 10 and a not in absent.ids and any(a in l for l in absent.segments[0])
    assert all(ec.slot(x, 6) == 10 for x in absent.ids) and absent.ids.size == 20
    wrap = by["hash_chain_wraps"]
    assert ec.table_log2(wrap.ids.size) == 6 and [ec.slot(x, 6) for x in wrap.ids] == [62] * 6 + [0] * 2
    rep = by["repeated_ids"]
    _, counts = np.unique(rep.ids, return_counts=True)
    assert sorted(counts[counts > 1].tolist()) == [2, 2, 3] and rep.ids.size == 100
    both = by["words_65_groups"].expect()
    assert np.any((both[:, 0] >> np.uint64(63)) & (both[:, 1] & np.uint64(1)))      # a doc in groups 63 and 64 at once
