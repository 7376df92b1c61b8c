"""CPU: ii2_query_batch_groups exists in every layer that can be looked at without a GPU - header, ctypes binding, the built
library's export table, the host mirror's use of it - engine.pack_group_batch flattens a batch of (groups, exclude) queries into
the entry point's arrays, and the random batches of the GPU test hold the mix of query classes that test relies on."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib, pack_andnot, pack_batch, pack_group_batch
from tests import group_batch_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ii2.h")).read()


def test_query_batch_groups_is_declared_bound_and_exported():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+ii2_query_batch_groups\s*\(", code)
    assert re.search(r"\bint\s+ii2_query_batch\s*\(", code)            # the flat batch stays
    assert "#define II2_ABI_VERSION 1" in code                        # additive: the ABI version stays
    res, args = _lib.PROTOTYPES["ii2_query_batch_groups"]
    assert res is C.c_int and len(args) == 12
    assert args[2] is _lib.u64p and args[3] is _lib.u64p and args[4] is _lib.u8p      # query_first, group_first, group_not
    assert len(_lib.PROTOTYPES["ii2_query_batch"][1]) == 11
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "ii2_query_batch_groups")
    lib.ii2_abi_version.restype = C.c_int
    assert lib.ii2_abi_version() == 1


def test_header_documents_the_option_the_limits_and_what_it_replaces():
    text = _header()
    assert "batch.groups" in text[text.index("int ii2_selftest"):]     # in the ii2_set_option comment
    start = text.index("MANY AND-of-ORs / NOT queries in one call")
    doc = text[start:text.index("int ii2_query_batch_groups(")]
    assert start > text.index("int ii2_query_batch(")                  # below its neighbour
    assert "Intersect / IntersectExcept" in doc and "inverted_index.go:192" in doc
    assert "ii2_andnot_ranges" in doc and "ii2_intersect_ranges" in doc and "bit-identical" in doc
    assert "II2_ECAPACITY" in doc and "II2_ERANGE" in doc and "II2_EINVAL" in doc and "query 17" in doc
    assert "batch.groups" in doc
    conventions = text[: text.index("#ifndef II2_H")]
    assert "ii2_query_batch_groups" in conventions
    mine = conventions[conventions.index("ii2_query_batch_groups"):]
    assert "2^20" in mine and "2^32" in mine and "8192" in mine and "128 blocks" in mine and "II2_MAX_LISTS" in mine


def test_option_and_kernel_are_known_to_the_library_source():
    csrc = os.path.join(ROOT, "inverted_index_2_amd", "csrc")
    assert '"batch.groups"' in open(os.path.join(csrc, "api.cpp")).read()
    assert "build/setop_groups_batch.o" in open(os.path.join(csrc, "Makefile")).read()
    kernel = open(os.path.join(csrc, "setop_groups_batch.hip")).read()
    assert "k_setop_groups_batch" in kernel and "ss_group_run_kept(" in kernel
    assert "ss_group_run_kept(" in open(os.path.join(csrc, "setop_groups.hip")).read()          # the run walk is shared, not copied
    assert "k_batch_pack" not in re.sub(r"//.*", "", kernel)                                     # the pack kernel is reused


def test_host_mirror_intersect_many_makes_one_batch_call():
    src = open(os.path.join(ROOT, "inverted_index_2_amd", "host", "host_index.cpp")).read()
    start = src.index("IntersectMany(const ")
    assert start > src.index("std::vector<uint32_t> IntersectExcept(")   # below IntersectExcept
    body = src[start:src.index("size_t ShardCount()")]
    assert body.count("ii2_query_batch_groups(") == 1
    assert "ii2_andnot_ranges(" not in body and "ii2_intersect_ranges(" not in body and "ii2_query_batch(" not in body
    assert body.count("ii2_copy_d2h(") == 1                              # one download
    assert "ii2h_intersect_batch" in src
    assert "internal.h" not in src
    from inverted_index_2_amd import host
    assert hasattr(host.InvertedIndex, "intersect_batch")


class _Seg:
    """stands in for a Segment: pack_group_batch passes segments through untouched"""

    def __init__(self, name):
        self.name = name


def test_pack_group_batch_zero_queries():
    qf, gf, gn, segs, first, end = pack_group_batch([])
    assert qf.dtype == np.uint64 and qf.tolist() == [0]
    assert gf.dtype == np.uint64 and gf.tolist() == [0]
    assert gn.dtype == np.uint8 and gn.size == 0
    assert segs == [] and first.size == 0 and end.size == 0
    assert first.dtype == np.uint64 and end.dtype == np.uint64


def test_pack_group_batch_hand_written_batch():
    a, b, c = _Seg("a"), _Seg("b"), _Seg("c")
    queries = [
        ([[(a, 0, 1), (b, 3, 4)], [(c, 2, 9)]], [[(a, 0, 1)]]),          # two required groups, one excluded: a list both
        ([], []),                                                        # a query with no groups
        ([[(a, 0, 5), (b, 2, 9), (c, 1, 1)]], []),                       # no exclusion; one empty range
        ([[(a, 0, 1)], []], [[(b, 0, 5), (c, 1, 1)], [(a, 0, 1)]]),      # a group without a range keeps its place; `a` again
        ([[(a, 0, 1)]], []),                                             # ... and once more in another query
    ]
    qf, gf, gn, segs, first, end = pack_group_batch(queries)
    assert qf.tolist() == [0, 3, 3, 4, 8, 9]
    assert gn.tolist() == [0, 0, 1, 0, 0, 0, 1, 1, 0]
    assert gf.tolist() == [0, 2, 3, 4, 7, 8, 8, 10, 11, 12]
    assert [s.name for s in segs] == list("abcaabcabcaa")
    assert first.tolist() == [0, 3, 2, 0, 0, 2, 1, 0, 0, 1, 0, 0]
    assert end.tolist() == [1, 4, 9, 1, 5, 9, 1, 1, 5, 1, 1, 1]
    assert qf[0] == 0 and gf[0] == 0 and qf[-1] == gn.size == gf.size - 1 and gf[-1] == len(segs)
    assert np.all(np.diff(qf.astype(np.int64)) >= 0) and np.all(np.diff(gf.astype(np.int64)) >= 0)
    assert segs[0] is a and segs[3] is a and segs[10] is a               # passed through, not copied
    for q, (groups, exclude) in enumerate(queries):                     # query q is pack_andnot's arrays, shifted to its place
        g0, g1 = int(qf[q]), int(qf[q + 1])
        pf, pn, ps, pa, pb = pack_andnot(groups, exclude)
        r0, r1 = int(gf[g0]), int(gf[g1])
        assert gn[g0:g1].tolist() == pn.tolist()
        assert (gf[g0:g1 + 1].astype(np.int64) - r0).tolist() == pf.tolist()
        assert segs[r0:r1] == ps and first[r0:r1].tolist() == pa.tolist() and end[r0:r1].tolist() == pb.tolist()
        assert sorted(gn[g0:g1].tolist()) == gn[g0:g1].tolist()          # required groups first


def test_pack_group_batch_accepts_numpy_indices():
    a = _Seg("a")
    qf, gf, gn, _, first, end = pack_group_batch([([[(a, np.uint64(3), np.int32(7))]], [[(a, np.int64(0), np.uint8(2))]])])
    assert qf.tolist() == [0, 2] and gf.tolist() == [0, 1, 2] and gn.tolist() == [0, 1]
    assert first.tolist() == [3, 0] and end.tolist() == [7, 2]


def test_pack_group_batch_rejects_negative_indices():
    good = ([[(_Seg("a"), 0, 1)]], [])
    for bad in (([[(_Seg("a"), -1, 2)]], []), ([[(_Seg("a"), 0, 1)]], [[(_Seg("b"), 0, -2)]])):
        with pytest.raises(ValueError) as e:
            pack_group_batch([good, good, bad])
        assert "query 2" in str(e.value)


@pytest.mark.parametrize("bad", ["not", "andnot"])
def test_pack_batch_goes_on_rejecting_not(bad):
    with pytest.raises(ValueError):
        pack_batch([(bad, [(_Seg("a"), 0, 1)])])


@pytest.mark.parametrize("universe,with_tomb,seed", cases.RANDOM_BATCHES)
def test_random_batches_hold_every_class_of_query(universe, with_tomb, seed):
    pool, queries, removed, wants = cases.random_batch(universe, with_tomb, seed)
    n, nonempty, removed_some = cases.check_mix(pool, queries, wants, removed)
    print("classes", n, "non-empty", nonempty, "an exclusion removed something in", removed_some)
    assert len(queries) == cases.N_QUERIES
    assert all(1 <= len(g) <= 5 and len(x) <= 3 for g, x in queries if g)
    count = lambda grp: sum(b - a for _, a, b in grp)                    # noqa: E731
    assert all(1 <= count(grp) <= 20 for g, _ in queries for grp in g)
    assert all(1 <= count(grp) <= 24 for _, x in queries for grp in x)    # (a range both required and excluded adds up to four)
    if universe > 1_000_000:
        assert any(w.size and w[0] == 0 for w in wants) or removed is not None


def test_capacity_table_holds_both_outcomes_with_and_without_exclusions():
    lists, queries = cases.CAPACITY_LISTS, cases.CAPACITY_QUERIES
    assert [len(ls) for ls in lists] == [33, 33, 2, 80, 1]
    assert all(l.size == 256 for l in lists[0]) and all(l.size == 64 for l in lists[1]) and all(l.size == 1 for l in lists[2])
    assert lists[4][0].tolist() == [1_000_000] and all(int(l[-1]) < 1_000_000 for ls in lists[:4] for l in ls)
    klass = [cases.query_class(lists, g, x) for g, x in queries]
    assert klass == cases.CAPACITY_CLASSES and len(klass) == 18
    with_x = [k for k, (_, x) in zip(klass, queries) if x]              # what the single call's one-launch form is asked about
    assert sum(k in ("tiny", "small") for k in with_x) >= 4 and with_x.count("large") >= 4
    # the far list: 64 lists count either way; excluded it is not one of them, required it empties the query
    counted = lambda g, x: sum(l.size > 0 for grp in g + x for l in cases.lists_of(lists, grp))      # noqa: E731
    for (g, x), k in zip(queries[16:], ("small", "empty")):
        assert counted(g, x) == 65 and any((4, 0, 1) in grp for grp in g + x)
        assert cases.query_class(lists, g, x) == k
    assert klass[10] == "small" and klass[11] == "large"                # ... and a 65th list that does count makes it large
