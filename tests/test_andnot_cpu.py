"""CPU: ii2_andnot_ranges exists in every layer that can be looked at without a GPU - header, ctypes binding, the built library's
export table, the host mirror's use of it - and engine.pack_andnot flattens required and excluded groups into the entry point's
arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib, pack_andnot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ii2.h")).read()


def test_andnot_ranges_is_declared_bound_and_exported():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+ii2_andnot_ranges\s*\(", code)
    assert "#define II2_ABI_VERSION 1" in code                        # additive: the ABI version stays
    res, args = _lib.PROTOTYPES["ii2_andnot_ranges"]
    assert res is C.c_int and len(args) == 11
    assert args[3] is _lib.u8p                                         # group_not: bytes
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(C.CDLL(_lib.LIB_PATH), "ii2_andnot_ranges")


def test_header_documents_the_option_the_error_and_the_capacity_rule():
    text = _header()
    assert "andnot.small" in text[text.index("int ii2_selftest"):]     # in the ii2_set_option comment
    doc = text[text.index("AND of ORs over list ranges MINUS"):text.index("int ii2_andnot_ranges(")]
    assert "no required group: II2_EINVAL" in doc
    assert "All-or-nothing" in doc and "nothing is written" in doc and "*count holds the size needed" in doc
    assert "group_not == NULL" in doc and "ii2_intersect_ranges" in doc
    conventions = text[: text.index("#ifndef II2_H")]
    assert "ii2_andnot_ranges" in conventions and "8192" in conventions and "128 blocks" in conventions


def test_host_mirror_intersect_except_makes_one_andnot_call():
    src = open(os.path.join(ROOT, "inverted_index_2_amd", "host", "host_index.cpp")).read()
    start = src.index("std::vector<uint32_t> IntersectExcept(")
    assert start > src.index("std::vector<uint32_t> Intersect(")          # after Intersect
    body = src[start:src.index("size_t ShardCount()")]
    assert body.count("ii2_andnot_ranges(") == 1
    assert "ii2_union_ranges(" not in body and "ii2_intersect_ranges(" not in body
    assert "ii2h_intersect_except" in src
    assert "internal.h" not in src
    from inverted_index_2_amd import host
    assert hasattr(host.InvertedIndex, "intersect_except")


def test_option_is_known_to_the_library_source():
    api = open(os.path.join(ROOT, "inverted_index_2_amd", "csrc", "api.cpp")).read()
    assert '"andnot.small"' in api
    mk = open(os.path.join(ROOT, "inverted_index_2_amd", "csrc", "Makefile")).read()
    assert "build/setop_groups.o" in mk


class _Seg:
    """stands in for a Segment: pack_andnot passes segments through untouched"""

    def __init__(self, name):
        self.name = name


def test_pack_andnot_no_groups():
    gf, gn, segs, first, end = pack_andnot([], [])
    assert gf.dtype == np.uint64 and gf.tolist() == [0]
    assert gn.dtype == np.uint8 and gn.size == 0
    assert segs == [] and first.size == 0 and end.size == 0
    assert first.dtype == np.uint64 and end.dtype == np.uint64


def test_pack_andnot_required_groups_first_then_the_excluded_ones():
    a, b, c = _Seg("a"), _Seg("b"), _Seg("c")
    groups = [[(a, 0, 1), (b, 3, 4)], [], [(c, 2, 9)]]                 # a group without a range keeps its place
    exclude = [[(a, 0, 1)], [(b, 0, 5), (c, 1, 1)]]                    # a list both required and excluded
    gf, gn, segs, first, end = pack_andnot(groups, exclude)
    assert gn.tolist() == [0, 0, 0, 1, 1]
    assert gf.tolist() == [0, 2, 2, 3, 4, 6]
    assert np.all(np.diff(gf.astype(np.int64)) >= 0) and gf[-1] == len(segs)
    assert [s.name for s in segs] == list("abcabc")
    assert first.tolist() == [0, 3, 2, 0, 0, 1] and end.tolist() == [1, 4, 9, 1, 5, 1]
    assert segs[0] is a and segs[3] is a                                # passed through, not copied
    for g, ranges in enumerate(groups + exclude):                      # group g owns ranges gf[g] .. gf[g + 1] - 1
        lo, hi = int(gf[g]), int(gf[g + 1])
        assert list(zip(segs[lo:hi], first[lo:hi].tolist(), end[lo:hi].tolist())) == [(s, x, y) for s, x, y in ranges]


def test_pack_andnot_without_exclusions_and_with_numpy_indices():
    a = _Seg("a")
    gf, gn, _, first, end = pack_andnot([[(a, np.uint64(3), np.int32(7))]], [])
    assert gn.tolist() == [0] and gf.tolist() == [0, 1] and first.tolist() == [3] and end.tolist() == [7]
    gf, gn, _, _, _ = pack_andnot([], [[(a, 0, 1)]])                   # (the library rejects it: no required group)
    assert gn.tolist() == [1] and gf.tolist() == [0, 1]


def test_pack_andnot_rejects_negative_indices():
    with pytest.raises(ValueError):
        pack_andnot([[(_Seg("a"), 0, 1)]], [[(_Seg("b"), -1, 2)]])
