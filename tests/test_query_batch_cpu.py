"""CPU: ii2_query_batch exists in every layer that can be looked at without a GPU - header, ctypes binding, the built library's
export table, the host mirror's use of it - and engine.pack_batch flattens a batch of queries into the entry point's arrays."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib, pack_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ii2.h")).read()


def test_query_batch_is_declared_bound_and_exported():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+ii2_query_batch\s*\(", code)
    assert re.search(r"II2_OP_AND\s*=\s*0\s*,\s*II2_OP_OR\s*=\s*1", code)
    assert "#define II2_ABI_VERSION 1" in code                        # additive: the ABI version stays
    res, args = _lib.PROTOTYPES["ii2_query_batch"]
    assert res is C.c_int and len(args) == 11
    assert (_lib.II2_OP_AND, _lib.II2_OP_OR) == (0, 1)
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    assert hasattr(C.CDLL(_lib.LIB_PATH), "ii2_query_batch")


def test_header_documents_the_option_the_limits_and_what_it_replaces():
    text = _header()
    assert "batch.small" in text
    assert "inverted_index.go:274-292" in text and "inverted_index.go:192" in text
    conventions = text[: text.index("#ifndef II2_H")]
    assert "ii2_query_batch" in conventions and "2^32" in conventions


def test_host_mirror_prefix_search_makes_one_batch_call():
    src = open(os.path.join(ROOT, "inverted_index_2_amd", "host", "host_index.cpp")).read()
    body = src[src.index("PrefixSearch(std::vector<Term> prefixes)"):src.index("std::vector<uint32_t> Intersect(")]
    assert "ii2_query_batch(" in body
    assert "internal.h" not in src


class _Seg:
    """stands in for a Segment: pack_batch passes segments through untouched"""

    def __init__(self, name):
        self.name = name


def test_pack_batch_zero_queries():
    op, qf, segs, first, end = pack_batch([])
    assert op.dtype == np.uint8 and op.size == 0
    assert qf.dtype == np.uint64 and qf.tolist() == [0]
    assert segs == [] and first.size == 0 and end.size == 0
    assert first.dtype == np.uint64 and end.dtype == np.uint64


def test_pack_batch_hand_written_batches():
    a, b, c = _Seg("a"), _Seg("b"), _Seg("c")
    queries = [
        ("and", [(a, 0, 1), (b, 3, 4)]),
        ("or", []),                                   # an OR without a range
        ("or", [(a, 0, 5), (b, 2, 9), (c, 1, 1)]),    # several segments, one empty range
        ("AND", [(a, 0, 1), (a, 0, 1)]),              # the same list twice
        ("or", [(a, 0, 1)]),                          # ... and once more in another query
    ]
    op, qf, segs, first, end = pack_batch(queries)
    assert op.tolist() == [_lib.II2_OP_AND, _lib.II2_OP_OR, _lib.II2_OP_OR, _lib.II2_OP_AND, _lib.II2_OP_OR] == [0, 1, 1, 0, 1]
    assert qf.tolist() == [0, 2, 2, 5, 7, 8]
    assert np.all(np.diff(qf.astype(np.int64)) >= 0) and qf[0] == 0 and qf[-1] == len(segs)
    assert [s.name for s in segs] == list("ababcaaa")
    assert first.tolist() == [0, 3, 0, 2, 1, 0, 0, 0]
    assert end.tolist() == [1, 4, 5, 9, 1, 1, 1, 1]
    assert segs[0] is a and segs[5] is a and segs[6] is a                       # passed through, not copied
    for q, (_, ranges) in enumerate(queries):                                     # query q owns ranges qf[q] .. qf[q + 1] - 1
        mine = list(zip(segs[int(qf[q]):int(qf[q + 1])], first[int(qf[q]):int(qf[q + 1])].tolist(), end[int(qf[q]):int(qf[q + 1])].tolist()))
        assert mine == [(s, x, y) for s, x, y in ranges]


def test_pack_batch_accepts_numpy_indices():
    a = _Seg("a")
    _, qf, _, first, end = pack_batch([("or", [(a, np.uint64(3), np.int32(7))])])
    assert qf.tolist() == [0, 1] and first.tolist() == [3] and end.tolist() == [7]


@pytest.mark.parametrize("bad", ["xor", "", "not", 2, None])
def test_pack_batch_rejects_an_unknown_op(bad):
    with pytest.raises(ValueError) as e:
        pack_batch([("or", []), (bad, [(_Seg("a"), 0, 1)])])
    assert "query 1" in str(e.value)


def test_pack_batch_rejects_negative_indices():
    with pytest.raises(ValueError):
        pack_batch([("or", [(_Seg("a"), -1, 2)])])
