"""GPU: the arrays the library derives when a segment is made (ii2_seg_export_meta / Segment.meta()) against plain numpy over the
lists, bit for bit, for every way of making a segment and every shape of tests/segment_kinds.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import segment_kinds as sk
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(kind, shape):
    return sk.reference(sk.plan(kind, shape))


@pytest.mark.parametrize("kind,shape", sk.CASES)
def test_derived_arrays_equal_the_reference(ctx, kind, shape):
    p, r = sk.plan(kind, shape), _reference(kind, shape)
    seg, keep = sk.make(ctx, p)
    try:
        m = seg.meta()
        assert (seg.info.n_lists, seg.info.n_blocks, seg.info.n_bytes) == (r.n_lists, r.n_blocks, r.n_bytes)
        for name in ("cnt", "last_doc", "blk_list"):
            got, want = m[name], getattr(r, name)
            assert got.dtype == np.uint32 and got.shape == want.shape, name
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (name, bad[:8], got[bad[:8]], want[bad[:8]])
        assert m["blk_list"][r.n_blocks] == sk.NONE                   # the entry past the last block: every maker writes it
        # the span mirror: kept by every segment of up to 65536 lists that is finished on the host; the aligned views are adopted
        # as the device built them and the big segment fetches spans on demand
        assert m["spans_mirrored"] == p.mirrored and m["is_view"] == p.is_view
        if p.mirrored:
            bad = np.flatnonzero((m["spans"] != r.spans).any(axis=1))
            assert bad.size == 0, (bad[:8], m["spans"][bad[:8]], r.spans[bad[:8]])
        else:
            assert m["spans"] is None
        if p.aligned:
            # documented as an upper bound (include/ii2.h): what it IS is the store's total - the aligned view never counts its own
            assert m["n_postings"] == r.store_postings and m["n_postings"] >= r.sum_cnt
        else:
            assert m["n_postings"] == r.sum_cnt                        # exact: whole segments and the views of ii2_seg_select
        assert seg.info.n_postings == m["n_postings"]
        if kind == "select":
            assert (m["merge_blocks"], m["merge_bytes"]) == (r.win_blocks, r.win_bytes) and r.win_blocks < r.n_blocks
        else:
            assert (m["merge_blocks"], m["merge_bytes"]) == (r.n_blocks, r.n_bytes)
        if not p.is_view:                                              # and the DV1 bytes are still the oracle's
            po, flat = sk.csr(p.slots)
            oblk, oskip, opayload = orc.dv1_encode(po, flat)
            blk, skip, payload = seg.export()
            assert np.array_equal(blk, oblk) and np.array_equal(skip["first_doc"][:-1], oskip["first_doc"][:-1])
            assert np.array_equal(skip["byte_off"], oskip["byte_off"]) and np.array_equal(payload, opayload)
            gpo, gv = seg.decode()
            assert np.array_equal(gpo, po) and np.array_equal(gv, flat)
    finally:
        seg.free()
        for s in keep:
            s.free()


def test_export_meta_checks_its_arguments_and_takes_no_path(ctx):
    seg = ctx.encode_lists([np.arange(5, 700, 2, dtype=np.uint32), [], [9]])
    f = ctx.lib.ii2_seg_export_meta
    assert f(None, seg.h, None, None, None, None, None) == -1          # II2_EINVAL
    assert f(ctx.h, None, None, None, None, None, None) == -1
    with path_delta(ctx) as d:
        assert f(ctx.h, seg.h, None, None, None, None, None) == 0      # every output may be NULL
        cnt = np.full(3, 77, np.uint32)
        assert f(ctx.h, seg.h, C.c_void_p(cnt.ctypes.data), None, None, None, None) == 0
        m = seg.meta()
    assert d == {} and cnt.tolist() == [348, 0, 1] and m["cnt"].tolist() == [348, 0, 1]
    assert m["last_doc"].tolist() == [699, 0, 9] and m["blk_list"].tolist() == [0, 0, 2, sk.NONE]
    assert m["spans"].tolist() == [[5, 517, 699], [0, 0, 0], [9, 9, 9]]
    seg.free()
