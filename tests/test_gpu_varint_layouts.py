"""GPU: every DV1 varint decoder on byte layouts aimed at its seams (tests/varint_cases.py): varints of every width across a
lane's dword, a 16-byte row-lane piece and the 256-byte chunk boundaries, lanes of four continuation bytes, blocks that end
inside a dword, payloads that start at every address residue mod 16.

  the codec        the matrix imported from the oracle's bytes and decoded; encoded on the device (ii2_seg_encode, and the
                   one-pass and two-pass encoders behind a merge: encode.stream 1 / 0) byte for byte like the oracle
  the consumers    VARINT_CASES: the exact Context.paths() delta and the numpy result, lists in one segment and over two
  ii2_count_ranges against a plain numpy count
  the merges       ii2_merge_small, and ii2_merge_segments / _to_seg with the plan and events of tests/merge_cases.py pinned
Everything is compared bit for bit; tests/test_varint_cases_cpu.py proves from the bytes which cells each case carries."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import path_cases as pc
from tests import varint_cases as vc
from tests.gpu_util import ctx, run_path_case  # noqa: F401
from tests.test_gpu_merge_cases import test_plan_events_and_result as run_merge_case

pytestmark = pytest.mark.gpu


# ---- the codec -------------------------------------------------------------------------------------------------------------
def _matrix():
    lists, _ = vc.matrix_segment()
    off, vals = vc.csr(lists)
    return off, vals, orc.dv1_encode(off, vals)


def _same_segment(seg, off, vals, oracle_bytes):
    oblk, oskip, opayload = oracle_bytes
    info = seg.info
    assert (info.n_lists, info.n_postings, info.n_blocks, info.n_bytes) == (off.size - 1, vals.size, oskip.size - 1, opayload.size)
    blk, skip, payload = seg.export()
    assert np.array_equal(blk, oblk)
    assert np.array_equal(skip["first_doc"][:-1], oskip["first_doc"][:-1]) and np.array_equal(skip["byte_off"], oskip["byte_off"])
    assert np.array_equal(payload, opayload)
    po, ids = seg.decode()
    assert np.array_equal(po, off) and np.array_equal(ids, vals)


def test_codec_decodes_the_matrix_from_oracle_bytes(ctx):
    off, vals, (oblk, oskip, opayload) = _matrix()
    seg = ctx.import_dv1(vals.size, oblk, oskip, opayload)
    _same_segment(seg, off, vals, (oblk, oskip, opayload))
    seg.free()


def test_codec_encodes_the_matrix_like_the_oracle(ctx):
    off, vals, oracle_bytes = _matrix()
    seg = ctx.encode(off, vals)
    _same_segment(seg, off, vals, oracle_bytes)
    seg.free()


@pytest.mark.parametrize("stream", [1, 0])
def test_merge_encoders_write_the_matrix_like_the_oracle(ctx, stream):
    """The encoders behind a merge (encode.stream 1: one pass with look-back, 0: two passes): a merge of the matrix segment
    alone decodes every block and writes the same bytes again."""
    off, vals, oracle_bytes = _matrix()
    seg = ctx.encode(off, vals)
    try:
        ctx.set_option("encode.stream", stream)
        again, st = ctx.merge_to_segment([seg])
        assert st.n_out == vals.size
        _same_segment(again, off, vals, oracle_bytes)
        again.free()
    finally:
        ctx.set_option("encode.stream", 1)
        seg.free()


# ---- every decoding consumer, its path asserted -------------------------------------------------------------------------------
CASE_LAYOUTS = [pytest.param(case, layout, id=f"{case.name}-{layout}") for case in vc.VARINT_CASES for layout in case.layouts()]


@pytest.mark.parametrize("case,layout", CASE_LAYOUTS)
def test_path_and_result(ctx, case, layout):
    run_path_case(ctx, case, layout, pc.DEFAULTS)


# ---- ii2_count_ranges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["one", "two"])
def test_count_ranges(ctx, layout):
    lists, ids = vc.count_lists()
    lay = pc.Layout(layout, lists)
    segs = [ctx.encode(*lay.flat(s)) for s in range(len(lay.segments))]
    named = [l for seg in lay.segments for l in seg]                                 # range order: segment by segment
    ranges = [(segs[s], 0, len(lay.segments[s])) for s in range(len(segs))]
    removed = np.union1d(ids[::3], np.concatenate(lists)[5::7]).astype(np.uint32)
    dset = ctx.empty(ids.size).upload(ids)
    tombs = ctx.tombstones(removed)
    try:
        for rem, tomb in ((np.empty(0, np.uint32), None), (removed, tombs)):
            want = np.array([np.count_nonzero(np.isin(l, ids) & ~np.isin(l, rem)) for l in named], np.uint64)
            got, st = ctx.count_ranges(ranges, dset, ids.size, tomb=tomb)
            assert np.array_equal(got, want) and st.n_hits == int(want.sum()) and st.n_lists == len(named)
            every, st = ctx.count_ranges(ranges, None, tomb=tomb)                     # every doc: the lists' own sizes
            assert np.array_equal(every, [np.count_nonzero(~np.isin(l, rem)) for l in named])
        assert 0 < want.sum() < sum(l.size for l in named)
    finally:
        for s in segs:
            s.free()
        tombs.free()
        dset.free()


# ---- the merges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vc.MERGE_CASES, ids=lambda c: c.name)
def test_merge_plan_events_and_result(ctx, case):
    run_merge_case(ctx, case)


@pytest.mark.parametrize("k", [2, 5])
def test_merge_small(ctx, k):
    terms = vc.merge_small_terms(k)
    names = [b"term%02d" % t for t in range(len(terms))]
    dicts = [[names[t] for t, lists in enumerate(terms) if s < len(lists)] for s in range(k)]
    segs = [ctx.encode_lists([lists[s] for lists in terms if s < len(lists)]) for s in range(k)]
    everything = np.unique(np.concatenate([l for lists in terms for l in lists]))
    made = []
    try:
        for removed in (np.empty(0, np.uint32), everything[2::5]):
            want = [np.setdiff1d(np.unique(np.concatenate(lists).astype(np.uint64)), removed.astype(np.uint64)) for lists in terms]
            seg, kept, st = ctx.merge_small(segs, dicts, removed)
            made.append(seg)
            assert kept == names and st.n_out == sum(w.size for w in want) and st.n_in == sum(l.size for lists in terms for l in lists)
            w_off = np.concatenate([[0], np.cumsum([w.size for w in want])]).astype(np.uint64)
            w_vals = np.concatenate(want).astype(np.uint32)
            po, v = seg.decode()
            assert np.array_equal(po, w_off) and np.array_equal(v, w_vals)
            oblk, oskip, opayload = orc.dv1_encode(w_off, w_vals)                      # what it wrote: the oracle's bytes
            blk, skip, payload = seg.export()
            assert np.array_equal(blk, oblk) and np.array_equal(skip["byte_off"], oskip["byte_off"]) and np.array_equal(payload, opayload)
    finally:
        for s in segs + [m for m in made if m is not None]:
            s.free()
