"""GPU: ii2_dict_build (csrc/dict_build.hip) - every case of tests/dict_build_cases.py through the kernels with host arrays and
with device arrays, sizes around every wave and tile boundary, input orders, the optional outputs, every error with nothing left
allocated, and the built dictionary downstream: ii2_dict_find, ii2_align_dicts and, on the device end to end, ii2_seg_build.
The reference is Python: sorted(set(terms)) on bytes and index() into it."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from inverted_index_2_amd.engine import DeviceArray, II2Error
from tests import dict_build_cases as cases
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

TILE = 4096      # pairs per workgroup of the sort (SB_TILE); the sizes of test_sizes_around_every_boundary bracket it
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * 16384 + 5]


def _live_bytes(ctx):
    live = C.c_uint64()
    ctx.lib.ii2_devmem_stats(C.byref(live), None)
    return live.value


def _plan_passes(ctx, terms):
    blob, off = cases.flat(terms)
    pos, lp = np.zeros(256, np.uint8), np.zeros(2, np.uint8)
    n, lo, hi = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert ctx.lib.ii2_dict_build_plan(blob.ctypes.data, off.ctypes.data, len(terms), pos.ctypes.data, lp.ctypes.data, C.byref(n), C.byref(lo),
                                       C.byref(hi)) == 0
    return n.value


def _check(ctx, terms, d, ids, st, expect=None):
    """the built dictionary, the ids and the stats against Python; frees the dictionary"""
    uniq, want_ids = cases.reference(terms)
    try:
        assert d.export() == uniq
        assert d.info() == (len(uniq), sum(len(t) for t in uniq))
        made = ctx.dictionary(uniq)                              # ii2_dict_create on the reference: the same arrays
        blob, off = d.export_flat()
        m_blob, m_off = made.export_flat()
        made.free()
        assert blob.tolist() == m_blob.tolist() and off.tolist() == m_off.tolist()
        if ids is not None:
            assert np.asarray(ids).tolist() == want_ids
        if st is not None:
            assert (st.n_terms, st.n_unique, st.n_bytes) == (len(terms), len(uniq), sum(len(t) for t in uniq))
            assert (st.min_len, st.max_len) == ((min(map(len, terms)), max(map(len, terms))) if terms else (0, 0))
            assert st.n_passes == _plan_passes(ctx, terms)
            for key in ("n_passes", "n_unique"):
                if expect and key in expect:
                    assert getattr(st, key) == expect[key]
    finally:
        d.free()


def _device_build(ctx, terms, want_ids=True):
    blob, off = cases.flat(terms)
    d_blob = DeviceArray(ctx, max(off[-1], 1), np.uint8).upload(blob[: int(off[-1])])      # no padding behind the last term
    d_off = DeviceArray(ctx, off.size, np.uint64).upload(off)
    d, ids, st = ctx.build_dictionary(d_blob, d_off, _lib.II2_DEVICE, want_ids)
    host_ids = ids.download(len(terms)) if ids is not None else None
    for a in (d_blob, d_off, ids):
        if a is not None:
            a.free()
    return d, host_ids, st


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_host_arrays(ctx, case):
    d, ids, st = ctx.build_dictionary(case.terms)
    _check(ctx, case.terms, d, ids, st, case.expect)


@pytest.mark.parametrize("case", cases.CASES, ids=lambda c: c.name)
def test_device_arrays(ctx, case):
    d, ids, st = _device_build(ctx, case.terms)
    _check(ctx, case.terms, d, ids, st, case.expect)


@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_every_boundary(ctx, n):
    """few distinct terms - the runs of equal terms cross wave and tile ends - and all distinct ones"""
    for terms in (cases.few_distinct(n, seed=n + 1), cases.BY_NAME["all_distinct"].terms[:n] if n <= 20000 else None):
        if terms is None:
            continue
        d, ids, st = ctx.build_dictionary(terms)
        _check(ctx, terms, d, ids, st)
    if n > 20000:
        terms = [b"%07d" % ((i * 7919) % n) for i in range(n)]          # distinct: 7919 is prime and n is not a multiple of it
        assert len(set(terms)) == n
        d, ids, st = _device_build(ctx, terms)
        _check(ctx, terms, d, ids, st)


def test_input_orders(ctx):
    base = cases.few_distinct(2 * TILE + 77, seed=8) + cases.BY_NAME["all_distinct"].terms[:1500]
    middle = base[:3000] + [b"one long run"] * (TILE + 300) + base[3000:]
    for terms in (sorted(base), sorted(base, reverse=True), middle):
        d, ids, st = ctx.build_dictionary(terms)
        _check(ctx, terms, d, ids, st)


def test_optional_outputs(ctx):
    terms = cases.BY_NAME["seams"].terms + cases.few_distinct(500)
    d, ids, st = ctx.build_dictionary(terms, want_ids=False)                 # term_id == NULL
    assert ids is None
    _check(ctx, terms, d, None, st)
    d, ids, st = _device_build(ctx, terms, want_ids=False)
    _check(ctx, terms, d, None, st)
    blob, off = cases.flat(terms)                                            # stats == NULL
    out_ids, h = np.zeros(len(terms), np.uint32), C.c_void_p()
    assert ctx.lib.ii2_dict_build(ctx.h, len(terms), blob.ctypes.data, off.ctypes.data, 0, C.byref(h), out_ids.ctypes.data, None) == 0
    from inverted_index_2_amd.engine import Dictionary
    _check(ctx, terms, Dictionary(ctx, h), out_ids, None)
    # no terms: the empty dictionary, all-zero stats, NULL arrays
    h, st = C.c_void_p(), _lib.DictBuildStats(n_terms=7, n_passes=7)
    assert ctx.lib.ii2_dict_build(ctx.h, 0, None, None, 1, C.byref(h), None, C.byref(st)) == 0 and h.value
    d = Dictionary(ctx, h)
    assert d.info() == (0, 0) and d.export() == [] and bytes(st) == bytes(40)
    first, end = d.find([b"a"])
    assert first.tolist() == [0] and end.tolist() == [0]
    d.free()


def test_errors_leave_nothing_behind(ctx):
    FILL = 0xABABABAB
    terms = [b"bb", b"a", b"ccc", b"a"]
    blob, off = cases.flat(terms)
    blob = np.concatenate([blob, np.zeros(300, np.uint8)])                   # (every offset below stays inside the buffer)
    ids = np.full(4, FILL, np.uint32)
    h = C.c_void_p(0)
    before = _live_bytes(ctx)

    def call(n=4, b=blob, o=off, where=0, out=h, t=ids):
        p = lambda a: a.ctypes.data if a is not None else None
        out_p = C.byref(out) if out is not None else None
        return ctx.lib.ii2_dict_build(ctx.h, n, p(b), p(o), where, out_p, p(t), None)

    def clean():
        return not h.value and (ids == FILL).all() and _live_bytes(ctx) == before

    descending, late = np.array([0, 2, 1, 6, 7], np.uint64), np.array([1, 2, 3, 6, 7], np.uint64)
    long_off = np.array([0, 2, 3, 260, 261], np.uint64)                      # a 257-byte term
    for kw, code in ((dict(o=descending), -1), (dict(o=late), -1), (dict(b=None), -1), (dict(o=None), -1), (dict(where=2), -1), (dict(out=None), -1),
                     (dict(o=long_off), -5), (dict(n=1 << 31), -5)):
        assert call(**kw) == code, kw
        assert clean(), kw
    # the same faults in arrays that live on the device: found there, in the first kernel
    d_blob = DeviceArray(ctx, blob.size, np.uint8).upload(blob)
    d_ids = DeviceArray(ctx, 4, np.uint32).upload(ids)
    before = _live_bytes(ctx)
    for o, code in ((descending, -1), (late, -1), (long_off, -5)):
        d_off = DeviceArray(ctx, 5, np.uint64).upload(o)
        with pytest.raises(II2Error) as e:
            ctx.build_dictionary(d_blob, d_off, _lib.II2_DEVICE)
        assert e.value.code == code
        rc = ctx.lib.ii2_dict_build(ctx.h, 4, d_blob.ptr, d_off.ptr, 1, C.byref(h), d_ids.ptr, None)
        assert rc == code and not h.value and (d_ids.download() == FILL).all()
        d_off.free()
        assert _live_bytes(ctx) == before
    d_blob.free()
    d_ids.free()
    assert call() == 0 and h.value and ids.tolist() == [1, 0, 2, 0]
    ctx.lib.ii2_dict_free(h)


def test_built_dictionary_answers_dict_find(ctx):
    terms = cases.BY_NAME["seams"].terms + cases.BY_NAME["zero_ties"].terms + cases.few_distinct(3000) + cases.BY_NAME["all_distinct"].terms[:3000]
    d, ids, _ = ctx.build_dictionary(terms)
    first, end = d.find(terms)
    assert first.tolist() == ids.tolist() and end.tolist() == (ids.astype(np.uint64) + 1).tolist()
    first, end = d.find([b"absent term", b"t0"], prefix=[0, 1])
    uniq = sorted(set(terms))
    assert int(end[0]) == int(first[0]) and [uniq[i] for i in range(int(first[1]), int(end[1]))] == [t for t in uniq if t.startswith(b"t0")]
    d.free()


def test_built_dictionaries_align_like_created_ones(ctx):
    a = cases.few_distinct(700, seed=1) + cases.BY_NAME["all_distinct"].terms[:900] + cases.BY_NAME["seams"].terms
    b = cases.few_distinct(300, seed=2)[::2] + cases.BY_NAME["all_distinct"].terms[450:1500] + cases.BY_NAME["zero_ties"].terms
    built = [ctx.build_dictionary(t)[0] for t in (a, b)]
    created = [ctx.dictionary(sorted(set(t))) for t in (a, b)]
    al_b, al_c = ctx.align_dicts(built), ctx.align_dicts(created)
    rep_b, src_b = al_b.export()
    terms_c, src_c = al_c.export()
    assert al_b.n_union == al_c.n_union == len(set(a) | set(b)) and src_b.tolist() == src_c.tolist()
    flat = sorted(set(a)) + sorted(set(b))
    assert [flat[int(g)] for g in rep_b] == terms_c == sorted(set(a) | set(b))
    for x in built + created + [al_b, al_c]:
        x.free()


def test_documents_to_segment_on_the_device(ctx):
    """terms of 300 docs x 8 -> ii2_dict_build(II2_DEVICE) -> ii2_seg_build(II2_DEVICE) on the ids as they are: the segment
    encode_lists makes of the Python-built lists"""
    rng = np.random.default_rng(77)
    vocab = cases.BY_NAME["all_distinct"].terms[:400]
    occ, vals = [], []
    for doc in range(300):
        for i in rng.choice(len(vocab), 8, replace=False):
            occ.append(vocab[int(i)])
            vals.append(doc * 3)
    blob, off = cases.flat(occ)
    d_blob, d_off = DeviceArray(ctx, int(off[-1]), np.uint8).upload(blob[: int(off[-1])]), DeviceArray(ctx, off.size, np.uint64).upload(off)
    d_vals = DeviceArray(ctx, len(vals), np.uint32).upload(np.array(vals, np.uint32))
    d, d_ids, st = ctx.build_dictionary(d_blob, d_off, _lib.II2_DEVICE)
    seg, bst = ctx.build_segment(d_ids, d_vals, st.n_unique, _lib.II2_DEVICE)
    uniq = sorted(set(occ))
    lists = {t: set() for t in uniq}
    for t, v in zip(occ, vals):
        lists[t].add(v)
    want = ctx.encode_lists([np.array(sorted(lists[t]), np.uint32) for t in uniq])
    assert d.export() == uniq and bst.n_postings == sum(len(v) for v in lists.values())
    for g, w in zip(seg.export(), want.export()):
        assert np.array_equal(g, w)
    for x in (d_blob, d_off, d_vals, d_ids, d, seg, want):
        x.free()
