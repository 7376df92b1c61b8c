"""GPU: the two-list AND of two lists that both have a dense form, ANDed word by word (csrc/intersect_words.hip k_and2_words;
options intersect.and2_words: 0 never, 1 by the rule of csrc/setop.cpp and2_words_pick, 2 always; intersect.and2_words_min).
Every case of tests/dense_form_cases.py and of tests/and2_words_cases.py runs forced (and2_words = 2): the ids equal numpy and the
run with and2_words = 0, both lists have their form, and the rows of cycle counters are the word kernel's grid for the pair's
window.  Everything is bit-exact, with FILL behind the result."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd.engine import II2Error
from tests import and2_words_cases as wc
from tests import dense_form_cases as dc
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu
FILL = 0xDEADBEEF
ECAPACITY = -4
FUSED = ({"and.and2_fused": 1}, {"and.and2_fused": 1, "and.and2_split": 1})     # (a look-back wait that ran out repeats the call)
DEFAULTS = (("intersect.and2_words", 1), ("intersect.and2_words_min", 0), ("intersect.dense_form", 1), ("intersect.and2_spin", 0), ("debug.stamps", 0))


@pytest.fixture
def words_option(ctx):
    ctx.set_option("intersect.and2_words", 2)
    yield lambda v: ctx.set_option("intersect.and2_words", v)
    for name, v in DEFAULTS:
        ctx.set_option(name, v)


def _run(c, ls, want, tomb=None, out=None):
    own = out is None
    out = c.empty(want.size + 64) if own else out
    out.upload(np.full(out.count, FILL, np.uint32))
    try:
        with path_delta(c) as took:
            _, n = c.intersect(ls, tomb=tomb, out=out)
        got = out.download()
    finally:
        if own:
            out.free()
    assert n == want.size and np.array_equal(got[:n], want)
    assert np.all(got[n:] == FILL)                                   # nothing written past the result
    return took


def _stamp_rows(c, ls, tomb=None):
    """workgroups of the call's kernel, by the rows of cycle counters it fills (debug.stamps; cleared per call)"""
    c.set_option("debug.stamps", 1)
    try:
        out, _ = c.intersect(ls, tomb=tomb)
        out.free()
        buf = (C.c_uint64 * (2048 * 8))()
        c._ck(c.lib.ii2_debug_read(c.h, buf, 2048 * 8))
    finally:
        c.set_option("debug.stamps", 0)
    arr = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 8)
    return int(np.count_nonzero(arr.sum(axis=1)))


def _old_rows(B):
    return (dc.blocks(B) + dc.WG_BLOCKS - 1) // dc.WG_BLOCKS        # the present instance at one tile a wave


def _form_is(seg, i, l):
    f = seg.dense_form(i)
    assert f is not None
    assert (f["origin"], f["n_words"]) == (dc.form_origin(l), dc.form_bytes(l) // 4)
    assert np.array_equal(f["words"], dc.form_words(l))
    return f


ALL = list(dc.CASES) + list(wc.CASES)


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_case_by_words_and_by_the_present_kernel(ctx, words_option, case):
    x, y, removed = case.data()
    want = wc.reference(x, y, removed)
    seg = ctx.encode_lists([x, y])
    tomb = ctx.tombstones(removed) if removed is not None else None
    ls = [(seg, 0), (seg, 1)]
    try:
        for _ in range(2):                                           # the query that makes the forms, then one that finds them
            assert _run(ctx, ls, want, tomb) in FUSED
            _form_is(seg, 0, x)
            _form_is(seg, 1, y)
        assert _stamp_rows(ctx, ls, tomb) == wc.workgroups(x, y)
        words_option(0)                                              # forms that exist are not used either
        assert _run(ctx, ls, want, tomb) in FUSED
        assert _stamp_rows(ctx, ls, tomb) in (_old_rows(dc.roles(x, y)[0]), (_old_rows(dc.roles(x, y)[0]) + 1) // 2)
    finally:
        seg.free()
        if tomb is not None:
            tomb.free()


@pytest.fixture(scope="module")
def pair():
    x, y, _ = dc.BY_NAME["uniform"].data()
    return x, y, dc.reference(dc.BY_NAME["uniform"])


def test_capacity_one_short(ctx, words_option, pair):
    B, A, want = pair
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    out = ctx.empty(want.size + 64)
    try:
        for _ in range(2):
            out.upload(np.full(out.count, FILL, np.uint32))
            with pytest.raises(II2Error) as e:
                ctx.intersect(ls, out=out, cap=want.size - 1)
            assert e.value.code == ECAPACITY
            assert np.all(out.download()[want.size - 1:] == FILL)    # nothing at or beyond the capacity
        _form_is(seg, 0, B)
        _, n = ctx.intersect(ls, out=out, cap=want.size)             # exactly enough
        assert n == want.size and np.array_equal(out.download(n), want)
        assert _stamp_rows(ctx, ls) == wc.workgroups(B, A)
    finally:
        out.free()
        seg.free()


@pytest.mark.parametrize("spin", [-1, -2], ids=["early", "late"])
def test_give_up(ctx, words_option, pair, spin):
    """The bounded waits of the look-back run out on purpose: the call notices, repeats itself through the two-kernel form - which
    reads the lists' blocks, forms or not - and returns the right ids; the counter of repeated calls goes up by one."""
    B, A, want = pair
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    try:
        assert _run(ctx, ls, want) in FUSED
        _form_is(seg, 0, B)
        ctx.set_option("intersect.and2_spin", spin)
        before = ctx.counters()[1]
        took = _run(ctx, ls, want)
        assert ctx.counters()[1] - before == 1
        assert took == {"and.and2_fused": 1, "and.and2_split": 1}
        ctx.set_option("intersect.and2_spin", 0)
        assert _run(ctx, ls, want) == {"and.and2_fused": 1}
        assert _stamp_rows(ctx, ls) == wc.workgroups(B, A)
    finally:
        ctx.set_option("intersect.and2_spin", 0)
        seg.free()


def test_the_rule(ctx, words_option, pair):
    B, A, want = pair
    words_option(1)
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    try:
        assert _run(ctx, ls, want) in FUSED                          # default minimum: the present instance, no form for B
        assert _stamp_rows(ctx, ls) == _old_rows(B) == 17
        _form_is(seg, 1, A)
        assert seg.dense_form(0) is None
        ctx.set_option("intersect.dense_form", 0)                    # (i): no forms, neither instance that reads one
        ctx.set_option("intersect.and2_words_min", 1024)
        assert _run(ctx, ls, want) in FUSED
        assert _stamp_rows(ctx, ls) == 17 and seg.dense_form(0) is None
        ctx.set_option("intersect.dense_form", 1)
        ctx.set_option("intersect.and2_words_min", dc.blocks(B) + 1) # (iii): one block short
        assert _stamp_rows(ctx, ls) == 17 and seg.dense_form(0) is None
        ctx.set_option("intersect.and2_words_min", dc.blocks(B))
        assert _run(ctx, ls, want) in FUSED
        assert _stamp_rows(ctx, ls) == wc.workgroups(B, A) == 13
        _form_is(seg, 0, B)
    finally:
        seg.free()


@pytest.mark.parametrize("dense_form", [1, 2])
def test_the_rule_asks_criterion_b_of_both_lists(ctx, words_option, dense_form):
    x, y, _ = dc.BY_NAME["criterion"].data()
    want = dc.reference(dc.BY_NAME["criterion"])
    B, A = dc.roles(x, y)
    assert B is x and dc.criterion_b(B) and not dc.criterion_b(A)
    words_option(1)
    ctx.set_option("intersect.dense_form", dense_form)
    seg = ctx.encode_lists([x, y])
    ls = [(seg, 0), (seg, 1)]
    try:
        for minimum in (0, 1, 1024):
            ctx.set_option("intersect.and2_words_min", minimum)
            assert _run(ctx, ls, want) in FUSED
            assert _stamp_rows(ctx, ls) == _old_rows(B)
            assert seg.dense_form(0) is None and (seg.dense_form(1) is None) == (dense_form == 1)
    finally:
        seg.free()


def test_views_share_both_forms(ctx, words_option, pair):
    B, A, want = pair
    rng = np.random.default_rng(9)
    s0, s1 = dc.bern(rng, 0.001, 0, 800_000), dc.bern(rng, 0.002, 0, 800_000)
    seg = ctx.encode_lists([s0, B, A, s1])
    view = ctx.select(seg, [1, 2])
    try:
        assert _run(ctx, [(view, 0), (view, 1)], want) in FUSED
        for l, iv, ip in ((B, 0, 1), (A, 1, 2)):                     # through the view and through the parent: the same entry
            _form_is(view, iv, l)
            _form_is(seg, ip, l)
        assert seg.dense_form(0) is None and seg.dense_form(3) is None
        assert _run(ctx, [(seg, 2), (seg, 1)], want) in FUSED        # the parent's query finds the view's forms
        assert seg.dense_form_bytes() == dc.form_bytes(A) + dc.form_bytes(B) + 32      # exactly two forms
    finally:
        view.free()
        seg.free()


def test_the_forms_memory_comes_back_with_the_segment(ctx, words_option, pair):
    B, A, want = pair

    def live():
        v = C.c_uint64()
        ctx.lib.ii2_devmem_stats(C.byref(v), None)
        return v.value
    out = ctx.empty(want.size + 64)
    for _ in range(2):                                               # (the first turn also grows the context's own buffers)
        before = live()
        seg = ctx.encode_lists([B, A])
        with_seg = live()
        _run(ctx, [(seg, 0), (seg, 1)], want, out=out)
        _form_is(seg, 0, B)
        _form_is(seg, 1, A)
        assert live() >= with_seg + dc.form_bytes(A) + dc.form_bytes(B)     # both forms are counted ...
        seg.free()
        assert live() == before                                      # ... and leave with the segment
    out.free()
