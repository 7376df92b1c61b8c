"""GPU: the dense form of a two-list AND's longer list (a bitmap over its docs, made by the first query that would mark the list
and cached with the segment's store) - csrc/setop.cpp dense_form_get, csrc/intersect_and2.hip k_dense_form_build and the instance
of k_and2_fused that reads the form instead of marking.  Every case of tests/dense_form_cases.py runs with option
intersect.dense_form = 0 (no form: the list is marked as before) and 1: the ids are equal to each other and to numpy, the form
is there or not as criterion (b) says, and its words equal the packed-bits reference.  Everything is bit-exact."""
import ctypes as C
import threading

import numpy as np
import pytest

from inverted_index_2_amd import Context
from inverted_index_2_amd.engine import II2Error
from tests import dense_form_cases as dc
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu
FILL = 0xDEADBEEF
ECAPACITY = -4
FUSED = ({"and.and2_fused": 1}, {"and.and2_fused": 1, "and.and2_split": 1})     # (a look-back wait that ran out repeats the call)


def _run(c, ls, want, tomb=None, out=None):
    out = out if out is not None else c.empty(want.size + 64)
    out.upload(np.full(out.count, FILL, np.uint32))
    with path_delta(c) as took:
        _, n = c.intersect(ls, tomb=tomb, out=out)
    got = out.download()
    assert n == want.size and np.array_equal(got[:n], want)
    assert np.all(got[n:] == FILL)                                  # nothing written past the result
    return took


def _form_is(seg, i, A, c=None):
    f = seg.dense_form(i, c)
    assert f is not None
    assert (f["origin"], f["n_words"]) == (dc.form_origin(A), dc.form_bytes(A) // 4)
    assert np.array_equal(f["words"], dc.form_words(A))
    return f


@pytest.fixture
def form_option(ctx):
    yield lambda v: ctx.set_option("intersect.dense_form", v)
    ctx.set_option("intersect.dense_form", 1)
    ctx.set_option("intersect.and2_spin", 0)


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_case_with_and_without_the_form(ctx, form_option, case):
    x, y, removed = case.data()
    want = dc.reference(case)
    _, A = dc.roles(x, y)
    ia = 0 if A is x else 1
    seg = ctx.encode_lists([x, y])
    tomb = ctx.tombstones(removed) if removed is not None else None
    ls = [(seg, 0), (seg, 1)]
    try:
        form_option(0)
        assert _run(ctx, ls, want, tomb) in FUSED
        assert seg.dense_form(0) is None and seg.dense_form(1) is None and seg.dense_form_bytes() == 0
        form_option(1)
        for _ in range(2):                                          # the query that makes the form, then one that finds it
            assert _run(ctx, ls, want, tomb) in FUSED
            assert seg.dense_form(1 - ia) is None                   # never the shorter list
            if case.form:
                f = _form_is(seg, ia, A)
                assert f["store_bytes"] == dc.form_bytes(A) + 16
            else:
                assert seg.dense_form(ia) is None and seg.dense_form_bytes() == 0
        if not case.form:                                           # option 2: whatever criterion (b) says
            form_option(2)
            assert _run(ctx, ls, want, tomb) in FUSED
            _form_is(seg, ia, A)
            form_option(0)                                          # a form that exists is not used either
            assert _run(ctx, ls, want, tomb) in FUSED
    finally:
        seg.free()
        if tomb is not None:
            tomb.free()


@pytest.fixture(scope="module")
def pair():
    x, y, _ = dc.BY_NAME["uniform"].data()
    return x, y, dc.reference(dc.BY_NAME["uniform"])


def test_views_share_the_form_of_their_store(ctx, form_option, pair):
    B, A, want = pair
    rng = np.random.default_rng(9)
    s0, s1 = dc.bern(rng, 0.001, 0, 800_000), dc.bern(rng, 0.002, 0, 800_000)
    seg = ctx.encode_lists([s0, B, A, s1])
    view = ctx.select(seg, [1, 2])
    try:
        assert _run(ctx, [(view, 0), (view, 1)], want) in FUSED
        fv = _form_is(view, 1, A)                                   # through the view ...
        fp = _form_is(seg, 2, A)                                    # ... and through the parent: the same entry
        assert fv["store_bytes"] == fp["store_bytes"] == dc.form_bytes(A) + 16
        assert all(seg.dense_form(i) is None for i in (0, 1, 3)) and view.dense_form(0) is None
        assert _run(ctx, [(seg, 2), (seg, 1)], want) in FUSED       # the parent's query finds the view's form
        assert seg.dense_form_bytes() == dc.form_bytes(A) + 16      # exactly one form
    finally:
        view.free()
        seg.free()


def test_concatenated_segment(ctx, form_option, pair):
    B, A, want = pair
    sb, sa = ctx.encode_lists([B]), ctx.encode_lists([A])
    cat = ctx.seg_concat([sb, sa])
    try:
        form_option(0)
        assert _run(ctx, [(cat, 0), (cat, 1)], want) in FUSED
        form_option(1)
        assert _run(ctx, [(cat, 0), (cat, 1)], want) in FUSED
        _form_is(cat, 1, A)
        assert sa.dense_form(0) is None                             # (its own store: nobody asked)
    finally:
        for s in (cat, sb, sa):
            s.free()


@pytest.mark.parametrize("spin", [-1, -2], ids=["early", "late"])
def test_give_up_with_a_form(ctx, form_option, pair, spin):
    """The bounded waits of the look-back run out on purpose (the existing test values of intersect.and2_spin): the call notices,
    repeats itself through the two-kernel form - which marks, form or not - and returns the right ids."""
    B, A, want = pair
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    try:
        assert _run(ctx, ls, want) in FUSED
        _form_is(seg, 1, A)
        ctx.set_option("intersect.and2_spin", spin)
        before = ctx.counters()[1]
        took = _run(ctx, ls, want)
        assert ctx.counters()[1] - before == 1
        assert took == {"and.and2_fused": 1, "and.and2_split": 1}
        ctx.set_option("intersect.and2_spin", 0)
        assert _run(ctx, ls, want) in FUSED
    finally:
        ctx.set_option("intersect.and2_spin", 0)
        seg.free()


def test_two_contexts_ask_first_at_the_same_time(ctx, form_option, pair):
    B, A, want = pair
    other = Context(0)
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    outs = [c.empty(want.size + 64) for c in (ctx, other)]
    start = threading.Barrier(2)
    res = [None, None]

    def ask(k, c):
        try:
            start.wait()
            res[k] = _run(c, ls, want, out=outs[k])
        except BaseException as e:      # noqa: BLE001 - handed to the main thread
            res[k] = e
    try:
        ts = [threading.Thread(target=ask, args=(k, c)) for k, c in enumerate((ctx, other))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for r in res:
            if isinstance(r, BaseException):
                raise r
            assert r in FUSED
        f = _form_is(seg, 1, A, other)
        assert f["store_bytes"] == dc.form_bytes(A) + 16            # one form, whoever made it
    finally:
        for o in outs:
            o.free()
        seg.free()
        other.close()


def test_the_forms_memory_comes_back_with_the_segment(ctx, form_option, pair):
    B, A, want = pair

    def live():
        v = C.c_uint64()
        ctx.lib.ii2_devmem_stats(C.byref(v), None)
        return v.value
    out = ctx.empty(want.size + 64)
    for _ in range(2):                                              # (the first turn also grows the context's own buffers)
        before = live()
        seg = ctx.encode_lists([B, A])
        with_seg = live()
        _run(ctx, [(seg, 0), (seg, 1)], want, out=out)
        _form_is(seg, 1, A)
        assert live() >= with_seg + dc.form_bytes(A)                # the form is counted ...
        seg.free()
        assert live() == before                                     # ... and leaves with the segment
    out.free()


def test_capacity_one_short(ctx, form_option, pair):
    B, A, want = pair
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    out = ctx.empty(want.size + 64)
    try:
        for opt in (0, 1, 1):
            form_option(opt)
            with pytest.raises(II2Error) as e:
                ctx.intersect(ls, out=out, cap=want.size - 1)
            assert e.value.code == ECAPACITY
        _form_is(seg, 1, A)
        _, n = ctx.intersect(ls, out=out, cap=want.size)            # exactly enough
        assert n == want.size and np.array_equal(out.download(n), want)
    finally:
        out.free()
        seg.free()
