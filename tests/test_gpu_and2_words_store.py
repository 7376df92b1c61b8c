"""GPU: where the word-by-word two-list AND (csrc/intersect_words.hip k_and2_words) puts its ids, under every instance of the
kernel: options intersect.and2_words_store (0 plain stores, 1 write-through stores at 16-byte-aligned addresses) x
intersect.and2_words_order (0 both chunks staged before the first store, 1 chunk 0's stores first).  Every case of
tests/and2_words_store_cases.py runs forced (and2_words = 2) under each: the ids equal numpy and each other, bit for bit, with
FILL behind the result, and the rows of cycle counters are the kernel's grid."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd.engine import II2Error
from tests import and2_words_cases as wc
from tests import and2_words_store_cases as sc
from tests import dense_form_cases as dc
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu
FILL = 0xDEADBEEF
ECAPACITY = -4
FUSED = {"and.and2_fused": 1}
DEFAULTS = (("intersect.and2_words", 1), ("intersect.and2_words_store", 1), ("intersect.and2_words_order", 0), ("intersect.and2_spin", 0),
            ("debug.stamps", 0))
INSTANCES = [(store, order) for store in (0, 1) for order in (0, 1)]
OTHER_STORE = 1 - dict(DEFAULTS)["intersect.and2_words_store"]


@pytest.fixture
def instance(ctx):
    ctx.set_option("intersect.and2_words", 2)

    def pick(store, order):
        ctx.set_option("intersect.and2_words_store", store)
        ctx.set_option("intersect.and2_words_order", order)
    yield pick
    for name, v in DEFAULTS:
        ctx.set_option(name, v)


def _run(c, ls, want, tomb=None):
    out = c.empty(want.size + 64)
    out.upload(np.full(out.count, FILL, np.uint32))
    try:
        with path_delta(c) as took:
            _, n = c.intersect(ls, tomb=tomb, out=out)
        got = out.download()
    finally:
        out.free()
    assert n == want.size
    assert np.all(got[n:] == FILL)                                   # nothing written past the result
    return got[:n], took


def _stamp_rows(c, ls, tomb=None):
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


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_case_under_every_instance(ctx, instance, case):
    x, y, removed = case.data()
    want = wc.reference(x, y, removed)
    seg = ctx.encode_lists([x, y])
    tomb = ctx.tombstones(removed) if removed is not None else None
    ls = [(seg, 0), (seg, 1)]
    try:
        first = None
        for store, order in INSTANCES:
            instance(store, order)
            got, took = _run(ctx, ls, want, tomb)
            assert took == FUSED, (store, order)
            assert np.array_equal(got, want), (store, order)
            first = got if first is None else first
            assert np.array_equal(got, first), (store, order)
            assert _stamp_rows(ctx, ls, tomb) == wc.workgroups(x, y), (store, order)
        assert seg.dense_form(0) is not None and seg.dense_form(1) is not None
    finally:
        seg.free()
        if tomb is not None:
            tomb.free()


@pytest.mark.parametrize("store,order", INSTANCES)
def test_capacity(ctx, instance, store, order):
    x, y, _ = sc.BY_NAME["capacity"].data()
    want = wc.reference(x, y)
    pos, _ = sc.capacity_positions(x, y)
    seg = ctx.encode_lists([x, y])
    ls = [(seg, 0), (seg, 1)]
    out = ctx.empty(want.size + 64)
    instance(store, order)
    try:
        for cap in (want.size - 1, pos["head"], pos["body"], pos["tail"]):
            out.upload(np.full(out.count, FILL, np.uint32))
            with pytest.raises(II2Error) as e:
                ctx.intersect(ls, out=out, cap=cap)
            assert e.value.code == ECAPACITY
            assert np.all(out.download()[cap:] == FILL), cap        # nothing at or beyond the capacity
        out.upload(np.full(out.count, FILL, np.uint32))
        _, n = ctx.intersect(ls, out=out, cap=want.size)             # exactly enough
        got = out.download()
        assert n == want.size and np.array_equal(got[:n], want) and np.all(got[n:] == FILL)
    finally:
        out.free()
        seg.free()


OLDER = [dc.BY_NAME["uniform"], wc.BY_NAME["stretches"], wc.BY_NAME["two_groups"]]


@pytest.mark.parametrize("case", OLDER, ids=lambda c: c.name)
def test_older_case_under_the_other_store_policy(ctx, instance, case):
    x, y, removed = case.data()
    want = wc.reference(x, y, removed)
    seg = ctx.encode_lists([x, y])
    ls = [(seg, 0), (seg, 1)]
    try:
        instance(OTHER_STORE, 0)
        got, took = _run(ctx, ls, want)
        assert took == FUSED and np.array_equal(got, want)
        assert _stamp_rows(ctx, ls) == wc.workgroups(x, y)
    finally:
        seg.free()


@pytest.mark.parametrize("spin", [-1, -2], ids=["early", "late"])
def test_give_up_under_write_through(ctx, instance, spin):
    """the look-back's bounded waits run out on purpose: the call repeats itself through the two-kernel form and returns the right
    ids; the counter of repeated calls goes up by one"""
    x, y, _ = dc.BY_NAME["uniform"].data()
    want = dc.reference(dc.BY_NAME["uniform"])
    seg = ctx.encode_lists([x, y])
    ls = [(seg, 0), (seg, 1)]
    try:
        instance(1, 0)
        got, took = _run(ctx, ls, want)
        assert took == FUSED and np.array_equal(got, want)
        ctx.set_option("intersect.and2_spin", spin)
        before = ctx.counters()[1]
        got, took = _run(ctx, ls, want)
        assert np.array_equal(got, want)
        assert ctx.counters()[1] - before == 1
        assert took == {"and.and2_fused": 1, "and.and2_split": 1}
        ctx.set_option("intersect.and2_spin", 0)
        got, took = _run(ctx, ls, want)
        assert took == FUSED and np.array_equal(got, want)
    finally:
        ctx.set_option("intersect.and2_spin", 0)
        seg.free()
