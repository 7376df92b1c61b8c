"""GPU: give-ups of the kernels whose workgroups wait for each other inside one launch (csrc/lookback.h: the one-launch two-list
AND, k_and2_fused, and the one-pass encoder behind a merge, k_enc_stream) reach the host however late they come.

Every wait there is bounded; a workgroup whose wait runs out writes no output and stores its launch's epoch into the error
word, and the host repeats the call on a path without waits.  The last workgroup only poisons the count when it already sees
that word set, so a give-up AFTER it looked leaves a count that looks valid.  The test values intersect.and2_spin = -2 and
encode.stream = -2 force exactly that: one workgroup in the middle of the grid gives up only once the last workgroup has
stored the count (and, if it never sees that, gives up not at all - then the "repeated once" assertions below fail instead
of passing by chance).  Results are compared bit-exact with numpy / the oracle."""
import numpy as np
import pytest

from inverted_index_2_amd import Context
from inverted_index_2_amd.engine import II2Error
from oracle import oracle as orc
from tests.gpu_util import ctx, sorted_unique  # noqa: F401
from tests.test_gpu_merge import _segment_equals_oracle_encoding

pytestmark = pytest.mark.gpu
FILL = 0xDEADBEEF
AND_WG_POSTINGS = 4 * 16 * 256          # driver postings per workgroup of k_and2_fused (4 waves x 16 DV1 blocks)
ENC_WG_IDS = 8192                       # ids per workgroup of k_enc_stream
LB_RECORDS_MIN = 4096                   # workgroups the look-back records hold at first (api.cpp: ii2_lookback_prepare)


def bernoulli(rng, p, lo, hi):
    return (np.flatnonzero(rng.random(hi - lo) < p) + lo).astype(np.uint32)


@pytest.fixture(scope="module")
def pair(ctx):
    """A dense pair: ~2.4M driver postings, ~150 workgroups of the one-launch AND (more than two groups of 64)."""
    rng = np.random.default_rng(31)
    U = 8_000_000
    a, b = bernoulli(rng, 0.5, 0, U), bernoulli(rng, 0.3, 0, U)
    assert b.size // AND_WG_POSTINGS >= 130
    removed = np.sort(rng.choice(U, 40_000, replace=False)).astype(np.uint32)
    seg = ctx.encode_lists([a, b])
    return dict(a=a, b=b, removed=removed, seg=seg, ls=[(seg, 0), (seg, 1)],
                want=np.intersect1d(a, b, assume_unique=True).astype(np.uint32))


def _merge_case(rng, k=4, T=600, max_len=120, universe=2_000_000):
    offs, vals = [], []
    for _ in range(k):
        lens = rng.integers(0, max_len + 1, T)
        lens[rng.random(T) < 0.3] = 0
        v = [sorted_unique(rng, int(n), universe) for n in lens]
        offs.append(np.concatenate([[0], np.cumsum([x.size for x in v])]).astype(np.uint64))
        vals.append(np.concatenate(v + [np.empty(0, np.uint32)]).astype(np.uint32))
    removed = np.unique(rng.integers(0, universe, 20_000)).astype(np.uint32)
    return offs, vals, removed


def _sync_and(c, ls, want, tomb=None, out=None):
    """ii2_intersect into a buffer filled with FILL: (count, fallbacks taken, ids exact, nothing written past the count)."""
    if out is None:
        out = c.empty(want.size + 64)
    out.upload(np.full(out.count, FILL, np.uint32))
    before = c.counters()[1]
    _, n = c.intersect(ls, tomb=tomb, out=out)
    got = out.download()
    return n, c.counters()[1] - before, bool(n == want.size and np.array_equal(got[:n], want)), bool(np.all(got[n:] == FILL))


def _late_and(c, ls, want, tomb=None):
    c.set_option("intersect.and2", 1)
    c.set_option("intersect.and2_spin", -2)
    try:
        n, fallbacks, exact, tail = _sync_and(c, ls, want, tomb)
    finally:
        c.set_option("intersect.and2_spin", 0)
    # one late give-up, noticed by the call and repeated once through the two-kernel form: exact, nothing past the count
    assert (n, fallbacks, exact, tail) == (want.size, 1, True, True)


def _async_and(c, ls, out, dcnt, tomb=None):
    out.upload(np.full(out.count, FILL, np.uint32))
    dcnt.upload(np.zeros(dcnt.count, np.uint64))
    c.intersect_async(ls, tomb, out, dcnt)


def _async_result(out, dcnt):
    n = int(dcnt.download(1)[0])
    return n, out.download(min(n, out.count))


# ---- 1. a late give-up inside a synchronous ii2_intersect
def test_late_give_up_sync_and(ctx, pair):
    _late_and(ctx, pair["ls"], pair["want"])


def test_late_give_up_sync_and_with_tombstones(ctx, pair):
    want = np.setdiff1d(pair["want"], pair["removed"], assume_unique=True).astype(np.uint32)
    _late_and(ctx, pair["ls"], want, tomb=ctx.tombstones(pair["removed"]))


def test_late_give_up_sync_and_lists_in_two_segments(ctx, pair):
    s0, s1 = ctx.encode_lists([pair["a"]]), ctx.encode_lists([pair["b"]])
    _late_and(ctx, [(s0, 0), (s1, 0)], pair["want"])


# ---- 2. ... inside an asynchronous one: ii2_ctx_sync reports it although the count looks valid
def test_late_give_up_async_and_is_reported_at_sync(ctx, pair):
    want = pair["want"]
    out, dcnt = ctx.empty(want.size + 64), ctx.empty(8, np.uint64)
    ctx.set_option("intersect.and2", 1)
    try:
        ctx.set_option("intersect.and2_spin", -2)
        _async_and(ctx, pair["ls"], out, dcnt)
        with pytest.raises(II2Error):
            ctx.sync()
        assert int(dcnt.download(1)[0]) == want.size        # (late: the last workgroup had stored a count that looks valid)
        ctx.set_option("intersect.and2_spin", 0)
        _async_and(ctx, pair["ls"], out, dcnt)              # the next call is clean again
        ctx.sync()
        n, got = _async_result(out, dcnt)
        assert n == want.size and np.array_equal(got, want)
    finally:
        ctx.set_option("intersect.and2_spin", 0)
        try:
            ctx.sync()
        except II2Error:
            pass


# ---- 3. a late give-up of the one-pass encoder behind ii2_merge_segments_to_seg
def test_late_give_up_encoder(ctx):
    rng = np.random.default_rng(41)
    offs, vals, removed = _merge_case(rng)
    w_off, w_vals, _ = orc.merge_segments(offs, vals, removed)
    assert int(w_off[-1]) >= 3 * ENC_WG_IDS                  # at least three encoder workgroups: one in the middle gives up
    segs = [ctx.encode(o, v) for o, v in zip(offs, vals)]
    ctx.set_option("encode.stream", -2)
    try:
        before = ctx.counters()[1]
        merged, st = ctx.merge_to_segment(segs, ctx.tombstones(removed))
        fallbacks = ctx.counters()[1] - before
    finally:
        ctx.set_option("encode.stream", 1)
    assert st.n_out == int(w_off[-1])
    assert fallbacks == 1                                   # seen by the call, encoded again by the two-pass encoder
    _segment_equals_oracle_encoding(merged, w_off, w_vals)   # offsets, ids and the exported DV1 bytes
    merged.free()


# ---- 4. an asynchronous give-up survives whatever comes between it and ii2_ctx_sync
def _async_failure_then(c, ls, want, between):
    out, dcnt = c.empty(want.size + 64), c.empty(8, np.uint64)
    c.set_option("intersect.and2", 1)
    try:
        c.set_option("intersect.and2_spin", -1)
        _async_and(c, ls, out, dcnt)
        c.set_option("intersect.and2_spin", 0)
        between()
        with pytest.raises(II2Error):
            c.sync()
        c.sync()                                            # reported once
    finally:
        c.set_option("intersect.and2_spin", 0)
        try:
            c.sync()
        except II2Error:
            pass


def test_async_failure_survives_a_sync_intersect(ctx, pair):
    def between():
        n, fallbacks, exact, tail = _sync_and(ctx, pair["ls"], pair["want"])
        assert (n, fallbacks, exact, tail) == (pair["want"].size, 0, True, True)
    _async_failure_then(ctx, pair["ls"], pair["want"], between)


def test_async_failure_survives_a_merge_to_segment(ctx, pair):
    offs, vals, removed = _merge_case(np.random.default_rng(43))
    w_off, w_vals, _ = orc.merge_segments(offs, vals, removed)
    segs = [ctx.encode(o, v) for o, v in zip(offs, vals)]

    def between():
        before = ctx.counters()[1]
        merged, _ = ctx.merge_to_segment(segs, ctx.tombstones(removed))
        assert ctx.counters()[1] == before
        po, v = merged.decode()
        assert np.array_equal(po, w_off) and np.array_equal(v, w_vals)
        merged.free()
    _async_failure_then(ctx, pair["ls"], pair["want"], between)


def test_async_failure_survives_new_look_back_records(pair):
    """A fresh context: its first (small) launch gives up; the next one has more workgroups than the records hold, so they are
    allocated again and cleared before it runs."""
    N = (LB_RECORDS_MIN + 4) * AND_WG_POSTINGS              # > LB_RECORDS_MIN workgroups of the one-launch AND
    big = np.arange(N, dtype=np.uint32)
    c = Context(0)
    try:
        seg = c.encode_lists([big, big])
        bls = [(seg, 0), (seg, 1)]
        bout, bcnt = c.empty(N + 64), c.empty(8, np.uint64)

        def between():
            _async_and(c, bls, bout, bcnt)
        _async_failure_then(c, pair["ls"], pair["want"], between)
        n, got = _async_result(bout, bcnt)
        assert n == N and np.array_equal(got, big)
        # (witness: this shape does go through the one-launch AND - a late give-up there is repeated)
        _late_and(c, bls, big)
    finally:
        c.close()


# ---- 5. a synchronous call's own give-up, handled there, is not reported again by ii2_ctx_sync
def test_handled_sync_give_up_is_no_false_alarm(ctx, pair):
    want = pair["want"]
    out, dcnt = ctx.empty(want.size + 64), ctx.empty(8, np.uint64)
    ctx.set_option("intersect.and2", 1)
    try:
        _async_and(ctx, pair["ls"], out, dcnt)              # clean, not yet synchronised ...
        _late_and(ctx, pair["ls"], want)                    # ... a synchronous AND gives up late and repeats itself ...
        ctx.sync()                                          # ... nothing to report
        n, got = _async_result(out, dcnt)
        assert n == want.size and np.array_equal(got, want)
        offs, vals, removed = _merge_case(np.random.default_rng(47))
        w_off, w_vals, _ = orc.merge_segments(offs, vals, removed)
        segs = [ctx.encode(o, v) for o, v in zip(offs, vals)]
        _async_and(ctx, pair["ls"], out, dcnt)
        ctx.set_option("encode.stream", -2)                 # the same with the one-pass encoder
        before = ctx.counters()[1]
        merged, _ = ctx.merge_to_segment(segs, ctx.tombstones(removed))
        ctx.set_option("encode.stream", 1)
        assert ctx.counters()[1] == before + 1
        ctx.sync()
        n, got = _async_result(out, dcnt)
        assert n == want.size and np.array_equal(got, want)
        po, v = merged.decode()
        assert np.array_equal(po, w_off) and np.array_equal(v, w_vals)
        merged.free()
    finally:
        ctx.set_option("intersect.and2_spin", 0)
        ctx.set_option("encode.stream", 1)


# ---- 6. the per-device order of look-back launches across contexts (ii2_lookback_launch): counted stream waits
def test_ordering_inserts_a_wait_at_each_switch_of_context(pair):
    """Strictly one call after the other, each synchronous: nothing overlaps.  Each switch to the other context puts one wait
    in front of its launch; a context alone needs none; debug.no_chain takes the order away."""
    ls, want = pair["ls"], pair["want"]
    out_len = want.size + 64

    def run(c):
        n, fallbacks, exact, tail = _sync_and(c, ls, want, out=c.empty(out_len))
        assert (n, fallbacks, exact, tail) == (want.size, 0, True, True)
        return c.counters()[3]

    A, B = Context(0), Context(0)
    try:
        run(A)                                              # (its first launch may follow another context's)
        a0, b0 = A.counters()[3], B.counters()[3]
        assert run(B) == b0 + 1
        assert run(A) == a0 + 1
        assert run(B) == b0 + 2
    finally:
        A.close()
        B.close()
    C, D = Context(0), Context(0)
    try:
        for c in (C, D):
            c.set_option("debug.no_chain", 1)
        assert [run(C), run(D), run(C)] == [0, 0, 0]
    finally:
        C.close()
        D.close()
    E = Context(0)                                          # (the contexts above are gone: nothing of them to wait for)
    try:
        assert [run(E), run(E), run(E)] == [0, 0, 0]
    finally:
        E.close()
