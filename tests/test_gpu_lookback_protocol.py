"""GPU: the look-back protocol of csrc/lookback.h, branch by branch, against the plain-Python specification of
tests/lookback_cases.py.

k_and2_fused and k_enc_stream take whichever branch of the protocol the timing of a launch gives them, and a wrong offset there
faults nowhere.  ii2_lookback_check (csrc/lookback_check.hip) runs the same functions of lookback.h without a payload, on the
context's own records and epochs, over a record state the test chooses: a seeded case finds everything outside its own group
exactly as the table says, so the prefix, the windows it looked at and the place of the prefix record it used are predicted
exactly, and the decoys in the records nobody may read show in the sum when somebody does.  The live cases launch whole grids
(up to 100 000 workgroups) and compare every prefix with numpy's cumulative sum and every record with what the protocol says it
holds afterwards.  The last tests put the real kernels and the check on ONE set of records, across the wrap of the 24-bit epoch
and the growth of the records."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import Context
from inverted_index_2_amd.engine import II2Error
from oracle import oracle as orc
from tests import lookback_cases as lc
from tests.gpu_util import ctx, path_delta  # noqa: F401
from tests.test_gpu_lookback import _async_and, _async_result, _merge_case, _sync_and, pair  # noqa: F401
from tests.test_gpu_merge import _segment_equals_oracle_encoding

pytestmark = pytest.mark.gpu
EINVAL = -1
LB_RECORDS_MIN = 4096                   # workgroups the look-back records hold at first (api.cpp: ii2_lookback_prepare)


def _tag(epoch):
    return epoch << lc.VALUE_BITS


def _ensure_records(c, n_wg):
    """the records hold n_wg workgroups (growing them starts the epochs again: not behind a debug.lb_epoch)"""
    if c.lookback_check(1, [0], lc.SPIN)["cap"] < n_wg:
        assert c.lookback_check(n_wg, np.zeros(n_wg, np.uint64), lc.SPIN)["cap"] >= n_wg


def _run_seeded(c, case, k):
    rec = case.records()
    state, value = rec.seeds()
    g_base = lc.GROUP * case.G
    amount = np.zeros(g_base + k, np.uint64)
    amount[g_base:] = case.amounts()[:k]
    if case.epoch is not None:
        _ensure_records(c, g_base + k)
        c.set_option("debug.lb_epoch", case.epoch - 1)
    r = c.lookback_check(g_base + k, amount, lc.SPIN_GIVE_UP if case.gives_up else lc.SPIN, g_base, state, value)
    if case.epoch is not None:
        assert r["epoch"] == case.epoch
    return rec, r


def _check_seeded(case, k, rec, r):
    live = case.amounts()[:k]
    want = [lc.walk(rec, i, live) for i in range(k)]
    print(case.name, k, "epoch", r["epoch"], "polls max", int(r["polls"].max()), "windows", set(r["windows"].tolist()), "dist", set(r["dist"].tolist()))
    agg, grp = lc.expected_records(case, k, r["epoch"]) if not case.gives_up else (None, None)
    if case.gives_up:
        assert all(w.prefix is None for w in want)
        assert r["state"].tolist() == [lc.GAVE_UP_PREFIX] * k                   # every one of them, and nothing but the prefix wait
        assert r["err"] == r["epoch"]
        assert r["prefix"].tolist() == [0] * k
        assert r["agg"].tolist() == [_tag(r["epoch"]) | int(a) for a in live]   # the amounts were published all the same ...
        assert int(r["grp"][0]) == _tag(r["epoch"]) | int(live.sum())           # ... and so was the group's
        return
    assert r["state"].tolist() == [0] * k and r["err"] != r["epoch"]
    assert r["prefix"].tolist() == [w.prefix for w in want]
    assert r["windows"].tolist() == [w.windows for w in want] and r["dist"].tolist() == [w.dist for w in want]
    assert r["agg"].tolist() == agg and r["grp"].tolist() == grp


@pytest.mark.parametrize("case", lc.CASES, ids=lambda c: c.name)
def test_seeded_case(ctx, pair, case):
    for k in lc.SIZES:
        rec, r = _run_seeded(ctx, case, k)
        _check_seeded(case, k, rec, r)
    if case.gives_up:
        # the give-up was this call's own: nothing of it is reported later, and the next real launch is exact
        ctx.sync()
        assert _sync_and(ctx, pair["ls"], pair["want"]) == (pair["want"].size, 0, True, True)


def _check_live(r, amounts):
    pre, agg, grp = lc.live_expected(amounts, r["epoch"])
    assert not r["state"].any() and r["err"] != r["epoch"]
    assert np.array_equal(r["prefix"], pre)
    assert np.array_equal(r["agg"], agg)
    assert np.array_equal(r["grp"], grp)


@pytest.mark.parametrize("n_wg", lc.LIVE_SIZES)
def test_live_case(ctx, n_wg):
    c = Context(0) if n_wg == LB_RECORDS_MIN + 1 else ctx          # (the first size that does not fit new records: on new records)
    try:
        cap0 = c.lookback_check(1, [0], lc.SPIN)["cap"]
        walked = False
        for delayed in (False, True):
            amounts = lc.live_amounts(n_wg, seed=int(delayed))
            r = c.lookback_check(n_wg, amounts, lc.SPIN, delay=lc.live_delays(n_wg) if delayed else None)
            print(n_wg, "delayed" if delayed else "plain", "polls max", int(r["polls"].max()), "windows max", int(r["windows"].max()),
                  "prefix records used at", sorted(set(r["dist"].tolist()) - {lc.NO_PREFIX}))
            _check_live(r, amounts)
            assert r["cap"] >= n_wg
            assert int(r["windows"].max()) <= max(((n_wg - 1) // lc.GROUP - 2) // lc.WINDOW + 1, 0)
            walked |= bool(np.any(r["windows"] >= 2) or np.any((r["dist"] != lc.NO_PREFIX) & (r["dist"] >= 1)))
        if n_wg == LB_RECORDS_MIN + 1:
            assert cap0 == LB_RECORDS_MIN and r["cap"] > cap0      # the records grew, and a real grid ran on the new ones at once
        if n_wg == 100_000:
            assert walked          # somewhere the walk went further than the nearest group's prefix
    finally:
        if c is not ctx:
            c.close()


def _encode_case(c, seed):
    """a merge whose result the one-pass encoder writes with three workgroups or more: byte for byte the oracle's encoding"""
    offs, vals, removed = _merge_case(np.random.default_rng(seed))
    w_off, w_vals, _ = orc.merge_segments(offs, vals, removed)
    assert int(w_off[-1]) >= 3 * 8192
    segs = [c.encode(o, v) for o, v in zip(offs, vals)]
    before = c.counters()[1]
    merged, st = c.merge_to_segment(segs, c.tombstones(removed))
    assert c.counters()[1] == before and st.n_out == int(w_off[-1])
    _segment_equals_oracle_encoding(merged, w_off, w_vals)
    merged.free()
    for s in segs:
        s.free()


def _live(c, n_wg, seed, delayed=True):
    amounts = lc.live_amounts(n_wg, seed=seed)
    r = c.lookback_check(n_wg, amounts, lc.SPIN, delay=lc.live_delays(n_wg) if delayed else None)
    _check_live(r, amounts)
    return r


def test_epoch_wrap_with_real_kernels(pair):
    """The records are never cleared between launches: the epoch alone tells a fresh record from an old one, and when its 24 bits
    wrap the host clears them.  Four launches pass the wrap here - 2^24 - 1, 1, 2, 3 - and the records still hold, from before,
    amounts of 300 workgroups tagged 3 (three checks at the epochs 1, 2, 3 of the new context; the first alone would leave
    them tagged 1, where only the second AND, whose workgroups look at each other's records by chance, could meet them).  A wrap
    that did not clear would hand exactly those to the fourth launch, a check of 300 other amounts whose late publishers make
    their successors poll."""
    c = Context(0)
    try:
        ls, want = pair["ls"], pair["want"]
        assert [_live(c, 300, 10 + i)["epoch"] for i in range(3)] == [1, 2, 3]
        c.set_option("debug.lb_epoch", lc.EPOCH_MAX - 1)
        fallbacks = c.counters()[1]
        assert _sync_and(c, ls, want) == (want.size, 0, True, True)                              # epoch 2^24 - 1
        out, dcnt = c.empty(want.size + 64), c.empty(8, np.uint64)
        _async_and(c, ls, out, dcnt)                                                             # the wrap: epoch 1
        c.sync()
        n, got = _async_result(out, dcnt)
        assert n == want.size and np.array_equal(got, want)
        kept = np.setdiff1d(want, pair["removed"], assume_unique=True).astype(np.uint32)
        assert _sync_and(c, ls, kept, tomb=c.tombstones(pair["removed"])) == (kept.size, 0, True, True)      # epoch 2
        assert c.counters()[1] == fallbacks
        r = _live(c, 300, 20)
        assert r["epoch"] == 3                                                                   # the epoch the old records carry
        _encode_case(c, 53)
        assert c.lookback_check(1, [0], lc.SPIN)["epoch"] == 5
    finally:
        c.close()


def test_wrap_keeps_a_pending_async_give_up(pair):
    c = Context(0)
    try:
        ls, want = pair["ls"], pair["want"]
        assert _sync_and(c, ls, want) == (want.size, 0, True, True)
        out, dcnt = c.empty(want.size + 64), c.empty(8, np.uint64)
        c.set_option("debug.lb_epoch", lc.EPOCH_MAX - 1)
        c.set_option("intersect.and2_spin", -2)
        _async_and(c, ls, out, dcnt)                                  # epoch 2^24 - 1: gives up late, nobody has looked yet
        c.set_option("intersect.and2_spin", 0)
        assert _sync_and(c, ls, want) == (want.size, 0, True, True)   # the wrap: the records, error word included, are cleared
        with pytest.raises(II2Error):
            c.sync()
        c.sync()                                                      # reported once
        assert c.lookback_check(1, [0], lc.SPIN)["epoch"] == 2
    finally:
        c.set_option("intersect.and2_spin", 0)
        c.close()


def test_check_and_real_kernels_share_the_records(pair):
    c = Context(0)
    try:
        ls, want = pair["ls"], pair["want"]
        fallbacks = c.counters()[1]
        with path_delta(c) as took:
            assert _sync_and(c, ls, want) == (want.size, 0, True, True)
            assert c.lookback_check(1, [0], lc.SPIN)["cap"] == LB_RECORDS_MIN
            assert _live(c, LB_RECORDS_MIN + 1, 30)["cap"] > LB_RECORDS_MIN            # new records ...
            assert _sync_and(c, ls, want) == (want.size, 0, True, True)                # ... and a real kernel right on them
            case = lc.BY_NAME["g40_big"]
            _check_seeded(case, 64, *_run_seeded(c, case, 64))
            _encode_case(c, 59)
            c.set_option("intersect.dense_form", 2)
            c.set_option("intersect.and2_tiles", 2)
            assert _sync_and(c, ls, want) == (want.size, 0, True, True)
        assert took == {"and.and2_fused": 3} and c.counters()[1] == fallbacks
    finally:
        c.close()


def test_argument_errors_touch_nothing(ctx):
    n, gb = 130, 64
    n_seed = gb + 2
    amount, state, value, delay = np.ones(n, np.uint64), np.ones(n_seed, np.uint8), np.ones(n_seed, np.uint64), np.zeros(n, np.uint16)
    FILL = 0xA5
    outs = [np.full(n, FILL, t) for t in (np.uint64, np.uint32, np.uint32, np.uint32, np.uint64)] + [np.full(6, FILL, np.uint64), np.full(4, FILL, np.uint64)]
    p = lambda a: None if a is None else C.c_void_p(a.ctypes.data)

    def call(n_wg=n, g_base=gb, amount=amount, spin=lc.SPIN, state=state, value=value, delay=delay, drop=None):
        o = [None if i == drop else a for i, a in enumerate(outs)]
        return ctx.lib.ii2_lookback_check(ctx.h, n_wg, g_base, p(amount), spin, p(state), p(value), p(delay), *[p(a) for a in o])

    def but(a, i, v):
        b = a.copy()
        b[i] = v
        return b
    epoch = ctx.lookback_check(1, [0], lc.SPIN)["epoch"]
    bad = [dict(n_wg=0), dict(n_wg=(1 << 24) + 1), dict(g_base=n), dict(g_base=192), dict(g_base=32), dict(amount=None), dict(spin=0), dict(spin=65537),
           dict(amount=but(amount, 7, 1 << 40)), dict(amount=but(but(amount, 3, 1 << 39), 99, 1 << 39)), dict(delay=but(delay, 129, 257)),
           dict(state=None), dict(value=None), dict(state=but(state, 65, 4)), dict(value=but(value, 0, 1 << 40))] + [dict(drop=i) for i in range(len(outs))]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert ctx.lib.ii2_lookback_check(None, n, gb, p(amount), lc.SPIN, p(state), p(value), p(delay), *[p(a) for a in outs]) == EINVAL
        assert all(bool(np.all(a == FILL)) for a in outs), kw
    assert ctx.lookback_check(1, [0], lc.SPIN)["epoch"] == epoch + 1          # nothing was launched in between
    assert call() == 0 and int(outs[-1][0]) == epoch + 2                      # the same arguments, unbroken: it runs,
    assert not outs[1][:n - gb].any() and bool(np.all(outs[1][n - gb:] == FILL))         # one entry per launched workgroup
