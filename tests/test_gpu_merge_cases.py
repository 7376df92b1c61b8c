"""GPU: every decision of the merge's plan and every recovery of its tile kernel, pinned.  For each case of tests/merge_cases.py
one ii2_merge_segments call must arrive at exactly the tile count of the plan model, show exactly the modelled delta of
Context.merge_events(), return the oracle's Shard.Merge (offsets, ids compared in uint64, counts) and leave the ids behind the
result untouched - with the direct placement and with the parking + packing pass (merge.direct = 1 / 0), without and with
tombstones.  Cases about what is written also compare ii2_merge_segments_to_seg byte for byte with the DV1 encoding of the
oracle's merge; the folded large term is unioned through ii2_union too (the merge passes, 'or.merge')."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import merge_cases as mc
from tests.gpu_util import ctx, path_delta  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = 0xDEADBEEF
OFF_SENTINEL = 0xABCDEF0123456789


def _delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def _segment_equals_oracle_encoding(seg, w_off, w_vals):
    oblk, oskip, opayload = orc.dv1_encode(w_off, w_vals)
    blk, skip, payload = seg.export()
    assert seg.info.n_postings == int(w_off[-1]) and seg.info.n_blocks == oskip.size - 1 and seg.info.n_bytes == opayload.size
    assert np.array_equal(blk, oblk)
    assert np.array_equal(skip["first_doc"], oskip["first_doc"]) and np.array_equal(skip["byte_off"], oskip["byte_off"])
    assert np.array_equal(payload, opayload)


def _filled(c, n):
    """n + 64 sentinel words; the entry points see n of them."""
    a = c.empty(n + 64).upload(np.full(n + 64, SENTINEL, np.uint32))
    a.count = n
    return a


def _ids_and_tail(a, n_out):
    cap = a.count
    a.count = cap + 64
    got = a.download()
    a.count = cap
    assert np.all(got[n_out:] == SENTINEL), "ids written behind the result"
    return got[:n_out].astype(np.uint64)


@pytest.mark.parametrize("case", mc.CASES, ids=lambda c: c.name)
def test_plan_events_and_result(ctx, case):
    host = case.segs()
    offs, vals = [o for o, _ in host], [v for _, v in host]
    T, n_in = offs[0].size - 1, int(sum(v.size for v in vals))
    removed = case.removed()
    want = {False: orc.merge_segments(offs, vals, ()), True: orc.merge_segments(offs, vals, removed)}
    plan, expect = case.plan(), case.events()
    segs = [ctx.encode(o, v) for o, v in host]
    tombs = {False: None, True: ctx.tombstones(removed)}
    out_off = ctx.empty(T + 1, np.uint64)
    try:
        for name, value in case.options.items():
            ctx.set_option(name, value)
        for direct in (1, 0):
            ctx.set_option("merge.direct", direct)
            for with_tomb in (False, True):
                w_off, w_vals, w_terms = want[with_tomb]
                n_out = int(w_off[-1])
                out_off.upload(np.full(T + 1, OFF_SENTINEL, np.uint64))
                out_vals = _filled(ctx, n_in)
                before, repeats = ctx.merge_events(), ctx.counters()[0]
                _, _, st = ctx.merge(segs, tombs[with_tomb], out_off, out_vals)
                delta = _delta(before, ctx.merge_events())
                print(case.name, "direct" if direct else "packed", "tomb" if with_tomb else "plain", "tiles", st.n_tiles, delta)
                assert ctx.counters()[0] == repeats                     # (a repeated merge would count its events twice)
                assert st.n_tiles == plan.n_tiles
                assert delta == expect
                assert np.array_equal(out_off.download(), w_off.astype(np.uint64))
                assert np.array_equal(_ids_and_tail(out_vals, n_out), w_vals.astype(np.uint64))
                assert (st.n_in, st.n_out, st.n_terms_out) == (n_in, n_out, w_terms)
                out_vals.free()
                if case.encoding:
                    before = ctx.merge_events()
                    merged, st2 = ctx.merge_to_segment(segs, tombs[with_tomb])
                    assert _delta(before, ctx.merge_events()) == expect and st2.n_tiles == plan.n_tiles
                    _segment_equals_oracle_encoding(merged, w_off, w_vals)
                    merged.free()
    finally:
        for name in list(case.options) + ["merge.direct"]:
            ctx.set_option(name, mc.DEFAULTS[name])
        for s in segs:
            s.free()
        tombs[True].free()


@pytest.mark.parametrize("case", [c for c in mc.CASES if c.union], ids=lambda c: c.name)
def test_union_counts_the_same_events(ctx, case):
    """The k lists of the case's one term as k lists of one segment, unioned: too many for the ranking kernel, too many postings
    for the small one, too few blocks for the tiles - the merge passes, which run the same tile kernel and count the same events."""
    lists = mc.lists_of(case.segs(), 0)
    removed = case.removed()
    plain = np.unique(np.concatenate(lists).astype(np.uint64))
    want = {False: plain, True: plain[~np.isin(plain, removed.astype(np.uint64))]}
    assert 0 < want[True].size < plain.size
    seg = ctx.encode_lists(lists)
    tombs = {False: None, True: ctx.tombstones(removed)}
    cap = 256 * sum((l.size + 255) // 256 for l in lists)
    try:
        for direct in (1, 0):
            ctx.set_option("merge.direct", direct)
            for with_tomb in (False, True):
                out = _filled(ctx, cap)
                before = ctx.merge_events()
                with path_delta(ctx) as paths:
                    _, n = ctx.union([(seg, i) for i in range(len(lists))], tomb=tombs[with_tomb], out=out)
                delta = _delta(before, ctx.merge_events())
                print(case.name, "union", "direct" if direct else "packed", "tomb" if with_tomb else "plain", paths, delta)
                assert paths == {"or.merge": 1}
                assert delta == case.events()
                assert n == want[with_tomb].size and np.array_equal(_ids_and_tail(out, n), want[with_tomb])
                out.free()
    finally:
        ctx.set_option("merge.direct", mc.DEFAULTS["merge.direct"])
        seg.free()
        tombs[True].free()


def test_events_belong_to_their_context(ctx):
    """The counters are the context's own: a second context starts at zero and does not see the first one's merges."""
    from inverted_index_2_amd import Context
    case = mc.BY_NAME["top_of_id_space_cluster"]
    other = Context(0)
    try:
        assert other.merge_events() == dict.fromkeys(mc.EVENTS, 0)
        before = ctx.merge_events()
        segs = [other.encode(o, v) for o, v in case.segs()]
        other.merge(segs)
        assert {k: v for k, v in other.merge_events().items() if v} == case.events()
        assert ctx.merge_events() == before
    finally:
        other.close()
