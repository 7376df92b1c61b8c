"""GPU: the dense two-list AND family (tests/dense_edge_cases.py: MODES) on every way of making a segment (tests/segment_kinds.py,
shape `pair`), against plain numpy.  Next to a list's DV1 bytes these kernels read what the maker derived - last_doc, the skip
entry one past the list's last block (a store's sentinel behind its last list: the form's criterion (b) takes the payload bytes
from it), the host span mirror or its device fetch, and the list's block number, the key of the form cache in the store - and until
now only for segments of ii2_seg_encode.  Segments are made once per module; merge_small cannot hold a list of 1024 blocks."""
import numpy as np
import pytest

from tests import dense_edge_cases as de
from tests import dense_form_cases as dc
from tests import segment_kinds as sk
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = [k for k in sk.KINDS if k not in sk.DENSE_EXEMPT]


@pytest.fixture(scope="module")
def made(ctx):
    """kind -> (segment, the objects it needs alive - a view's store first -, plan, dense queries, the lists whose spans were fetched
    where the segment keeps no host span mirror - dense_edge_cases.call): made once."""
    cache = {}

    def get(kind):
        if kind not in cache:
            p = sk.plan(kind, sk.DENSE_SHAPE)
            seg, alive = sk.make(ctx, p)
            cache[kind] = (seg, alive, p, sk.dense_queries(kind), {} if p.mirrored else {id(seg): set()})
        return cache[kind]
    yield get
    for seg, alive, _, _, _ in cache.values():
        seg.free()
        for s in alive:
            s.free()


@pytest.fixture(scope="module")
def tombs(ctx):
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = ctx.tombstones(sk.dense_queries(kind).removed)
        return cache[kind]
    yield get
    for t in cache.values():
        t.free()


def test_the_small_merge_holds_no_dense_list():
    assert sk.DENSE_EXEMPT == ("merge_small",) and sk.SMALL_MERGE_POSTINGS < sk.DENSE_MIN_BLOCKS * sk.BLOCK
    assert max(sk.nblk(l) for l in sk.plan("merge_small", sk.DENSE_SHAPE).slots) < sk.DENSE_MIN_BLOCKS


def _handles(seg, alive, p, q, slots):
    """every (segment, list) a slot is known by: the segment's own and, for a view, its parent's"""
    own = tuple((seg, i) for i in slots)
    return [own, tuple((alive[0], q.parent[i]) for i in slots)] if p.is_view else [own]


@pytest.mark.parametrize("kind", KINDS)
def test_a_list_that_fails_criterion_b_gets_no_form(ctx, made, tombs, kind):
    """The third list against A2, whose form would be 5 / 8 of its payload: with intersect.dense_form = 1 the one-launch AND marks
    A2 as before, also where the rule of the word kernel is asked (and2_words = 1 with a minimum of one block).  Criterion (b)
    takes A2's payload bytes from the skip entry behind its last block: A2 is the last non-empty list of a whole segment."""
    seg, alive, p, q, unmirrored = made(kind)
    ls = [(seg, q.third), (seg, q.a2)]
    known = _handles(seg, alive, p, q, q.crit)
    assert p.is_view or q.last_non_empty_of_store
    out = ctx.empty(q.T.size + 64)
    try:
        for opts in ({"intersect.dense_form": 1, "intersect.and2_tiles": 1}, {"intersect.dense_form": 1, "intersect.and2_words": 1, "intersect.and2_words_min": 1}):
            for refs, removed, tomb in ((ls, None, None), (ls[::-1], None, None), (ls, q.removed, tombs(kind))):
                with de.options(ctx, opts):
                    took = de.call(ctx, ctx.intersect, refs, de.reference([q.T, q.A2], removed), tomb, out, unmirrored)
                    assert took in de.FUSED, (opts, took)
                    assert de.stamp_rows(ctx, refs, tomb) == de.fused_rows(q.T)      # the fused kernel's grid, one tile a wave
                assert all(de.no_form(r) for pair in known for r in pair), opts
    finally:
        out.free()


@pytest.mark.parametrize("kind", KINDS)
def test_the_family_on_the_main_pair(ctx, made, tombs, kind):
    seg, alive, p, q, unmirrored = made(kind)
    ls = [(seg, q.b), (seg, q.a)]
    known = _handles(seg, alive, p, q, (q.b, q.a))
    # a view: the forms of modes 4 and 5 are made through the view and must show through the parent; mode 6 asks through the parent
    # and its second form must show through the view
    took = de.run_family(ctx, (q.B, q.A, q.T), ls, (seg, q.third), tombs=[(q.removed, tombs(kind))], seen_through=known,
                         words_ls=list(known[-1]), swapped=("fused_form",), unmirrored=unmirrored)
    print(kind, took)
    two_forms = dc.form_bytes(q.A) + dc.form_bytes(q.B) + 32
    assert seg.dense_form_bytes() == two_forms                                       # exactly two forms in the store ...
    assert all(de.no_form((seg, i)) for i in q.others)                               # ... and no other slot shows one, the empty ones included
    if p.is_view:
        store = alive[0]
        assert store.dense_form_bytes() == two_forms
        assert all(de.no_form((store, j)) for j in range(store.info.n_lists) if j not in (q.parent[q.b], q.parent[q.a]))


def test_a_pair_split_over_two_kinds(ctx):
    """B from a streamed merge, A from ii2_seg_build: each form lands in its own store."""
    made = []
    try:
        for kind in ("merge_stream", "build_pairs"):
            seg, alive = sk.make(ctx, sk.plan(kind, sk.DENSE_SHAPE))
            made.append((seg, alive))
        (ms, _), (bp, _) = made
        qm, qb = sk.dense_queries("merge_stream"), sk.dense_queries("build_pairs")
        assert np.array_equal(qm.A, qb.A)
        took = de.run_family(ctx, (qm.B, qb.A, qm.T), [(ms, qm.b), (bp, qb.a)], (ms, qm.third), swapped=("fused_form",))
        print(took)
        assert ms.dense_form_bytes() == dc.form_bytes(qm.B) + 16 and bp.dense_form_bytes() == dc.form_bytes(qb.A) + 16
        assert all(de.no_form((ms, i)) for i in range(ms.info.n_lists) if i != qm.b)
        assert all(de.no_form((bp, i)) for i in range(bp.info.n_lists) if i != qb.a)
    finally:
        for seg, alive in made:
            seg.free()
            for s in alive:
                s.free()
