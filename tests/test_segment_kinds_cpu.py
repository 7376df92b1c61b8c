"""CPU: the table of segment kinds itself (tests/segment_kinds.py) - every maker is there, every edge the derived arrays can go
wrong at occurs in some shape, every plan has the structure its kind is about, and the numpy reference agrees with the block table
of the oracle's encoding of the store."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import segment_kinds as sk


def test_every_maker_has_a_kind():
    assert set(sk.KINDS) == {"encode_host", "encode_device", "build_pairs", "import_oracle", "merge_stream", "merge_two_pass",
                             "merge_tomb_stream", "merge_tomb_two_pass", "select", "select_aligned", "select_aligned_all",
                             "merge_small", "concat", "allgather", "big"}
    assert len(sk.CASES) == len(sk.KINDS) * len(sk.SHAPES)
    for k, (plan, make, is_view, aligned) in sk.KINDS.items():
        assert is_view == k.startswith("select") and aligned == k.startswith("select_aligned"), k


def test_the_shapes_hold_every_edge():
    shapes = {n: sk.shape(n) for n in sk.SHAPES}
    every = [l for s in shapes.values() for l in s]
    lens = {len(l) for l in every}
    assert {0, 1, 255, 256, 257, 511, 512, 513, 16384} <= lens
    assert any(l.tolist() == [0] for l in every)
    assert any(len(l) > 1 and l[-1] == 0xFFFFFFFF for l in every) and any(l.tolist() == [0xFFFFFFFF] for l in every)
    assert any(len(l) > 1 and l[0] == 0 for l in every)
    assert any(len(l) > 256 and len(l) % 256 == 1 for l in every)                   # a last block of one posting
    for name, s in shapes.items():
        assert all(l.dtype == np.uint32 and np.all(np.diff(l.astype(np.int64)) > 0) for l in s), name
        if name == sk.DENSE_SHAPE:                                                   # (the one large shape: see the tests of dense_queries)
            continue
        assert sum(len(l) for l in s) < 60_000, name
        span = max(int(l[-1]) for l in s if len(l)) - min(int(l[0]) for l in s if len(l))
        assert 2048 < span < (1 << 19), name                                         # several 2048-doc windows, not thousands
    s = shapes["lengths"]
    assert len(s[0]) == 0 and len(s[-1]) == 0                                        # empty first and last ...
    assert any(len(a) == 0 and len(b) == 0 for a, b in zip(s, s[1:]))                # ... and in a run
    a, b, c = s[2], s[3], s[4]
    assert b[0] == a[-1] and b[1] > a[-1] and c[0] > b[-1]
    crowd = shapes["crowd"]
    n = np.array([len(l) for l in crowd])
    assert n.size > 3000 and n.max() == 20000 and np.sum(n > 3) == 1 and set(n[n <= 3]) == {0, 1, 2, 3}
    start = np.concatenate([[0], np.cumsum(n)])[:-1]
    big = int(np.argmax(n))
    assert start[big] % 1024 != 0 and (start[big] + 20000) // 8192 - start[big] // 8192 >= 2      # inside a partition, across workgroups
    assert np.max(np.bincount(start[n > 0] // 1024)) > 64                             # more than 64 list starts in one 1024-id tile
    assert np.all(n[:3] == 0) and np.all(n[-2:] == 0) and 0 < big < n.size - 1


@pytest.mark.parametrize("kind,shape", sk.CASES)
def test_reference_agrees_with_the_oracles_block_table(kind, shape):
    p = sk.plan(kind, shape)
    r = sk.reference(p)
    store = [l for l, _ in p.store]
    po, flat = sk.csr(store)
    blk, skip, payload = orc.dv1_encode(po, flat)
    assert np.array_equal(np.diff(blk.astype(np.int64)), [sk.nblk(l) for l in store])
    assert r.n_blocks == int(blk[-1]) and r.n_bytes == payload.size and r.blk_list.size == r.n_blocks + 1
    assert r.blk_list[-1] == sk.NONE
    seen = set()
    for j, (l, slot) in enumerate(p.store):
        b0, b1 = int(blk[j]), int(blk[j + 1])
        assert np.all(r.blk_list[b0:b1] == (sk.NONE if slot is None else slot))
        if slot is None:
            continue
        assert slot not in seen and np.array_equal(p.slots[slot], l)
        seen.add(slot)
        assert r.cnt[slot] == len(l)
        if b1 > b0:
            assert tuple(r.spans[slot]) == (skip["first_doc"][b0], skip["first_doc"][b1 - 1], l[-1]) and r.last_doc[slot] == l[-1]
    for i, l in enumerate(p.slots):                       # slots no list of the store stands behind are empty
        if i not in seen:
            assert len(l) == 0
        if len(l) == 0:
            assert r.cnt[i] == 0 and r.last_doc[i] == 0 and not r.spans[i].any()
    owned = [j for j, (_, slot) in enumerate(p.store) if slot is not None]
    assert owned == list(range(owned[0], owned[-1] + 1))                              # a window: consecutive lists of the store
    b0, b1 = int(blk[owned[0]]), int(blk[owned[-1] + 1])
    assert r.win_blocks == b1 - b0 and r.win_bytes == int(skip["byte_off"][b1]) - int(skip["byte_off"][b0])
    if not p.is_view:
        assert (r.win_blocks, r.win_bytes, r.sum_cnt) == (r.n_blocks, r.n_bytes, r.store_postings)
    assert p.mirrored == (not p.aligned and kind != "big")


@pytest.mark.parametrize("shape", sk.SHAPES)
def test_every_plan_has_the_structure_its_kind_is_about(shape):
    lists = sk.shape(shape)
    same = lambda a, b: len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    for kind in ("encode_host", "encode_device", "import_oracle", "allgather", "build_pairs", "merge_stream", "merge_two_pass"):
        assert same(sk.plan(kind, shape).slots, lists), kind
    p = sk.plan("build_pairs", shape).inputs
    assert p.list_ids.size > sum(len(l) for l in lists) and np.any(np.diff(p.list_ids.astype(np.int64)) < 0)      # repeats, shuffled
    pairs = np.unique(np.stack([p.list_ids, p.values]), axis=1)
    assert pairs.shape[1] == sum(len(l) for l in lists)
    for kind in ("merge_stream", "merge_tomb_stream"):
        p = sk.plan(kind, shape)
        a, b = p.inputs.segs
        rem = p.inputs.removed if p.inputs.removed is not None else sk.E
        assert same(p.slots, [np.setdiff1d(np.union1d(x, y), rem).astype(np.uint32) for x, y in zip(a, b)])
        assert any(len(np.intersect1d(x, y)) and len(np.setdiff1d(x, y)) and len(np.setdiff1d(y, x)) for x, y in zip(a, b))
    p = sk.plan("merge_tomb_two_pass", shape)
    n = len(p.slots)
    assert p.inputs.emptied[0] == 0 and 0 < p.inputs.emptied[1] < n - 1 and p.inputs.emptied[2] == n - 1
    for s in p.inputs.emptied:                                                       # whole lists emptied by the tombstones
        assert len(np.union1d(p.inputs.segs[0][s], p.inputs.segs[1][s])) > 0 and len(p.slots[s]) == 0
    assert sum(len(l) for l in p.slots) < sum(len(l) for l in lists)                 # ... and docs inside other lists
    p = sk.plan("select", shape)
    src = p.inputs.src_list
    assert src[0] == -1 and src[-1] == -1 and np.any(src[1:-1][1:-1] == -1) and np.any(src >= 0)
    first, last = np.flatnonzero(src >= 0)[[0, -1]]
    assert np.any(src[first:last] == -1)                                             # an inner empty slot
    assert p.store[0][1] is None and len(p.store[0][0]) > 256 and p.store[-1][1] is None and len(p.store[-1][0]) > 0      # the window lies in the middle
    assert same([p.slots[i] for i in np.flatnonzero(src >= 0)], lists)
    for kind, fl in (("select_aligned", 0), ("select_aligned_all", len(sk.JUNK_BEFORE))):
        p = sk.plan(kind, shape)
        assert p.inputs.first_list == fl and len(p.slots[0]) == 0 and p.inputs.union[0] not in p.inputs.dicts[0]
        assert same([l for l, t in zip(p.slots, p.inputs.union) if t in set(p.inputs.dicts[0])], lists)
        assert len(p.slots) > len(lists) and p.inputs.union[-1] not in p.inputs.dicts[0]
    assert sk.plan("select_aligned_all", shape).store[0][1] is None
    p = sk.plan("merge_small", shape)
    assert sum(len(d) for d in p.inputs.dicts) <= sk.SMALL_MERGE_TERMS and p.inputs.removed.size <= 4096
    assert sum(len(l) for s in p.inputs.segs for l in s) <= sk.SMALL_MERGE_POSTINGS
    assert all(len(l) for l in p.slots) and len(p.slots) == len(p.inputs.dicts[0]) - (1 if p.inputs.dropped else 0)
    assert shape == "crowd" or any(len(l) > 256 for l in p.slots)      # (the crowd's one long list is beyond the small merge)
    p = sk.plan("concat", shape)
    parts = p.inputs.parts
    assert len(parts) == 4 and len(parts[1]) == 0 and len(parts[2]) == 3 and all(len(l) == 0 for l in parts[2])
    assert all(sum(len(l) for l in parts[i]) > 0 for i in (0, 3))
    p = sk.plan("big", shape)
    assert len(p.slots) == 65537 and same(p.slots[:len(lists)], lists) and all(len(l) == 0 for l in p.slots[len(lists):])


@pytest.mark.parametrize("kind", list(sk.KINDS))
def test_the_readers_questions_are_not_trivial(kind):
    """What tests/test_gpu_segment_kinds.py asks of every kind has an answer worth comparing."""
    p, q = sk.plan(kind, sk.READER_SHAPE), sk.queries(kind)
    s = p.slots
    assert 0 < q.union_tomb.size < q.union.size
    assert (max(int(l[-1]) for l in s if len(l)) - min(int(l[0]) for l in s if len(l))) > 4 * 2048                # several windows
    assert 0 < q.counts.sum() < q.lens.sum() and np.any(~np.isin(q.dset, q.all))
    assert all(b > a for a, b in q.groups) and q.groups[0][1] <= q.groups[1][0] and q.groups[1][1] <= q.groups[2][0]
    assert 0 < q.atleast2.size < q.union.size and q.top_scores[0] >= 2 and q.top_ids.size == 10
    assert sk.nblk(s[q.pair[1]]) >= 2 and sk.nblk(s[q.pair[0]]) >= 2 and 0 < q.pair_and.size < len(s[q.pair[0]])
    if kind != "merge_small":                             # (whose limits leave the 16384-posting list out)
        assert len(s[q.pair[1]]) > 8192
        assert "tomb" in kind or (len(s[q.pair[0]]), len(s[q.pair[1]])) == (513, 16384)      # (tombstones take some of their docs)
    assert q.miss is not None and q.touch is not None
    r, e = q.touch
    assert np.intersect1d(s[r], s[e]).tolist() == [s[r][-1]] and s[e][0] == s[r][-1]
    r, e = q.miss
    assert s[e][0] > s[r][-1]
    assert any(len(m) > len(a) > 0 for m, a in zip(q.merged, s))
    # ---- what tests/test_gpu_segment_kinds_readers.py asks: the size classes of the one-workgroup forms, rows worth explaining
    total = lambda slots: (sum(len(s[i]) for i in slots), sum(sk.nblk(s[i]) for i in slots))
    assert len(q.trio) == 3 and len(set(q.trio)) == 3 and set(q.trio) <= set(q.short)
    assert all(0 < len(s[i]) <= 513 for i in q.short) and len(s[q.long]) == max(len(l) for l in s)
    assert 100 <= q.trio_and.size < min(len(s[i]) for i in q.trio) and q.trio_or.size > max(len(s[i]) for i in q.trio)
    post, blocks = total(q.trio)
    assert post <= 2048 and blocks <= 32 and sk.size_class([s[i] for i in q.trio]) == "tiny"                      # the 256-thread form
    post, blocks = total(q.short)
    assert 2048 < post <= 8192 and blocks <= 128 and len(q.short) <= 64                                         # the 1024-thread form
    assert sk.size_class([s[i] for i in q.short]) == "small" and post * len(q.short) <= sk.ONE_LAUNCH_WORK
    fallback = sk.size_class([s[i] for i in q.short + [q.long]]) == "large"
    assert fallback == (len(s[q.long]) > 8192) == (kind != "merge_small")
    assert (sk.size_class([s[q.trio[0]], s[q.long]]) == "large") == fallback and q.trio[0] != q.long
    assert sk.size_class([s[i] for i in q.trio + [q.not_slot]]) == "tiny" and q.not_slot not in q.trio
    bits = np.array([bin(int(w)).count("1") for w in q.explain_masks[:, 0]])
    assert q.explain_masks.shape == (q.page.size, 1) and bits.max() >= 3 and np.any(bits == 0) and np.any(np.diff(q.page.astype(np.int64)) < 0)
    rows = np.flatnonzero(q.page == q.repeated)
    assert rows.size == 3 and bits[rows[0]] > 0 and not bits[rows[1:]].any()
    assert np.unique(q.page).size == q.page.size - 2 and np.any(~np.isin(q.page, q.all))
    assert len(q.explain_groups) == len([l for l in s if len(l)]) + 3 <= 64
    assert 0 < q.short_atleast2.size < sk.union_of([s[i] for i in q.short]).size
    ids, scores, eligible = q.short_top
    assert ids.size == 10 and scores[0] >= 3 and scores[-1] >= 2 and np.all(np.diff(scores.astype(np.int64)) <= 0) and eligible > 2048
    (groups, exclude), answer = q.gq
    assert groups == [[q.trio[0], q.trio[1]], [q.trio[2]]] and exclude == [[q.not_slot]] and 0 < answer.size < len(s[q.trio[2]])
    assert 250 <= len(s[q.not_slot]) <= 300


@pytest.mark.parametrize("kind", list(sk.KINDS))
def test_the_readers_questions_at_the_top_of_the_id_space(kind):
    """... and of the shape `high`: a page with rows to explain and an axis whose last buckets are [2^32 - 2] and [2^32 - 1]."""
    p, q = sk.plan(kind, "high"), sk.queries(kind, "high")
    bits = np.array([bin(int(w)).count("1") for w in q.explain_masks[:, 0]])
    assert bits.max() >= 3 and np.any(bits == 0) and 0xFFFFFFFF in q.page and q.page.size > 20
    rows = np.flatnonzero(q.page == q.repeated)
    assert rows.size == 3 and bits[rows[0]] > 0 and not bits[rows[1:]].any()
    e = q.top_edges
    assert e[-3:] == [sk.TOP - 2, sk.TOP - 1, sk.TOP] and all(a < b for a, b in zip(e, e[1:])) and e[0] == int(q.all[0])
    assert any(len(l) and l[-1] == 0xFFFFFFFF for l in p.slots)


def test_the_pair_shape_has_the_layout_the_dense_family_asks_for():
    s = sk.shape(sk.DENSE_SHAPE)
    n = [len(l) for l in s]
    assert n[0] == 0 and n[-1] == 0 and n[3] == 0 and n[7] == 0                      # empty first, between the long lists, last
    assert 256 < n[1] < 512 and n[5] == 100                                          # a short sparse list in front of the pair, one behind
    assert sk.nblk(s[2]) < sk.nblk(s[6]) < sk.nblk(s[8]) < sk.nblk(s[4])             # B, the third list, A2, A
    assert len(s[4]) == max(n)                                                       # (A is the list the tombstoned merges thin out)
    assert sk.PAIR_DOCS % 65536 == 0 and max(int(l[-1]) for l in s[:7] if len(l)) < sk.PAIR_DOCS and int(s[8][-1]) < 2 * sk.PAIR_DOCS


@pytest.mark.parametrize("kind", list(sk.KINDS))
def test_every_kind_keeps_the_pair_dense(kind):
    """What tests/test_gpu_segment_kinds_dense.py asks of every kind: under the kind's plan the slots of B, A and the third list
    still go to the dense kernels, a form of B and A meets criterion (b), A2's does not."""
    p = sk.plan(kind, sk.DENSE_SHAPE)
    if kind in sk.DENSE_EXEMPT:                                                      # no list of 1024 blocks fits the small merge
        assert sk.SMALL_MERGE_POSTINGS < sk.DENSE_MIN_BLOCKS * sk.BLOCK and max(sk.nblk(l) for l in p.slots) < sk.DENSE_MIN_BLOCKS
        return
    q = sk.dense_queries(kind)
    s = p.slots
    assert q.b < q.a < q.third < q.a2 and q.crit == (q.third, q.a2)
    for l in (q.B, q.A, q.T):                                                        # the chooser, whichever of them has the fewest blocks
        assert sk.nblk(l) >= sk.DENSE_MIN_BLOCKS and 0 < sk.docs_per_block(l) <= sk.DENSE_MAX_DOCS_PER_BLOCK
    assert sk.nblk(q.B) < sk.nblk(q.A) and sk.nblk(q.B) <= sk.nblk(q.T) < sk.nblk(q.A2)      # the roles: B and the third list pace
    for l in (q.B, q.A):
        assert 2 * sk.form_bytes(l) <= sk.payload_bytes(l)                           # criterion (b) holds ...
    assert 2 * sk.form_bytes(q.A2) > sk.payload_bytes(q.A2)                          # ... and fails: no form
    assert abs(sk.form_bytes(q.A2) / sk.payload_bytes(q.A2) - 5 / 8) < 0.05
    own = int(q.A[-1]) - int(q.A[0]) + 1                                             # the streaming OR: A paces, B lies inside its reach
    assert max(int(q.A[-1]), int(q.B[-1])) - min(int(q.A[0]), int(q.B[0])) + 1 <= own + own // 4 + 65536
    hits = np.intersect1d(q.B, q.A)
    assert 1000 < np.setdiff1d(hits, q.removed).size < hits.size and 1000 < np.intersect1d(q.T, q.A2).size
    assert all(len(s[i]) == 0 or i in (q.third, q.a2) or len(s[i]) <= 400 for i in q.others)
    assert any(len(s[i]) == 0 for i in range(q.b + 1, q.a))                          # an empty slot between B and A: it shares A's block number
    assert len(s[0]) == 0 and len(s[-1]) == 0
    if p.is_view:
        assert (q.parent[q.b], q.parent[q.a]) != (q.b, q.a)                          # the parent numbers the lists differently
    else:
        assert all(q.parent[i] == i for i in (q.b, q.a, q.third, q.a2))
        assert q.last_non_empty_of_store                                             # A2's one-past-last skip entry is the store's sentinel
