"""The table of segment kinds: one entry per way of making a segment, each a function from a shape (a list of posting lists) to
what the library must be given and to the lists every slot of the resulting segment must hold.

Every query and merge kernel reads, next to a segment's DV1 bytes, arrays the library derives when the segment is made - cnt,
last_doc, blk_list, the host span mirror, a view's window (include/ii2.h: ii2_seg_export_meta).  They come from another piece of
code for every maker:

  encode_host, encode_device, build_pairs    k_enc_blocks / k_enc_list_meta                     csrc/api.cpp: ii2_seg_encode_dev_unlocked
  import_oracle                              k_list_last_doc over the imported bytes            csrc/codec.hip
  merge_stream, merge_tomb_stream            k_enc_stream (option encode.stream = 1)            csrc/encode_stream.hip
  merge_two_pass, merge_tomb_two_pass        the two-pass encoder behind a merge (= 0)          csrc/api.cpp
  select                                     host block table + k_list_last_doc + the window    csrc/api.cpp: ii2_seg_select
  select_aligned, select_aligned_all         k_align_view / k_align_blk_list, no host mirror    csrc/align.hip
  merge_small                                its own kernel and its own spans                   csrc/merge_small.hip
  concat, allgather                          k_seg_rebase / k_seg_close                         csrc/codec.hip, csrc/comm.cpp
  big                                        65537 lists: no span mirror                        csrc/internal.h: SPAN_MIRROR_MAX

A kind is a pair: plan(shape) - pure numpy, no GPU - says what goes in (`inputs`), the lists each slot of the result holds
(`slots`) and, in store order, every list of the store the result numbers its blocks in together with the slot that owns it
(`store`: [(ids, slot or None)]; a whole segment's store is its slots); make(ctx, plan) calls the library.  reference(plan) is
the derived arrays in plain numpy over those lists - it knows nothing of what the library answers.
tests/test_segment_kinds_cpu.py checks the table itself, tests/test_gpu_segment_meta.py pins Segment.meta() to the reference for
every (kind, shape), tests/test_gpu_segment_kinds.py and tests/test_gpu_segment_kinds_readers.py run the readers of the derived
arrays on every kind.

The shapes are the smallest at which each array can go wrong (under 60 k postings each, doc spans of 2^19 so that a union in
windows of 2048 docs stays at 256 windows): see SHAPES.  One shape is large, `pair` (~ 1.5 M postings): the dense two-list AND
takes lists of at least 1024 blocks, and tests/test_gpu_segment_kinds_dense.py runs that family of kernels (tests/dense_edge_cases.py)
on what every maker but merge_small, whose limit is 8192 postings, derives for such lists (dense_queries)."""
import functools
from types import SimpleNamespace

import numpy as np

BLOCK = 256
NONE = 0xFFFFFFFF
SPAN_MIRROR_MAX = 1 << 16
BIG_LISTS = SPAN_MIRROR_MAX + 1
SMALL_MERGE_TERMS, SMALL_MERGE_POSTINGS = 512, 8192          # include/ii2.h: II2_SMALL_MERGE_*
SPAN = 1 << 19                                               # docs a shape spreads over
PAIR_DOCS = 14 << 16                                         # ... and of the dense lists of `pair`: the smallest multiple of 65536 at which every plan keeps them dense (13: the tombstoned merges leave 969 blocks)
E = np.empty(0, np.uint32)


def u32(a):
    return np.asarray(a, np.uint32)


def draw(rng, n, lo, hi):
    """n ascending, distinct ids in [lo, hi]."""
    assert hi - lo + 1 >= n
    return (np.sort(rng.choice(hi - lo + 1, n, replace=False)).astype(np.int64) + lo).astype(np.uint32)


# ---- shapes ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shape(name):
    rng = np.random.default_rng({"lengths": 1, "high": 2, "crowd": 3, "pair": 4}[name])
    if name == "pair":
        # what the dense two-list AND family needs of a maker (dense_queries): a shorter dense list B and a longer one A - under
        # every kind's plan both keep >= 1024 blocks at <= 1100 docs per block and a dense form of at most half their payload -,
        # a third dense list, and a list A2 at one posting in five docs whose form would be 5 / 8 of its payload (no form);
        # empty lists first, between the long lists and last, a short sparse list in front of the pair and one behind it; A2 is
        # the last non-empty list: the skip entry behind its last block is a whole segment's sentinel
        bern = lambda p, hi: np.flatnonzero(rng.random(hi) < p).astype(np.uint32)
        B, A, third = bern(1 / 3, PAIR_DOCS), bern(1 / 2, PAIR_DOCS), bern(0.36, PAIR_DOCS)
        return [E, draw(rng, 400, 1, PAIR_DOCS - 1), B, E, A, draw(rng, 100, 1, PAIR_DOCS - 1), third, E, bern(1 / 5, 2 * PAIR_DOCS), E]
    if name == "lengths":
        # every block-count edge; [0], whose last_doc is an empty list's; a list from 0; runs of empty lists first, inside, last;
        # a(255) / b(256) / c(257): b starts at a's last doc (their spans touch by one doc), c lies wholly behind b
        base = 4096
        a = draw(rng, 255, base + 1000, base + 9000)
        b = np.concatenate([[a[-1]], draw(rng, 255, int(a[-1]) + 1, int(a[-1]) + 9000)]).astype(np.uint32)
        c = draw(rng, 257, int(b[-1]) + 10, int(b[-1]) + 9000)
        l513 = draw(rng, 513, 1, SPAN - 1)

        def mixed(n, part):                                # n ids, `part` among them (the multi-block lists share docs)
            rest = np.setdiff1d(draw(rng, n, 1, SPAN - 1), part)
            return np.union1d(part, rng.choice(rest, n - len(part), replace=False)).astype(np.uint32)
        return [E, u32([0]), a, b, c, E, E, mixed(511, l513[::4]), mixed(512, l513[::2]), l513,
                np.concatenate([[0], draw(rng, 299, 1, 40000)]).astype(np.uint32), draw(rng, 16384, 1, SPAN - 1), E, u32([SPAN - 1]), E]
    if name == "high":
        # the top of the id space: a list that ends at 0xFFFFFFFF, the list [0xFFFFFFFF], a last block of one posting
        top, lo = 0xFFFFFFFF, 0xFFFFFFFF - (1 << 18) + 1
        return [draw(rng, 3, lo, top - 1), E, draw(rng, 257, lo, top - 1), u32([top]),
                np.concatenate([draw(rng, 599, lo, top - 1), [top]]).astype(np.uint32), E]
    # crowd: 3000 lists of 0 .. 3 postings around one list of 20000 - lists start inside the one-pass encoder's 1024-position
    # partitions, one list crosses several of its workgroups, more than 64 lists start inside one tile
    lens = rng.integers(0, 4, 3001)
    lens[:3] = 0
    lens[-2:] = 0
    lens[1500] = 20000
    return [draw(rng, int(n), 0, SPAN - 1) for n in lens]


SHAPES = ("lengths", "high", "crowd", "pair")
READER_SHAPE = "lengths"          # the shape the readers run on: it holds the 513- and the 16384-posting list and the a / b / c lists
DENSE_SHAPE = "pair"              # the shape the dense two-list AND family runs on (dense_queries)


# ---- the reference: the derived arrays from the lists alone ----------------------------------------------------------------
def nblk(l):
    return (len(l) + BLOCK - 1) // BLOCK


def payload_bytes(l):
    """Bytes of a list's DV1 payload: one LEB128 varint per gap, none for the first posting of a block."""
    l = np.asarray(l, np.int64)
    if l.size < 2:
        return 0
    g = np.diff(l) % (1 << 32)
    g = g[(np.arange(1, l.size) % BLOCK) != 0]
    return int((1 + (g >= 1 << 7) + (g >= 1 << 14) + (g >= 1 << 21) + (g >= 1 << 28)).sum())


def reference(plan):
    """cnt, last_doc, spans per slot; blk_list over the blocks of the store (NONE where no slot owns the block, and in the entry
    past the last block); the store's totals; the window of the store that the slots' lists cover."""
    slots, store = plan.slots, plan.store
    n = len(slots)
    r = SimpleNamespace()
    r.cnt = np.array([len(l) for l in slots], np.uint32)
    r.last_doc = np.array([l[-1] if len(l) else 0 for l in slots], np.uint32)
    r.spans = np.zeros((n, 3), np.uint32)
    for i, l in enumerate(slots):
        if len(l):
            r.spans[i] = (l[0], l[BLOCK * (nblk(l) - 1)], l[-1])
    owners = [np.full(nblk(l), NONE if s is None else s, np.uint32) for l, s in store]
    r.blk_list = np.concatenate(owners + [np.array([NONE], np.uint32)])
    r.n_blocks = int(r.blk_list.size - 1)
    r.n_bytes = sum(payload_bytes(l) for l, _ in store)
    r.n_lists = n
    r.sum_cnt = int(r.cnt.sum())
    r.store_postings = sum(len(l) for l, _ in store)
    owned = [(nblk(l), payload_bytes(l)) for l, s in store if s is not None]
    r.win_blocks, r.win_bytes = sum(b for b, _ in owned), sum(q for _, q in owned)
    return r


def csr(lists):
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.uint64)
    vals = np.concatenate([u32(l) for l in lists] + [E]).astype(np.uint32)
    return off, vals


def whole(slots, **inputs):
    slots = [u32(l) for l in slots]
    return SimpleNamespace(slots=slots, store=[(l, i) for i, l in enumerate(slots)], inputs=SimpleNamespace(**inputs))


def halves(lists):
    """Two segments whose slot-wise union is `lists`: every third posting in both, the others in one of them."""
    a = [l[np.arange(len(l)) % 3 != 1] for l in lists]
    b = [l[np.arange(len(l)) % 3 != 2] for l in lists]
    return a, b


# ---- the kinds: plan(shape), make(ctx, plan) -> (segment, [objects the segment needs alive]) ------------------------------------
def plan_plain(lists):
    return whole(lists)


def make_encode_host(ctx, p):
    return ctx.encode(*csr(p.slots)), []


def make_encode_device(ctx, p):
    from inverted_index_2_amd._lib import II2_DEVICE
    off, vals = csr(p.slots)
    d_off = ctx.empty(off.size, np.uint64).upload(off)
    d_vals = ctx.empty(max(vals.size, 1)).upload(vals if vals.size else np.zeros(1, np.uint32))
    seg = ctx.encode(d_off, d_vals, where=II2_DEVICE)
    d_off.free()
    d_vals.free()
    return seg, []


def plan_build_pairs(lists):
    """(list, value) pairs in shuffled order, every seventh one twice."""
    ids = np.concatenate([np.full(len(l), i, np.uint32) for i, l in enumerate(lists)] + [E]).astype(np.uint32)
    vals = csr(lists)[1]
    rep = np.arange(0, ids.size, 7)
    ids, vals = np.concatenate([ids, ids[rep]]), np.concatenate([vals, vals[rep]])
    order = np.random.default_rng(5).permutation(ids.size)
    return whole(lists, list_ids=ids[order], values=vals[order])


def make_build_pairs(ctx, p):
    seg, st = ctx.build_segment(p.inputs.list_ids, p.inputs.values, len(p.slots))
    assert st.n_postings == sum(len(l) for l in p.slots)
    return seg, []


def make_import_oracle(ctx, p):
    from oracle import oracle as orc
    off, vals = csr(p.slots)
    blk, skip, payload = orc.dv1_encode(off, vals)
    return ctx.import_dv1(vals.size, blk, skip, payload), []


def plan_merge(lists):
    a, b = halves([u32(l) for l in lists])
    return whole(lists, segs=[a, b], removed=None)


def plan_merge_tomb(lists):
    """Three extra lists - first, in the middle, last - whose every doc is removed, and every fourth doc of the longest list;
    the first and last doc of every other list stay (the readers look for lists whose spans touch)."""
    lists = [u32(l) for l in lists]
    lo = min(int(l[0]) for l in lists if len(l))
    hi = max(int(l[-1]) for l in lists if len(l))
    rng = np.random.default_rng(6)
    extra = [draw(rng, n, lo, hi) for n in (2, 300, 1)]
    h = len(lists) // 2
    full = [extra[0]] + lists[:h] + [extra[1]] + lists[h:] + [extra[2]]
    longest = max(lists, key=len)
    ends = np.unique(np.concatenate([[l[0], l[-1]] for l in lists if len(l)]))
    removed = np.setdiff1d(np.union1d(np.concatenate(extra), longest[1:-1:4]), ends).astype(np.uint32)
    extra_slots = (0, h + 1, len(full) - 1)
    for s in extra_slots:                                   # (an extra doc that is some list's end stays: draw it out of the list)
        full[s] = np.intersect1d(full[s], removed).astype(np.uint32)
    slots = [np.setdiff1d(l, removed).astype(np.uint32) for l in full]
    a, b = halves(full)
    p = whole(slots, segs=[a, b], removed=removed, emptied=extra_slots)
    return p


def _make_merge(stream):
    def make(ctx, p):
        segs = [ctx.encode(*csr(s)) for s in p.inputs.segs]
        tomb = ctx.tombstones(p.inputs.removed) if p.inputs.removed is not None else None
        try:
            ctx.set_option("encode.stream", stream)
            out, st = ctx.merge_to_segment(segs, tomb)
        finally:
            ctx.set_option("encode.stream", 1)
            for s in segs:
                s.free()
            if tomb is not None:
                tomb.free()
        assert st.n_out == sum(len(l) for l in p.slots)
        return out, []
    return make


JUNK_BEFORE = [np.arange(7, 7 + 3 * 300, 3, dtype=np.uint32), E]      # lists of the store in front of a view's window ...
JUNK_AFTER = [u32([1, 5, 9, 4000, 70000])]                            # ... and behind it


def plan_select(lists):
    """A view of the lists in the middle of a store: slots -1 first, after every second list, and last."""
    lists = [u32(l) for l in lists]
    src, slots = [-1, -1], [E, E]
    for i, l in enumerate(lists):
        src.append(len(JUNK_BEFORE) + i)
        slots.append(l)
        if i % 2 == 1:
            src.append(-1)
            slots.append(E)
    src.append(-1)
    slots.append(E)
    store_lists = JUNK_BEFORE + lists + JUNK_AFTER
    owner = {j: s for s, j in enumerate(src) if j >= 0}
    return SimpleNamespace(slots=slots, store=[(l, owner.get(j)) for j, l in enumerate(store_lists)],
                           inputs=SimpleNamespace(store=store_lists, src_list=np.array(src, np.int64)))


def make_select(ctx, p):
    store = ctx.encode(*csr(p.inputs.store))
    return ctx.select(store, p.inputs.src_list), [store]


def term(i):
    return b"t%06d" % i


def plan_aligned(lists, first_list):
    """The segment's dictionary names its lists [first_list, first_list + n) with the odd terms; a second dictionary holds every
    fourth even term - one in front of all (slot 0 is a term the segment lacks), some in between, one behind."""
    lists = [u32(l) for l in lists]
    n = len(lists)
    d0 = [term(2 * i + 1) for i in range(n)]
    d1 = [term(4 * j) for j in range(n // 2 + 2)]
    union = sorted(set(d0) | set(d1))
    at = {t: i for i, t in enumerate(d0)}
    slots = [lists[at[t]] if t in at else E for t in union]
    assert union[0] not in at
    store_lists = (JUNK_BEFORE if first_list else []) + lists + (JUNK_AFTER if first_list else [])
    owner = {first_list + at[t]: u for u, t in enumerate(union) if t in at}
    return SimpleNamespace(slots=slots, store=[(l, owner.get(j)) for j, l in enumerate(store_lists)],
                           inputs=SimpleNamespace(store=store_lists, dicts=[d0, d1], first_list=first_list, union=union))


def make_select_aligned(ctx, p):
    store = ctx.encode(*csr(p.inputs.store))
    al = ctx.align_terms(p.inputs.dicts)
    assert al.n_union == len(p.inputs.union)
    view = ctx.select_aligned(store, al, 0, first_list=p.inputs.first_list)
    al.free()
    return view, [store]


def make_select_aligned_all(ctx, p):
    store = ctx.encode(*csr(p.inputs.store))
    other = ctx.encode_lists([u32([i]) for i in range(len(p.inputs.dicts[1]))])
    al = ctx.align_terms(p.inputs.dicts)
    views = ctx.select_aligned_all([store, other], al, first_list=[p.inputs.first_list, 0])
    al.free()
    views[1].free()
    return views[0], [store, other]


def plan_merge_small(lists):
    """ii2_merge_small takes 512 terms and 8192 postings in all and drops emptied terms: the non-empty lists of the shape, in
    order, while 250 lists (two dictionaries of them) / 5000 postings are not exceeded (their two halves overlap by a third); the last kept list, when it is
    short, has every doc removed and leaves with its term."""
    kept, total = [], 0
    for l in lists:
        if len(l) and len(kept) < 250 and total + len(l) <= 5000:
            kept.append(u32(l))
            total += len(l)
    removed = max(kept, key=len)[1:-1:5]
    gone = len(kept) > 2 and len(kept[-1]) <= 300
    if gone:
        removed = np.union1d(removed, kept[-1])
    removed = removed.astype(np.uint32)
    a, b = halves(kept)
    terms = [term(i) for i in range(len(kept))]
    has_b = [i for i, l in enumerate(b) if len(l)]
    slots = [np.setdiff1d(l, removed).astype(np.uint32) for l in kept]
    slots = [l for l in slots if len(l)]
    return whole(slots, segs=[a, [b[i] for i in has_b]], dicts=[terms, [terms[i] for i in has_b]], removed=removed, dropped=gone)


def make_merge_small(ctx, p):
    segs = [ctx.encode(*csr(s)) for s in p.inputs.segs]
    out, terms, st = ctx.merge_small(segs, p.inputs.dicts, p.inputs.removed)
    for s in segs:
        s.free()
    assert len(terms) == len(p.slots) and st.n_out == sum(len(l) for l in p.slots)
    return out, []


def plan_concat(lists):
    """Four parts: the first half of the lists, a segment without lists, a segment of three empty lists, the second half."""
    lists = [u32(l) for l in lists]
    h = len(lists) // 2
    parts = [lists[:h], [], [E, E, E], lists[h:]]
    return whole([l for part in parts for l in part], parts=parts)


def make_concat(ctx, p):
    segs = [ctx.encode(*csr(part)) for part in p.inputs.parts]
    out = ctx.seg_concat(segs)
    for s in segs:
        s.free()
    return out, []


def make_allgather(ctx, p):
    seg = ctx.encode(*csr(p.slots))
    out = ctx.seg_allgather(seg)
    seg.free()
    return out, []


def plan_big(lists):
    lists = [u32(l) for l in lists]
    return whole(lists + [E] * (BIG_LISTS - len(lists)))


# name -> (plan, make, is_view, aligned)
KINDS = {
    "encode_host": (plan_plain, make_encode_host, False, False),
    "encode_device": (plan_plain, make_encode_device, False, False),
    "build_pairs": (plan_build_pairs, make_build_pairs, False, False),
    "import_oracle": (plan_plain, make_import_oracle, False, False),
    "merge_stream": (plan_merge, _make_merge(1), False, False),
    "merge_two_pass": (plan_merge, _make_merge(0), False, False),
    "merge_tomb_stream": (plan_merge_tomb, _make_merge(1), False, False),
    "merge_tomb_two_pass": (plan_merge_tomb, _make_merge(0), False, False),
    "select": (plan_select, make_select, True, False),
    "select_aligned": (lambda lists: plan_aligned(lists, 0), make_select_aligned, True, True),
    "select_aligned_all": (lambda lists: plan_aligned(lists, len(JUNK_BEFORE)), make_select_aligned_all, True, True),
    "merge_small": (plan_merge_small, make_merge_small, False, False),
    "concat": (plan_concat, make_concat, False, False),
    "allgather": (plan_plain, make_allgather, False, False),
    "big": (plan_big, make_encode_host, False, False),
}


@functools.lru_cache(maxsize=None)
def plan(kind, shape_name):
    p = KINDS[kind][0](shape(shape_name))
    p.kind, p.shape, p.is_view, p.aligned = kind, shape_name, KINDS[kind][2], KINDS[kind][3]
    # the span mirror: every segment of up to 65536 lists that is finished on the host; the aligned views are adopted as the
    # device built them
    p.mirrored = not p.aligned and len(p.slots) <= SPAN_MIRROR_MAX
    return p


def make(ctx, p):
    return KINDS[p.kind][1](ctx, p)


CASES = [(k, s) for k in KINDS for s in SHAPES]


# ---- what the readers ask of a kind, and the answers in plain numpy ------------------------------------------------------------
def union_of(lists):
    return np.unique(np.concatenate([u32(l) for l in lists] + [E])).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def queries(kind, shape_name=READER_SHAPE):
    """The fixed handful of calls of tests/test_gpu_segment_kinds.py for one kind, by slot numbers, with their results:
      removed / dset      every fifth doc of all the lists' union is removed; the doc set of the facet count is every third doc
                          of the union and, next to every seventh, a doc that may lie in no list
      groups              the non-empty slots cut into three runs of consecutive slots (the empty slots between them included)
      pair                the longest list and the longest of the others that holds at most 513 postings: the 16384- and the
                          513-posting list wherever the kind keeps them whole
      miss / touch        (required, excluded) slots of 100 .. 300 postings: the excluded list starts behind the required list's
                          last doc / AT its last doc - their spans share exactly one doc
    and what tests/test_gpu_segment_kinds_readers.py asks: see _later_readers."""
    p = plan(kind, shape_name)
    s = p.slots
    ne = [i for i, l in enumerate(s) if len(l)]
    q = SimpleNamespace()
    q.all = union_of(s)
    q.removed = q.all[::5].copy()
    near = q.all[1::7].astype(np.int64) + 1
    q.dset = np.unique(np.concatenate([q.all[::3].astype(np.int64), near[near < (1 << 32)]])).astype(np.uint32)
    q.union = q.all
    q.union_tomb = np.setdiff1d(q.all, q.removed).astype(np.uint32)
    q.counts = np.array([np.setdiff1d(np.intersect1d(l, q.dset), q.removed).size if len(l) else 0 for l in s], np.uint64)
    q.lens = np.array([len(l) for l in s], np.uint64)
    cut = [0, len(ne) // 3, 2 * len(ne) // 3, len(ne)]
    q.groups = [(ne[cut[g]], ne[cut[g + 1] - 1] + 1) for g in range(3)]
    score = np.zeros(q.all.size, np.int64)
    for a, b in q.groups:
        score += np.isin(q.all, union_of(s[a:b]))
    q.atleast2 = q.all[score >= 2]
    order = np.lexsort((q.all, -score))[:10]
    q.top_ids, q.top_scores = q.all[order], score[order].astype(np.uint32)
    by_len = sorted(ne, key=lambda i: len(s[i]))
    longest = by_len[-1]
    q.pair = (max((i for i in by_len[:-1] if len(s[i]) <= 513), key=lambda i: len(s[i])), longest)
    q.pair_and = np.intersect1d(s[q.pair[0]], s[q.pair[1]]).astype(np.uint32)
    mid = [i for i in ne if 100 <= len(s[i]) <= 300]
    q.miss = next(((r, e) for r in mid for e in mid if s[e][0] > s[r][-1]), None)
    q.touch = next(((r, e) for r in mid for e in mid if r != e and s[e][0] == s[r][-1]), None)
    # the other segment of the merge: slot i holds every third doc of the next slot's list
    q.other = [s[(i + 1) % len(s)][::3] for i in range(len(s))]
    q.merged = [np.union1d(a, b).astype(np.uint32) if len(a) or len(b) else E for a, b in zip(s, q.other)]
    _later_readers(q, s, ne, shape_name)
    return q


# ---- ... and of the readers that came later (tests/test_gpu_segment_kinds_readers.py) -----------------------------------------
TINY_POSTINGS, TINY_BLOCKS = 2048, 32            # csrc/internal.h: BATCH_TINY_* - the 256-thread form of the batch kernels
SMALL_POSTINGS, SMALL_BLOCKS, SMALL_LISTS = 8192, 128, 64      # SMALL_SET_*, MAX_LISTS - one workgroup of 1024 threads
ONE_LAUNCH_WORK = 32768                          # ANDNOT_SMALL_WORK: postings x lists of the one-launch threshold query
TOP = 1 << 32


def size_class(lists):
    """Where lists that are named together run: "tiny" - the 256-thread form -, "small" - one workgroup of 1024 threads - or
    "large" - the fallback; empty lists do not count."""
    lists = [l for l in lists if len(l)]
    post, blocks = sum(len(l) for l in lists), sum(nblk(l) for l in lists)
    if len(lists) > SMALL_LISTS or post > SMALL_POSTINGS or blocks > SMALL_BLOCKS:
        return "large"
    return "tiny" if post <= TINY_POSTINGS and blocks <= TINY_BLOCKS else "small"


def ranked(group_lists, k):
    """(ids, scores, eligible docs): the k docs in the most groups, ties to the lower id"""
    ids = union_of([l for g in group_lists for l in g])
    score = np.zeros(ids.size, np.int64)
    for g in group_lists:
        score += np.isin(ids, union_of(g))
    order = np.lexsort((ids, -score))[:k]
    return ids[order], score[order].astype(np.uint32), int(ids.size)


def _later_readers(q, s, ne, shape_name):
    """What tests/test_gpu_segment_kinds_readers.py asks, by slot numbers, with the answers:
      page                every 37th doc of the lists' union, docs that lie in no list (one below and one above all of them where
                          the id space has room), the first and the last doc of every non-empty slot; shuffled, and the last
                          doc of the longest slot twice more (70 .. 560 ids: the union's size decides)
      explain_groups      (first slot, end slot) per group: every non-empty slot alone, then the three runs of `groups` - a doc of
                          a list sets two bits at least, every list sits in two groups; explain_masks: the rows of `page`
      top_edges           (shape `high`) an axis over the shape's span that ends with the edges 2^32 - 2, 2^32 - 1, 2^32
    and, for the other shapes:
      short / long        the non-empty slots of at most 513 postings / the longest slot
      trio                the three longest slots of `short`, the shortest of them first; trio_and, trio_or
      short_atleast2      the docs in at least two lists of `short`; short_top: ranked(one group per list of `short`, 10)
      not_slot            the longest slot of at most 300 postings (the 300-posting list wherever the kind keeps it whole)
      gq                  ((groups, excluded groups) by slots, the answer): (trio[0] OR trio[1]) AND trio[2], NOT not_slot - the
                          excluded list's span meets the required groups' and, under today's plans, holds none of the answer's docs:
                          it has to be read, and to remove nothing"""
    from tests import explain_cases
    by_len = sorted(ne, key=lambda i: (len(s[i]), i))
    q.long = by_len[-1]
    absent = q.all[1::7].astype(np.int64) + 1
    absent = absent[(absent < TOP) & ~np.isin(absent, q.all)][:24]
    around = [x for x in (int(q.all[0]) - 1, int(q.all[-1]) + 5) if 0 <= x < TOP]
    ends = [x for i in ne for x in (s[i][0], s[i][-1])]
    page = np.unique(np.concatenate([q.all[::37].astype(np.int64), absent, around, ends])).astype(np.uint32)
    page = np.random.default_rng(37).permutation(page)
    q.repeated = s[q.long][-1]
    q.page = np.insert(page, [page.size // 3, page.size - 2], q.repeated).astype(np.uint32)
    q.explain_groups = [(i, i + 1) for i in ne] + list(q.groups)
    q.explain_masks = explain_cases.truth([s[a:b] for a, b in q.explain_groups], q.page)
    if shape_name == "high":
        lo = int(q.all[0])
        q.top_edges = [lo + (TOP - 2 - lo) * b // 20 for b in range(20)] + [TOP - 2, TOP - 1, TOP]
        return
    q.short = [i for i in ne if len(s[i]) <= 513]
    q.trio = [i for i in by_len if i in q.short][-3:]
    t0, t1, t2 = (s[i] for i in q.trio)
    q.trio_and = np.intersect1d(np.intersect1d(t0, t1), t2).astype(np.uint32)
    q.trio_or = union_of([t0, t1, t2])
    in_short = union_of([s[i] for i in q.short])
    n_in = np.zeros(in_short.size, np.int64)
    for i in q.short:
        n_in += np.isin(in_short, s[i])
    q.short_atleast2 = in_short[n_in >= 2]
    q.short_top = ranked([[s[i]] for i in q.short], 10)
    q.not_slot = max((i for i in ne if len(s[i]) <= 300), key=lambda i: (len(s[i]), i))
    answer = np.setdiff1d(np.intersect1d(np.union1d(t0, t1), t2), s[q.not_slot]).astype(np.uint32)
    q.gq = (([[q.trio[0], q.trio[1]], [q.trio[2]]], [[q.not_slot]]), answer)


DENSE_MIN_BLOCKS, DENSE_MAX_DOCS_PER_BLOCK = 1024, 1100.0   # the dense chooser: blocks of the list with the fewest, its docs per block
DENSE_EXEMPT = ("merge_small",)                              # 8192 postings are 32 blocks: no dense list fits that maker


def docs_per_block(l):
    """what the set-op choosers look at: (first doc of the last block - first doc) / (blocks - 1)"""
    return (int(l[BLOCK * (nblk(l) - 1)]) - int(l[0])) / (nblk(l) - 1)


def form_bytes(l):
    """bytes of a list's dense form: one bit per doc from its first doc's 32-doc word to its last doc's"""
    return 4 * (((int(l[-1]) - (int(l[0]) & ~31)) >> 5) + 1)


@functools.lru_cache(maxsize=None)
def dense_queries(kind, shape_name=DENSE_SHAPE):
    """What tests/test_gpu_segment_kinds_dense.py asks of one kind, by slot numbers, with the answers:
      b, a, third         the slots of the main pair (b: fewer blocks) and of the third dense list; B, A, T: their lists
      removed             every fifth doc of the union of all the lists
      crit                (slot of the third list, slot of A2): the pair for criterion (b) - A2, at one posting in five docs, gets
                          no dense form where the option leaves it to the criterion; A2 is the kind's last non-empty slot
      others              every other slot: none of them may ever show a form
      parent              slot -> list number in the store (what a view's parent calls the list); a whole segment's is its own"""
    p = plan(kind, shape_name)
    s = p.slots
    ne = [i for i, l in enumerate(s) if len(l)]
    assert len(ne) == 6, kind                                # sparse, B, A, sparse, third, A2 - in this order under every plan
    q = SimpleNamespace()
    _, q.b, q.a, _, q.third, q.a2 = ne
    q.B, q.A, q.T, q.A2 = s[q.b], s[q.a], s[q.third], s[q.a2]
    q.crit = (q.third, q.a2)
    q.removed = union_of(s)[::5].copy()
    q.others = [i for i in range(len(s)) if i not in (q.b, q.a)]
    q.parent = {slot: j for j, (_, slot) in enumerate(p.store) if slot is not None}
    q.last_non_empty_of_store = max(j for j, (l, _) in enumerate(p.store) if len(l)) == q.parent[q.a2]
    return q
