import numpy as np
import pytest


@pytest.fixture(scope="module")
def ctx():
    from inverted_index_2_amd import Context
    c = Context(0)
    yield c
    c.close()


class path_delta:
    """with path_delta(ctx) as d: ...  - afterwards d holds what the calls inside launched: {path name: count} of the kernel
    paths whose counters moved (Context.paths())."""

    def __init__(self, ctx):
        self.ctx, self.d = ctx, {}

    def __enter__(self):
        self.before = self.ctx.paths()
        return self.d

    def __exit__(self, *exc):
        after = self.ctx.paths()
        self.d.update({k: after[k] - self.before[k] for k in after if after[k] != self.before[k]})


# ---- one case of a path table (tests/path_cases.py: Case, Layout) on the device ---------------------------------------------
SENTINEL = 0xDEADBEEF


def _delta(before, after):
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def call_case(c, case, segs, lay, tomb, want):
    """One call of the case; returns its results, one array per query."""
    kind, *args = case.call
    total = int(sum(w.size for w in want))
    # (the capacity is part of the choice - the paths that may write part of a result want one that surely fits, a union over
    # several windows counts first below 256 ids per block: every block of the case's lists fits unless the case says "exact")
    cap = total if case.cap == "exact" else 256 * int(sum((l.size + 255) // 256 for s in lay.segments for l in s)) + 64
    out = c.empty(cap + 64).upload(np.full(cap + 64, SENTINEL, np.uint32))
    out.count = cap                                       # (what the entry points take as the capacity)
    R = lambda rs: [(segs[s], a, b) for s, a, b in lay.ranges(rs)]
    off = None
    if kind == "intersect":
        _, n = c.intersect([(segs[s], i) for s, i in lay.pairs(args[0])], tomb=tomb, out=out)
    elif kind == "union":
        _, n = c.union([(segs[s], i) for s, i in lay.pairs(args[0])], tomb=tomb, out=out)
    elif kind == "union_ranges":
        _, n = c.union_ranges(R(args[0]), tomb=tomb, out=out)
    elif kind == "intersect_ranges":
        _, n = c.intersect_ranges([R(g) for g in args[0]], tomb=tomb, out=out)
    elif kind == "andnot":
        _, n = c.andnot_ranges([R(g) for g in args[0]], [R(g) for g in args[1]], tomb=tomb, out=out)
    elif kind == "batch":
        _, off = c.query_batch([(op, R(rs)) for op, rs in args[0]], tomb=tomb, out=out)
    else:
        _, off = c.query_batch_groups([([R(g) for g in groups], [R(g) for g in exclude]) for groups, exclude in args[0]], tomb=tomb, out=out)
    if off is None:
        off = np.array([0, n], np.uint64)
    out.count = cap + 64
    got = out.download()
    assert np.all(got[int(off[-1]):] == SENTINEL), "ids written behind the result"
    return [got[int(a):int(b)] for a, b in zip(off[:-1], off[1:])], off


def case_capacity(case, lay):
    """The generous capacity call_case gives a case that does not ask for an exact one: 256 ids per block of its lists, and 64."""
    return 256 * int(sum((l.size + 255) // 256 for s in lay.segments for l in s)) + 64


def raw_call_case(c, case, segs, lay, out, cap, tomb=None):
    """One call of the case straight through the C ABI, with `cap` as the capacity whatever `out` holds: (return code, *count - a
    batch's out_off[-1] -, out_off).  *count and out_off start at zero, so what comes back is what the library wrote."""
    import ctypes as C

    from inverted_index_2_amd import _lib
    from inverted_index_2_amd.engine import pack_andnot, pack_batch, pack_group_batch
    kind, *args = case.call
    lib, t = c.lib, (tomb.h if tomb else None)
    R = lambda rs: [(segs[s], a, b) for s, a, b in lay.ranges(rs)]
    handles = lambda ss: (C.c_void_p * max(len(ss), 1))(*[s.h for s in ss])
    u64 = lambda a: a.ctypes.data_as(_lib.u64p)
    cnt = C.c_uint64(0)
    if kind in ("intersect", "union"):
        sa, idx = c._listargs([(segs[s], i) for s, i in lay.pairs(args[0])])
        fn = lib.ii2_intersect if kind == "intersect" else lib.ii2_union
        rc = fn(c.h, len(args[0]), sa, idx, t, out.data_ptr(), cap, C.byref(cnt))
    elif kind == "union_ranges":
        gf, _, gs, first, end = pack_andnot([R(args[0])], [])
        rc = lib.ii2_union_ranges(c.h, len(gs), handles(gs), u64(first), u64(end), t, out.data_ptr(), cap, C.byref(cnt))
    elif kind in ("intersect_ranges", "andnot"):
        groups, exclude = [R(g) for g in args[0]], [R(g) for g in args[1]] if kind == "andnot" else []
        gf, gn, gs, first, end = pack_andnot(groups, exclude)
        if kind == "andnot":
            rc = lib.ii2_andnot_ranges(c.h, len(gn), u64(gf), gn.ctypes.data_as(_lib.u8p), handles(gs), u64(first), u64(end), t, out.data_ptr(), cap,
                                       C.byref(cnt))
        else:
            rc = lib.ii2_intersect_ranges(c.h, len(gn), u64(gf), handles(gs), u64(first), u64(end), t, out.data_ptr(), cap, C.byref(cnt))
    elif kind == "batch":
        op, qf, qs, first, end = pack_batch([(o, R(rs)) for o, rs in args[0]])
        off = np.zeros(len(args[0]) + 1, np.uint64)
        rc = lib.ii2_query_batch(c.h, len(args[0]), op.ctypes.data_as(_lib.u8p), u64(qf), handles(qs), u64(first), u64(end), t, out.data_ptr(), cap, u64(off))
        return rc, int(off[-1]), off
    elif kind == "gbatch":
        qf, gf, gn, qs, first, end = pack_group_batch([([R(g) for g in groups], [R(g) for g in exclude]) for groups, exclude in args[0]])
        off = np.zeros(len(args[0]) + 1, np.uint64)
        rc = lib.ii2_query_batch_groups(c.h, len(args[0]), u64(qf), u64(gf), gn.ctypes.data_as(_lib.u8p), handles(qs), u64(first), u64(end), t,
                                        out.data_ptr(), cap, u64(off))
        return rc, int(off[-1]), off
    else:
        raise ValueError(kind)
    return rc, cnt.value, np.array([0, cnt.value], np.uint64)


def run_path_case(ctx, case, layout, defaults):
    """The case's call with its lists laid out as `layout` says: the exact delta of Context.paths() it must show and the plain
    numpy reference bit for bit; defaults: the value every option the case sets goes back to."""
    from tests import path_cases as pc
    lists = case.lists()
    lay = pc.Layout(layout, lists)
    removed = pc.removed_ids(case, lists) if case.tomb else None
    want = pc.reference(case, lists, removed)
    segs = [ctx.encode(*lay.flat(s)) for s in range(len(lay.segments))]
    assert [s.info.n_lists for s in segs] == lay.n_lists
    tomb = ctx.tombstones(removed) if case.tomb else None
    try:
        for name, value in case.options.items():
            ctx.set_option(name, value)
        for repeat in (False, True) if layout == "big" else (False,):
            before = ctx.paths()
            got, off = call_case(ctx, case, segs, lay, tomb, want)
            delta = _delta(before, ctx.paths())
            print(case.name, layout, "repeat" if repeat else "first", delta)
            assert delta == case.expect_in(layout, repeat)
            assert list(off) == list(np.cumsum([0] + [w.size for w in want]))              # (a batch's out_off; else [0, count])
            for q, (g, w) in enumerate(zip(got, want)):
                assert g.dtype == np.uint32 and np.array_equal(g.astype(np.uint64), w), q
    finally:
        for name in case.options:
            ctx.set_option(name, defaults[name])
        for s in segs:
            s.free()
        if tomb is not None:
            tomb.free()


def blocks_of(l):
    """DV1 blocks of a list of ids (256 postings each, the last one may be short)."""
    return (len(l) + 255) // 256


def one_block_lists_past_a_wave(rng, universe, reach=6000):
    """Lists for the walk of a wave over SEVERAL query blocks (cr_walk.h), which a call reaches only beyond 32 waves per CU of one
    block each: two segments of one- to three-posting lists - every list owns one block, its ids within `reach` docs of each
    other except in every 97th list, which spreads over the universe - named as six ranges of odd block counts, the segments in
    turn.  Returns ([lists of A, lists of B], [(segment, first list, end list), ...], blocks a wave walks); asserts that the
    ranges' blocks are more than two per wave and that range ends fall inside a wave's run."""
    import torch
    waves = 32 * torch.cuda.get_device_properties(0).multi_processor_count
    sizes = (waves + 21, waves + 19)
    segments = []
    for n in sizes:
        first = rng.integers(0, universe - 3 * reach, n)
        gaps = rng.integers(1, reach, (n, 2))
        wide = np.arange(n) % 97 == 0
        first[wide] = rng.integers(0, universe // 8, int(wide.sum()))
        gaps[wide] = rng.integers(universe // 4, universe // 3, (int(wide.sum()), 2))
        ids = np.cumsum(np.column_stack([first, gaps]), axis=1)
        segments.append([ids[j, :k].astype(np.uint32) for j, k in enumerate(rng.integers(1, 4, n))])
    ranges = [(0, 0, 301), (1, 0, 77), (0, 301, 1002), (1, 77, 578), (0, 1002, sizes[0]), (1, 578, sizes[1])]
    n_blocks = sum(b - a for _, a, b in ranges)
    per_wave = -(-n_blocks // waves)
    assert n_blocks > 2 * waves and per_wave >= 3 and all((b - a) % 2 == 1 for _, a, b in ranges)
    ends = np.cumsum([b - a for _, a, b in ranges])[:-1]
    assert np.count_nonzero(ends % per_wave) >= 3, (ends, per_wave)
    assert sum(l.size for lists in segments for l in lists) < 50_000
    return segments, ranges, per_wave


def sorted_unique(rng, n, universe):
    if n == 0:
        return np.empty(0, np.uint32)
    if n > universe // 2:
        v = np.flatnonzero(rng.random(universe) < n / universe)
    else:
        v = np.unique(rng.integers(0, universe, int(n * 1.1) + 8, dtype=np.int64))[:n]
    return v.astype(np.uint32)
