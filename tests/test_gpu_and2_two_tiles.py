"""The dense-form instance of the one-launch two-list AND with TWO tiles per wave (csrc/intersect_and2.hip k_and2_fused_x2; option
intersect.and2_tiles: 0 auto, 1, 2).  Workgroup g owns B's blocks [128 g, 128 g + 128): tile 0 is the first 64 of them, tile 1 the
other 64, so block b of B falls into tile (b // 64) % 2 of workgroup b // 128.

Every case of tests/dense_form_cases.py runs forced to one tile and to two, as it stands and padded - both lists get the same
64 x 256 docs in front, which moves every block of B from a tile 0 into a tile 1 or back; the numpy tests at the top of this file
(no device) state where the hard rows, the window gap and the wide gap then lie.  Everything is bit-exact against numpy."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd.engine import II2Error
from tests import dense_form_cases as dc
from tests.gpu_util import ctx, path_delta  # noqa: F401

gpu = pytest.mark.gpu
FILL = 0xDEADBEEF
ECAPACITY = -4
TILE_BLOCKS = 16                # blocks of B a wave takes per tile
PAD = dc.WG_BLOCKS * dc.BLOCK   # postings (and docs) in front of a padded list: 64 blocks of B, one tile of a workgroup
FUSED = ({"and.and2_fused": 1}, {"and.and2_fused": 1, "and.and2_split": 1})     # (a look-back wait that ran out repeats the call)


def padded(case):
    """(x, y, removed) with the docs [0, PAD) in front of both lists and everything else PAD further up"""
    x, y, removed = case.data()
    front = np.arange(PAD, dtype=np.uint32)
    up = lambda l: np.concatenate([front, l + np.uint32(PAD)]).astype(np.uint32)
    return up(x), up(y), None if removed is None else (removed + np.uint32(PAD)).astype(np.uint32)


def reference(x, y, removed):
    want = np.intersect1d(x, y, assume_unique=True)
    if removed is not None:
        want = np.setdiff1d(want, removed, assume_unique=True)
    return want.astype(np.uint32)


def tile_of_block(b):
    return (b // dc.WG_BLOCKS) % 2


def tile_of_gap(B, doc):
    """the tile (0 / 1 of its workgroup) whose docs hold the gap of B over `doc`: the one of the posting before the gap (a tile's
    docs reach up to the next tile's first doc)"""
    i = int(np.searchsorted(B, doc))
    return tile_of_block((i - 1) // dc.BLOCK)


def hard_blocks(B):
    """blocks of B the kernel decodes with the whole wave: a multi-byte gap inside, or a short last block"""
    n = dc.blocks(B)
    out = []
    for b in range(n):
        blk = B[b * dc.BLOCK:(b + 1) * dc.BLOCK].astype(np.int64)
        if blk.size < dc.BLOCK or np.any(np.diff(blk) >= 128):
            out.append(b)
    return out


# ---- where the edge cases lie (plain numpy) ---------------------------------------------------------------------------------
def test_the_table_has_an_odd_number_of_tiles():
    x, y, _ = dc.BY_NAME["uniform"].data()
    B, _ = dc.roles(x, y)
    tiles = (dc.blocks(B) + TILE_BLOCKS - 1) // TILE_BLOCKS
    assert (dc.blocks(B), tiles) == (1067, 67)                       # 17 workgroups at one tile, 9 at two: the last one has one tile ...
    assert dc.blocks(B) % (4 * TILE_BLOCKS) == 2 * TILE_BLOCKS + 11  # ... whose third wave has 11 blocks and whose fourth is idle
    for case in dc.CASES:                                            # and every case of the table has workgroups with both tiles
        x, y, _ = case.data()
        assert dc.blocks(dc.roles(x, y)[0]) > 2 * 2 * dc.WG_BLOCKS, case.name


def test_padding_moves_every_block_to_the_other_tile():
    x, y, _ = dc.BY_NAME["uniform"].data()
    px, py, _ = padded(dc.BY_NAME["uniform"])
    B, _ = dc.roles(x, y)
    PB, _ = dc.roles(px, py)
    assert dc.blocks(PB) == dc.blocks(B) + dc.WG_BLOCKS
    assert np.array_equal(PB[PAD:], B + np.uint32(PAD))              # block b of B is block b + 64 of the padded list


def test_where_the_gaps_and_the_hard_rows_fall():
    gap = dc.BY_NAME["gap_in_b"]
    x, y, _ = gap.data()
    px, py, _ = padded(gap)
    B, _ = dc.roles(x, y)
    PB, _ = dc.roles(px, py)
    # the window gap (a tile of two windows) and the wide gap (ids that do not fit 16-bit offsets): tile 1 and tile 0 as the
    # table stands, the other way round padded
    assert (tile_of_gap(B, dc.GAP_WINDOW[0]), tile_of_gap(B, dc.GAP_WIDE[0])) == (1, 0)
    assert (tile_of_gap(PB, dc.GAP_WINDOW[0] + PAD), tile_of_gap(PB, dc.GAP_WIDE[0] + PAD)) == (0, 1)
    hard = dc.BY_NAME["hard_rows_in_b"]
    x, y, _ = hard.data()
    px, py, _ = padded(hard)
    B, _ = dc.roles(x, y)
    PB, _ = dc.roles(px, py)
    hb, phb = hard_blocks(B), hard_blocks(PB)
    assert phb == [b + dc.WG_BLOCKS for b in hb]
    assert {tile_of_block(b) for b in hb} == {0, 1}                  # rows with multi-byte gaps in both tiles, either way
    assert hb[-1] == dc.blocks(B) - 1 and B.size % dc.BLOCK != 0     # the short last block:
    assert (tile_of_block(hb[-1]), tile_of_block(phb[-1])) == (1, 0)   # tile 1 as the table stands, tile 0 padded


# ---- on the device ------------------------------------------------------------------------------------------------------------
def _run(c, ls, want, tomb=None, cap=None):
    out = c.empty(want.size + 64)
    out.upload(np.full(out.count, FILL, np.uint32))
    try:
        with path_delta(c) as took:
            _, n = c.intersect(ls, tomb=tomb, out=out) if cap is None else c.intersect(ls, tomb=tomb, out=out, cap=cap)
        got = out.download()
    finally:
        out.free()
    assert n == want.size and np.array_equal(got[:n], want)
    assert np.all(got[n:] == FILL)                                   # nothing written past the result
    return took


def _stamp_rows(c, ls):
    """workgroups of the call's kernel, by the rows of cycle counters it fills (debug.stamps; cleared per call)"""
    c.set_option("debug.stamps", 1)
    try:
        out, _ = c.intersect(ls)
        out.free()
        buf = (C.c_uint64 * (2048 * 8))()
        c._ck(c.lib.ii2_debug_read(c.h, buf, 2048 * 8))
    finally:
        c.set_option("debug.stamps", 0)
    arr = np.frombuffer(buf, dtype=np.uint64).reshape(-1, 8)
    return int(np.count_nonzero(arr.sum(axis=1)))


@pytest.fixture
def tiles_option(ctx):
    ctx.set_option("intersect.dense_form", 2)                        # every case's longer list gets a form: the instance under test runs
    yield lambda v: ctx.set_option("intersect.and2_tiles", v)
    for name, v in (("intersect.and2_tiles", 0), ("intersect.and2_slots", 0), ("intersect.and2_spin", 0), ("intersect.dense_form", 1), ("debug.stamps", 0)):
        ctx.set_option(name, v)


def _workgroups(B, tiles):
    one = (dc.blocks(B) + dc.WG_BLOCKS - 1) // dc.WG_BLOCKS
    return one if tiles == 1 else (one + 1) // 2


@gpu
@pytest.mark.parametrize("pad", [False, True], ids=["as_is", "padded"])
@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_case_at_one_tile_and_at_two(ctx, tiles_option, case, pad):
    x, y, removed = padded(case) if pad else case.data()
    want = reference(x, y, removed)
    seg = ctx.encode_lists([x, y])
    tomb = ctx.tombstones(removed) if removed is not None else None
    ls = [(seg, 0), (seg, 1)]
    try:
        for tiles in (1, 2, 2):                                      # (the first call makes the form)
            tiles_option(tiles)
            assert _run(ctx, ls, want, tomb) in FUSED
    finally:
        seg.free()
        if tomb is not None:
            tomb.free()


@pytest.fixture(scope="module")
def pair():
    x, y, _ = dc.BY_NAME["uniform"].data()
    return x, y, dc.reference(dc.BY_NAME["uniform"])


@gpu
def test_the_two_tile_instance_really_runs(ctx, tiles_option, pair):
    B, A, want = pair
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    try:
        assert _run(ctx, ls, want) in FUSED                          # (makes the form)
        tiles_option(1)
        assert _stamp_rows(ctx, ls) == _workgroups(B, 1) == 17
        tiles_option(2)
        assert _stamp_rows(ctx, ls) == _workgroups(B, 2) == 9
    finally:
        seg.free()


@gpu
def test_the_auto_rule(ctx, tiles_option, pair):
    """Two tiles exactly when the one-tile grid (17 workgroups here) is larger than what the device holds at once; that number is
    CUs x the occupancy query's answer, or what option intersect.and2_slots says."""
    B, A, want = pair
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    try:
        assert _run(ctx, ls, want) in FUSED
        tiles_option(0)
        assert _stamp_rows(ctx, ls) == 17                            # a real device holds hundreds of workgroups: one round already
        for slots, rows in ((16, 9), (17, 17), (18, 17), (1, 9)):
            ctx.set_option("intersect.and2_slots", slots)
            assert _stamp_rows(ctx, ls) == rows, slots
            assert _run(ctx, ls, want) in FUSED
        ctx.set_option("intersect.and2_slots", 16)                   # without a form there is one instance
        ctx.set_option("intersect.dense_form", 0)
        assert _stamp_rows(ctx, ls) == 17
    finally:
        seg.free()


@gpu
def test_more_than_one_look_back_group_at_two_tiles(ctx, tiles_option):
    rng = np.random.default_rng(21)
    U = 5_500_000
    B, A = dc.bern(rng, 0.4, 0, U), dc.bern(rng, 0.5, 0, U)
    assert dc.blocks(B) > 8192 and _workgroups(B, 2) > 64            # 64 workgroups a group, 128 blocks a workgroup
    want = np.intersect1d(B, A, assume_unique=True).astype(np.uint32)
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    try:
        for tiles in (1, 2, 2):
            tiles_option(tiles)
            assert _run(ctx, ls, want) in FUSED
    finally:
        seg.free()


@gpu
def test_tombstones_in_both_tiles_and_a_tile_wholly_removed(ctx, tiles_option, pair):
    B, A, _ = pair
    rng = np.random.default_rng(22)
    T = TILE_BLOCKS * dc.BLOCK                                       # postings of a tile
    k0, k1 = 2 * 8 + 1, 3 * 8 + 4 + 2                                # workgroup 2: tile 0 of wave 1; workgroup 3: tile 1 of wave 2
    whole = [np.arange(int(B[T * k]), int(B[T * (k + 1)]), dtype=np.uint32) for k in (k0, k1)]
    removed = np.unique(np.concatenate([dc.bern(rng, 0.05, 0, int(B[-1]) + 1)] + whole)).astype(np.uint32)
    want = reference(B, A, removed)
    hits = np.intersect1d(B, A, assume_unique=True)
    for w in whole:                                                  # the two tiles have hits, and none is left
        assert np.intersect1d(hits, w).size > 100 and np.intersect1d(want, w).size == 0
    for t in (0, 1):                                                 # and removed hits lie in tiles 0 and in tiles 1 all over
        gone = np.setdiff1d(hits, want, assume_unique=True)
        blk = np.searchsorted(B, gone) // dc.BLOCK
        assert np.count_nonzero(tile_of_block(blk) == t) > 1000
    seg = ctx.encode_lists([B, A])
    tomb = ctx.tombstones(removed)
    ls = [(seg, 0), (seg, 1)]
    try:
        for tiles in (1, 2, 2):
            tiles_option(tiles)
            assert _run(ctx, ls, want, tomb) in FUSED
    finally:
        seg.free()
        tomb.free()


@gpu
def test_capacity_one_short_at_two_tiles(ctx, tiles_option, pair):
    B, A, want = pair
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    out = ctx.empty(want.size + 64)
    try:
        tiles_option(2)
        for _ in range(2):
            with pytest.raises(II2Error) as e:
                ctx.intersect(ls, out=out, cap=want.size - 1)
            assert e.value.code == ECAPACITY
        _, n = ctx.intersect(ls, out=out, cap=want.size)             # exactly enough
        assert n == want.size and np.array_equal(out.download(n), want)
        assert _stamp_rows(ctx, ls) == 9
    finally:
        out.free()
        seg.free()


@gpu
@pytest.mark.parametrize("spin", [-1, -2], ids=["early", "late"])
def test_give_up_at_two_tiles(ctx, tiles_option, pair, spin):
    """The bounded waits of the look-back run out on purpose: the call notices, repeats itself through the two-kernel form and
    returns the right ids; the counter of repeated calls goes up by one."""
    B, A, want = pair
    seg = ctx.encode_lists([B, A])
    ls = [(seg, 0), (seg, 1)]
    try:
        tiles_option(2)
        assert _run(ctx, ls, want) in FUSED
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
