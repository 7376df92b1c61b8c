"""Posting lists whose DV1 bytes are laid out on purpose: a varint of every width at every position at which one of the device
decoders (csrc/dv1_device.h and its private copies) can go wrong, and the cases that carry those layouts through every consumer.

A decoder of LEB128 gaps that works four or sixteen bytes per lane can be wrong only where a varint meets one of its seams: the
lane's dword (offset mod 4), the 16-byte piece of a row lane (offset mod 16), the 256-byte chunk of one pass (offsets 256, 512),
a lane of four continuation bytes, a block that ends inside a dword, a payload that starts at an odd address.  A *cell* names
such a place: ("v", width, offset mod 4, offset mod 16, split) with split = (256 | 512, bytes of the varint in front of that
boundary) for a varint that touches a chunk boundary (0: it starts there, width: it ends there), else None.

  ids_from_widths    gap widths -> ascending ids
  matrix()           single-block lists: one planted varint (w, s) per list and the further layouts (fullest block, short
                     blocks, exact payload sizes, uniform widths); matrix_segment() orders them behind filler lists of 0..15
                     payload bytes, so that the blocks start at every address residue mod 16
  cover_blocks       composite blocks that hold many cells at once - what the set-operation cases are built from: a small
                     kernel takes 2048 postings, the whole matrix holds 30 000
  partner            the list to AND with: the ids around every planted varint, and decoys where a wrong shift would land
  cells_of           the cells a segment holds, recomputed from its ENCODED BYTES: the coverage oracle of
                     tests/test_varint_cases_cpu.py, which knows nothing of what the generator meant
  VARINT_CASES       path_cases.Case entries (exact Context.paths() delta + numpy reference), run by
                     tests/test_gpu_varint_layouts.py in the layouts "one" and "two"

What a case must carry (checked from the bytes by the CPU test):
  need = "w23"    every width-2 and width-3 cell of the matrix.
  need = "dense"  the streaming kernels want 1024 driver blocks at <= 1100 docs per block (setop.cpp: intersect_unlocked,
                  union_stream): 1.1M docs in all, of which the one-byte gaps take 0.65M - room for a few dozen three-byte gaps
                  (>= 16384 docs each) and for no wider one.  Such a case carries every dword phase of width 2 and 3 and every
                  split across the 256 boundary.
  need = "w45"    one list cannot hold more than 15 five-byte gaps (15 * 2^28 < 2^32 <= 16 * 2^28), so an AND of one wide list
                  with its partners carries a share of the width-4 and width-5 cells, and none of the narrower ones by design.
                  For these consumers the condition holds PER CONSUMER, not per case: the cases of a consumer in WIDE_CONSUMERS
                  carry every width-4 and width-5 cell between them, and its "w23" case every width-2 and width-3 cell.
Widths excluded by a selection rule:
  and.and2_*, and.dense*, or.stream*   width 4 and 5, and most of width 3: <= 1100 docs per driver / pacer block (above).
  or.tiles, or.tiles_wide              width 4 and 5: union.sparsity = 2048 docs of the common range per posting (setop.cpp:
                                       union_unlocked) - one five-byte gap needs 512 blocks, the 26 four-byte cells 104 blocks
                                       more than the ~80 the path is pinned at.
"""
import functools

import numpy as np

from tests import merge_cases as mc
from tests import path_cases as pc

BLOCK = 256
WIDTHS = (2, 3, 4, 5)
CHUNKS = (256, 512)
MAX_W5 = 15                       # five-byte gaps one list can hold: 15 * 2^28 < 2^32


# ---- gap widths -> ids ------------------------------------------------------------------------------------------------------
def varint_len(v):
    v = np.asarray(v, np.uint64)
    return 1 + (v >= 1 << 7).astype(np.int64) + (v >= 1 << 14) + (v >= 1 << 21) + (v >= 1 << 28)


def ids_from_widths(first, widths, jitter_rng, max_gap1=127, jitter_bits=28):
    """Ascending uint32 ids: `first`, then one id per entry of `widths` (1..5) - the gap in front of it is a value whose LEB128
    length is exactly that width: the smallest such value (1, 2^7, 2^14, 2^21, 2^28) plus seeded jitter inside the width's range.
    The jitter of a one-byte gap stays below max_gap1; that of a wider gap fills min(7 (w - 1), jitter_bits) low bits, and every
    whole 7-bit group among them is made non-zero: the top group of the gap is 1, and no byte of it contributes nothing (a wrong
    shift of a zero group would go unseen)."""
    widths = np.asarray(widths, np.int64)
    assert widths.ndim == 1 and (widths.size == 0 or (widths.min() >= 1 and widths.max() <= 5))
    one = widths == 1
    bits = np.minimum(7 * (widths - 1), jitter_bits)
    lim = np.where(one, max_gap1, np.int64(1) << bits)
    jit = jitter_rng.integers(0, lim) if widths.size else np.zeros(0, np.int64)
    for g in range(4):
        zero = ~one & (bits >= 7 * (g + 1)) & (((jit >> (7 * g)) & 127) == 0)
        jit[zero] |= 1 << (7 * g)
    gaps = np.where(one, 1, np.int64(1) << (7 * (widths - 1))) + jit
    assert np.array_equal(varint_len(gaps), widths)
    ids = int(first) + np.concatenate([[0], np.cumsum(gaps)])
    assert ids[-1] < 1 << 32, "the list leaves the id space"
    return ids.astype(np.uint32)


# ---- cells -------------------------------------------------------------------------------------------------------------------
def split_of(w, s):
    w, s = int(w), int(s)
    for B in CHUNKS:
        if B - w <= s <= B:
            return (B, B - s)
    return None


def cell(w, s):
    return ("v", int(w), int(s) % 4, int(s) % 16, split_of(w, s))


def wanted_offsets(w):
    """Where the matrix plants a varint of width w: all four dword phases and the first 16-byte piece boundary; every split
    across both chunk boundaries, with the positions just before and just after."""
    return list(range(20)) + list(range(256 - w, 257)) + list(range(512 - w, 513))


def wanted_cells(widths=WIDTHS):
    return {cell(w, s) for w in widths for s in wanted_offsets(w)}


def dense_ok(cells):
    """need = "dense": every dword phase of width 2 and 3, every split across the 256 boundary."""
    v = [c for c in cells if c[0] == "v"]
    return all({c[2] for c in v if c[1] == w} == {0, 1, 2, 3} and {c[4] for c in v if c[1] == w} >= {(256, k) for k in range(w + 1)}
               for w in (2, 3))


def cells_of(payload, skip, blk_off, lists=None):
    """The cells a segment holds, from its encoded bytes (payload u8, the skip table with its closing entry, blk_off u32
    [n_lists + 1]; lists: only the blocks of these lists):
      ("v", w, s % 4, s % 16, split)   a varint of width w >= 2 starts at offset s of its block's payload
      ("start", r)                      a block that holds such a varint starts at a payload address = r mod 16
      ("cont4",)                        a lane's dword (block offset = 0 mod 4) is four continuation bytes
      ("cont4_piece",)                  the four bytes in front of a 16-byte piece (block offset = 0 mod 16) are continuation bytes
      ("tail", n)                       a block that holds such a varint ends n = 1..3 bytes into a dword
      ("len", n)                        a block that holds such a varint has n = 255 or 256 payload bytes (the lengths at which
                                        the streaming kernels' fast-path tests are decided by the continuation bytes alone)"""
    payload = np.asarray(payload, np.uint8)
    byte_off = np.asarray(skip["byte_off"], np.int64)
    blk_off = np.asarray(blk_off, np.int64)
    keep = np.zeros(byte_off.size - 1, bool)
    for l in (range(blk_off.size - 1) if lists is None else lists):
        keep[blk_off[l]:blk_off[l + 1]] = True
    ends = np.flatnonzero(payload[: byte_off[-1]] < 128)                          # terminator bytes
    starts = np.concatenate([[0], ends[:-1] + 1]) if ends.size else ends
    width = ends - starts + 1
    blk = np.searchsorted(byte_off, starts, "right") - 1
    assert np.all(byte_off[blk] <= starts) and np.all(ends < byte_off[blk + 1]), "a varint crosses its block's end"
    sel = (width >= 2) & keep[blk]
    out = set()
    s = starts[sel] - byte_off[blk[sel]]
    for w, so in set(zip(width[sel].tolist(), s.tolist())):
        out.add(cell(w, so))
    wide_blocks = np.unique(blk[sel])
    for r in np.unique(byte_off[wide_blocks] % 16):
        out.add(("start", int(r)))
    for n in np.unique((byte_off[wide_blocks + 1] - byte_off[wide_blocks]) % 4):
        if n:
            out.add(("tail", int(n)))
    for n in np.unique(byte_off[wide_blocks + 1] - byte_off[wide_blocks]):
        if n in (BLOCK - 1, BLOCK):
            out.add(("len", int(n)))
    w5 = sel & (width == 5)
    rel = starts[w5] - byte_off[blk[w5]]
    if np.any(rel % 4 == 0):
        out.add(("cont4",))
    if np.any(rel % 16 == 12):
        out.add(("cont4_piece",))
    return out


# ---- blocks --------------------------------------------------------------------------------------------------------------
def block_widths(targets, bg, n_gaps=BLOCK - 1):
    """The gap widths of one block in which a varint of width w starts at payload offset s for every (s, w) of targets: between
    them background gaps of width bg, in front of those as many one-byte gaps as it takes to hit s exactly; background to the end."""
    out, off = [], 0
    for s, w in sorted(targets):
        d = s - off
        assert d >= 0, "planted varints overlap"
        out += [1] * (d % bg) + [bg] * (d // bg) + [w]
        off = s + w
    assert len(out) <= n_gaps, "the block has no room for its planted varints"
    return np.array(out + [bg] * (n_gaps - len(out)), np.uint8)


def cells_of_widths(widths):
    """{cell: index of the first gap that holds it} of a block, from its gap widths (the generator's own bookkeeping)."""
    off = np.concatenate([[0], np.cumsum(widths.astype(np.int64))[:-1]])
    out = {}
    for i in np.flatnonzero(widths >= 2):
        out.setdefault(cell(widths[i], off[i]), int(i))
    return out


class Block:
    """widths: the block's gap widths; marks: indices of the gaps that were planted, or that hold a wanted cell first."""

    def __init__(self, widths, marks):
        self.widths, self.marks = widths, sorted(set(marks))


def _fits(targets, bg, n_gaps):
    off, gaps = 0, 0
    for s, w in sorted(targets):
        if s < off:
            return False
        gaps += (s - off) // bg + (s - off) % bg + 1
        off = s + w
    return gaps <= n_gaps


def cover_blocks(wanted, bg, max_w5=5, n_gaps=BLOCK - 1):
    """Full blocks that hold every cell of `wanted` between them, as few as a greedy walk finds.  Only one or two varints of a
    block can touch a chunk boundary, so each block first takes, per boundary, a missing cell that ends there and one that starts
    there (else one that straddles it); then, from its start on, the nearest missing cell that still fits - the gaps it takes to
    get there, at most max_w5 five-byte gaps - over a background of width bg, one wider where nothing fits otherwise (offset 512
    cannot be reached with 255 two-byte gaps)."""
    left, blocks = set(wanted), []
    while left:
        best_try = None
        for width, boost in ((bg, 0), (bg, 4), (bg, 8), (bg + 1, 0), (bg + 2, 0)):
            if width > 5:
                continue
            targets, got = [(3 * i, 3) for i in range(boost)], set()         # (three-byte gaps up front: bytes to reach 512 with)

            def take(c, s):
                if sum(w == 5 for _, w in targets) + (c[1] == 5) > max_w5 or not _fits(targets + [(s, c[1])], width, n_gaps):
                    return False
                targets.append((s, c[1]))
                got.add(c)
                return True
            for B in CHUNKS:
                at = sorted((c for c in left if c[4] and c[4][0] == B), key=lambda c: (-c[1], c[4][1]))
                ends, begins = [c for c in at if c[4][1] == c[1]], [c for c in at if c[4][1] == 0]
                inner = [c for c in at if 0 < c[4][1] < c[1]]
                for c in (ends[:1] + begins[:1]) or inner[:1]:
                    take(c, B - c[4][1])
            while True:
                best = None
                for c in left - got:
                    if c[4] is not None:
                        continue
                    w, r16 = c[1], c[3]
                    for s in range(r16, CHUNKS[-1], 16):
                        if split_of(w, s) is None and (best is None or (s, w) < best[:2]) and \
                                all(s + w <= t or t + tw <= s for t, tw in targets) and _fits(targets + [(s, w)], width, n_gaps):
                            best = (s, w, c)
                            break
                if best is None or not take(best[2], best[0]):
                    break
            if got:
                held = set(cells_of_widths(block_widths(targets, width, n_gaps))) & left
                if best_try is None or len(held) > best_try[0]:
                    best_try = (len(held), width, targets, got)
        assert best_try, "a wanted cell fits no block"
        _, width, targets, got = best_try
        widths = block_widths(targets, width, n_gaps)
        held = cells_of_widths(widths)
        assert got <= set(held)
        offs = np.concatenate([[0], np.cumsum(widths.astype(np.int64))[:-1]])
        planted = [int(np.flatnonzero(offs == s)[0]) for s, _ in targets]
        blocks.append(Block(widths, planted + [i for c, i in held.items() if c in left]))
        left -= set(held)
    return blocks


def chain(blocks, first, rng, max_gap1=127, jitter_bits=28):
    """One list of the blocks' gap widths, a one-byte gap between two blocks (it is not encoded: the next block's first doc is
    its skip entry).  Returns (ids, marks): marks = indices of the ids that END a marked gap."""
    widths, marks, at = [], [], 0
    for b in blocks:
        w = b.widths if isinstance(b, Block) else np.asarray(b, np.uint8)
        assert at % BLOCK == 0, "only a list's last block may be short"
        marks += [at + i + 1 for i in (b.marks if isinstance(b, Block) else [])]
        widths += [w, np.ones(1, np.uint8)]
        at += w.size + 1
    ids = ids_from_widths(first, np.concatenate(widths)[:-1], rng, max_gap1, jitter_bits)
    return ids, marks


def partner(ids, cells, extra=()):
    """The list to AND against `ids`: for every planted varint (cells: indices of the ids that end one) that id and the one
    before it, and decoys at the values a decoder would produce if it shifted one byte of the varint by 7 bits too many or too
    few, or forgot the continuation bytes pending in front of one of its bytes - decoys that are ids of the list are left out.
    A wrong decode then shows as a missing id and as a spurious one.  extra: further ids to hold."""
    v = ids.astype(np.int64)
    real, decoy = set(int(x) for x in extra), set()
    for i in cells:
        prev, gap = int(v[i - 1]), int(v[i] - v[i - 1])
        grp = []
        while True:
            grp.append(gap & 127)
            gap >>= 7
            if not gap:
                break
        gap = int(v[i] - v[i - 1])
        alts = set()
        for j, b in enumerate(grp):
            alts.add(gap - (b << 7 * j) + (b << 7 * (j + 1)))
            if j:
                alts.add(gap - (b << 7 * j) + (b << 7 * (j - 1)))
        for k in range(1, len(grp)):
            alts.add(sum(b << 7 * j for j, b in enumerate(grp[:k])) + sum(b << 7 * j for j, b in enumerate(grp[k:])))
        real |= {prev, prev + gap}
        decoy |= {(prev + a) & 0xFFFFFFFF for a in alts if a != gap}
    decoy = np.setdiff1d(np.array(sorted(decoy), np.int64), v)
    assert decoy.size >= len(cells)
    return np.union1d(np.array(sorted(real), np.int64), decoy).astype(np.uint32)


def grown(p, carrier, n, rng):
    """p grown to n ids: half of the new ones are further ids of the carrier (never more than half of what is left of it), the
    others ids of its doc range that it lacks."""
    assert p.size <= n, (p.size, n)
    k = n - p.size
    hits = np.setdiff1d(carrier, p)
    hits = hits[rng.permutation(hits.size)[: min(k // 2, hits.size // 2)]]
    p = pc.with_ids(p, hits)
    lo, hi = int(carrier[0]), int(carrier[-1]) + 1
    while p.size < n:
        miss = np.setdiff1d(np.unique(rng.integers(lo, hi, 2 * (n - p.size) + 16, dtype=np.int64)), np.union1d(carrier, p))
        p = pc.with_ids(p, miss[rng.permutation(miss.size)[: n - p.size]])
    assert p.size == n
    return p


# ---- the matrix ------------------------------------------------------------------------------------------------------------
def planted(w, s):
    """One varint of width w at payload offset s: one-byte background where the offset can be reached with it, else three-byte."""
    return Block(block_widths([(s, w)], 1 if s <= BLOCK - 2 else 3), [])


def fullest_block():
    """The gap widths of the block with the most payload bytes that fits below 2^32: n5 five-byte, n4 four-byte, the rest
    three-byte gaps at their smallest values, searched - 14 and 241: 1034 bytes, more than four chunks."""
    best = None
    for n5 in range(MAX_W5 + 1):
        for n4 in range(BLOCK - n5):
            n3 = BLOCK - 1 - n5 - n4
            if (n5 << 28) + (n4 << 21) + (n3 << 14) + (BLOCK << 16) < 1 << 32 and (best is None or 5 * n5 + 4 * n4 + 3 * n3 > best[0]):
                best = (5 * n5 + 4 * n4 + 3 * n3, n5, n4, n3)
    nbytes, n5, n4, n3 = best
    w = np.array([4] * n4 + [3] * n3, np.uint8)
    at = np.linspace(0, w.size, n5 + 2).astype(np.int64)[1:-1]                     # the five-byte gaps spread over the block
    w = np.insert(w, at, 5)
    assert w.size == BLOCK - 1 and int(w.sum()) == nbytes
    return w, (n5, n4, n3)


def exact_payload(nbytes):
    """A full block of exactly nbytes payload bytes: the narrowest widths that reach it, the wider gaps spread over the block."""
    base = nbytes // (BLOCK - 1)
    n_wide = nbytes - base * (BLOCK - 1)
    w = np.full(BLOCK - 1, base, np.uint8)
    w[np.linspace(3, BLOCK - 5, n_wide).astype(np.int64)] += 1
    assert int(w.sum()) == nbytes and np.count_nonzero(w > base) == n_wide
    return w


@functools.lru_cache(maxsize=None)
def matrix():
    """[(name, ids)]: the single-block lists."""
    rng = np.random.default_rng(20)
    out = []
    add = lambda name, widths, **kw: out.append((name, ids_from_widths(int(rng.integers(0, 5000)), widths, rng, **kw)))
    for w in WIDTHS:
        for s in wanted_offsets(w):
            add(f"w{w}_s{s}", planted(w, s).widths)
    full, _ = fullest_block()
    add("fullest", full, jitter_bits=16)
    out.append(("one_posting", np.array([int(rng.integers(0, 1 << 32))], np.uint32)))
    for n in (2, 3, 4, 5):
        for w in WIDTHS:
            add(f"short_{n}_last_w{w}", [1] * (n - 2) + [w])
    for nbytes in (255, 256, 257, 511, 512, 513):
        add(f"payload_{nbytes}", exact_payload(nbytes))
    add("payload_255_short_block", [2] * 56 + [1] * 143)                            # 200 postings, multi-byte gaps, 255 bytes
    for w in (2, 3, 4):
        add(f"all_w{w}", [w] * (BLOCK - 1))
    assert len({n for n, _ in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def matrix_segment():
    """(lists, is_matrix): the matrix lists dealt into sixteen groups, in front of group f a filler list of f payload bytes."""
    groups = [matrix()[f::16] for f in range(16)]
    lists, is_matrix = [], []
    for f, g in enumerate(groups):
        lists.append(np.arange(7, 7 + f + 1, dtype=np.uint32))                     # f one-byte gaps
        is_matrix.append(False)
        for _, ids in g:
            lists.append(ids)
            is_matrix.append(True)
    return tuple(lists), tuple(is_matrix)


def csr(lists):
    return mc.csr(lists)


# ---- the lists of the cases ------------------------------------------------------------------------------------------------
W23, W45 = wanted_cells((2, 3)), wanted_cells((4, 5))


@functools.lru_cache(maxsize=None)
def s23():
    return tuple(cover_blocks(W23, 2))


@functools.lru_cache(maxsize=None)
def s45():
    return tuple(cover_blocks(W45, 2))


@functools.lru_cache(maxsize=None)
def wide_groups():
    """The blocks of s45() as lists: blocks in order, a new list where one more block would bring the list above seven
    five-byte gaps (their jittered values reach 2^29: seven stay below 2^32 with room for the rest)."""
    groups, n5 = [[]], 0
    for b in s45():
        k = int(np.count_nonzero(b.widths == 5))
        if groups[-1] and n5 + k > 7:
            groups.append([])
            n5 = 0
        groups[-1].append(b)
        n5 += k
    return tuple(tuple(g) for g in groups)


N45 = len(wide_groups())
PLAIN = np.ones(BLOCK - 1, np.uint8)                  # a block of one-byte gaps


@functools.lru_cache(maxsize=None)
def carrier23(seed, reps=1):
    """(ids, marks): the blocks that hold every width-2 and width-3 cell, reps times over (fresh jitter each time)."""
    return chain(s23() * reps, 1000 + 37 * seed, np.random.default_rng(2300 + seed))


@functools.lru_cache(maxsize=None)
def carrier45(seed, j, pad=0):
    """(ids, marks): list j of those that hold the width-4 and width-5 cells, behind `pad` blocks of one-byte gaps."""
    return chain((PLAIN,) * pad + wide_groups()[j], 500 + 11 * seed + j, np.random.default_rng(4500 + 10 * seed + j))


@functools.lru_cache(maxsize=None)
def pair23(seed, n_partner, reps=1):
    c, marks = carrier23(seed, reps)
    p = partner(c, marks)
    return c, grown(p, c, max(n_partner, p.size), np.random.default_rng(2350 + seed))


@functools.lru_cache(maxsize=None)
def pair45(seed, j, n_partner, pad=0):
    c, marks = carrier45(seed, j, pad)
    p = partner(c, marks)
    return c, grown(p, c, max(n_partner, p.size), np.random.default_rng(4550 + seed + j))


PROBE_PAD = 20                    # blocks of one-byte gaps on either side of a probed carrier's wide blocks
PROBE_MIN_BLOCKS = 16             # intersect.hip: a list with this many blocks in a tile's doc range is probed sixteen bytes per lane


@functools.lru_cache(maxsize=None)
def probe_pair(seed, j, n_partner):
    """(carrier, partner, marks) for the split-driver probes: the carrier's wide blocks (j = None: the width-2 / width-3 blocks,
    else wide list j) between PROBE_PAD blocks of one-byte gaps on either side; the partner - two blocks, it drives - holds an
    id of the carrier's first and last block, so each of its blocks spans at least one whole pad: PROBE_MIN_BLOCKS blocks of the
    carrier and more lie in the doc range of every driver block (probed_blocks() counts them; the CPU test requires it)."""
    pad = (PLAIN,) * PROBE_PAD
    c, marks = chain(pad + (s23() if j is None else wide_groups()[j]) + pad, 300 + seed, np.random.default_rng(9000 + 10 * seed + (j or 0)))
    p = partner(c, marks, extra=(int(c[1]), int(c[-2])))
    p = grown(p, c, n_partner, np.random.default_rng(9050 + seed + (j or 0)))
    assert BLOCK < p.size <= 2 * BLOCK
    return c, p, tuple(marks)


def probed_blocks(driver, probed, ids):
    """For every id of `ids`: the blocks of `probed` inside the doc range of the driver's block that holds the id - bh - bl of
    k_isect_partition (from the last block that starts at or before the driver block's first doc to the first one that starts
    behind its last)."""
    first = probed[::BLOCK].astype(np.int64)
    d_first = driver[::BLOCK].astype(np.int64)
    out = []
    for x in np.asarray(ids, np.int64):
        b = int(np.searchsorted(d_first, x, "right")) - 1
        lo = int(d_first[b])
        hi = int(d_first[b + 1]) - 1 if b + 1 < d_first.size else int(driver[-1])
        ub = int(np.searchsorted(first, lo, "right"))
        out.append(int(np.searchsorted(first, hi, "right")) - (ub - 1 if ub else 0))
    return out


def supersets(p, carrier, n_lists, n, seed):
    """n_lists lists of n ids that all hold p (an AND of many lists keeps exactly what they share with the carrier and each other)."""
    return tuple(grown(p, carrier, n, np.random.default_rng(seed + i)) for i in range(n_lists))


def wide_carriers(seed, pad=0):
    return tuple(carrier45(seed, j, pad)[0] for j in range(N45))


@functools.lru_cache(maxsize=None)
def dense_blocks():
    """Blocks of one-byte gaps with the few wide gaps the streaming kernels' density leaves room for: a three-byte gap at
    253 .. 256 (every split across the chunk boundary, every dword phase), a two-byte gap at 254 .. 256 and at 5, 10, 15 -
    259 or 260 payload bytes each, which the length term of the streaming kernels' own `hard` tests (intersect_and2.hip: len !=
    255, intersect_dense.hip: len > 256) sends to the general decoder; then a full block of exactly 256 bytes (one two-byte gap
    at 254), which only the continuation-byte term of intersect_dense.hip's test catches.  (dense_lists() ends the list with a
    short block of 255 bytes: the one only the continuation-byte term of intersect_and2.hip's test catches.)"""
    early = [(5, 2), (10, 2), (15, 2)]
    out = []
    for w in (2, 3):
        for k in range(w + 1):
            widths = block_widths(early + [(256 - k, w)], 1)
            out.append(Block(widths, np.flatnonzero(widths >= 2).tolist()))
    widths = block_widths([(254, 2)], 1)
    assert int(widths.sum()) == BLOCK
    out.append(Block(widths, np.flatnonzero(widths >= 2).tolist()))
    return tuple(out)


SHORT_255 = np.array([2] * 56 + [1] * 143, np.uint8)          # 200 postings, 255 payload bytes


@functools.lru_cache(maxsize=None)
def dense_lists(seed, k, n_blocks=1024):
    """k lists of n_blocks blocks at no more than 1100 docs per block: the first holds dense_blocks() spread among blocks of
    one-byte gaps (gaps of 1 .. 4 docs) and ends with the short block SHORT_255, every other one half of its ids and as many
    that it lacks."""
    rng = np.random.default_rng(seed)
    at = {int(i): b for i, b in zip(np.linspace(5, n_blocks - 6, len(dense_blocks())).astype(np.int64), dense_blocks())}
    blocks = [at.get(i, PLAIN) for i in range(n_blocks - 1)] + [Block(SHORT_255, np.flatnonzero(SHORT_255 >= 2).tolist())]
    c, marks = chain(blocks, 100, rng, max_gap1=4)
    per_block = (int(c[(n_blocks - 1) * BLOCK]) - int(c[0])) / (n_blocks - 1)
    assert c.size == (n_blocks - 1) * BLOCK + SHORT_255.size + 1 and per_block <= 1100.0, per_block
    p = partner(c, marks)
    return (c,) + tuple(grown(p, c, c.size, np.random.default_rng(seed + 1 + i)) for i in range(k - 1))


@functools.lru_cache(maxsize=None)
def stream_lists(seed, m):
    """The pacer of 1024 blocks with the dense layouts, then m - 1 lists of 50 000 ids of its doc range."""
    c = dense_lists(seed, 1)[0]
    rng = np.random.default_rng(seed + 50)
    return (c,) + tuple(pc.pick(rng, 50_000, int(c[0]), int(c[-1]) + 1) for _ in range(m - 1))


@functools.lru_cache(maxsize=None)
def plain_lists(seed, sizes, lo, hi):
    rng = np.random.default_rng(seed)
    return tuple(pc.pick(rng, n, lo, hi) for n in sizes)


# ---- the cases -------------------------------------------------------------------------------------------------------------
class VCase(pc.Case):
    """A path case with what it carries: consumer = the decoding consumer it pins (a path id, or a group of them), need = "w23" |
    "dense" | "w45" (see the module's docstring)."""

    def __init__(self, name, consumer, need, lists, call, expect, **kw):
        super().__init__(name, lists, call, expect, **kw)
        self.consumer, self.need = consumer, need

    def layouts(self):
        return ["one", "two"]


# consumers whose selection rules admit four- and five-byte gaps: their "w45" cases carry every such cell between them
WIDE_CONSUMERS = ("and.small", "or.small", "andnot.small", "batch", "gbatch", "and.tiles_pair", "and.tiles", "and.tiles_sub",
                  "and.tiles_wide", "and.tiles_wide_sub", "or.rank", "or.merge", "or.many", "ir.probe", "ir.mark", "andnot.general")


def _windows(lists, log2=30):
    lo, hi = min(int(l[0]) for l in lists), max(int(l[-1]) for l in lists)
    base = lo & ~31
    return (hi - base + 1 + (1 << log2) - 1) >> log2


def _group_lists(seed):
    """[carriers | z | partners | b, bw]: the AND-of-ORs operands.  Group 1 = the carriers and z, group 2 = z and the partners
    (z, in both, holds the partner ids of the excluded lists: the ids they must remove, and decoys they must not).  Excluded: b,
    a second w23 carrier, and bw, the first wide list - the drop passes run the keep passes' kernel and decoder with one flag
    set, so they get every width-2 / width-3 cell and one list's share of the wider ones."""
    cs = [carrier23(seed)] + [carrier45(seed, j) for j in range(N45)]
    ps = [partner(c, m) for c, m in cs]
    b, bm = carrier23(seed + 1)
    bw, bwm = carrier45(seed + 1, 0)
    z = np.union1d(partner(b, bm), partner(bw, bwm)).astype(np.uint32)
    return tuple([c for c, _ in cs] + [z] + ps + [b, bw])


def _cases():
    c = []
    PROBE, MARK = {"intersect.ranges_mark": 0}, {"intersect.ranges_mark": pc.ALWAYS_MARK}
    UNSPLIT = {"intersect.submax": 1}
    n23 = len(s23()) * BLOCK

    def both(*a, **kw):
        c.extend([VCase(*a, **kw), VCase(a[0] + "_tomb", *a[1:], tomb=True, **kw)])

    def per_wide_block(name, consumer, lists_of_j, call, expect, **kw):
        for j in range(N45):
            c.append(VCase(f"{name}_w45_{j}", consumer, "w45", (lambda j=j: lists_of_j(j)), call, expect, **kw))

    # -- the one-workgroup kernels (small_set_device.h: the pre-loaded dword in front of decode_block_wave)
    both("and_small_w23", "and.small", "w23", lambda: pair23(1, 2048 - n23), ("intersect", [0, 1]), {"and.small": 1})
    per_wide_block("and_small", "and.small", lambda j: pair45(1, j, 600), ("intersect", [0, 1]), {"and.small": 1})
    or_small = lambda: (carrier23(2)[0],) + wide_carriers(2) + plain_lists(2, (500,), 0, 1_000_000)
    n_or = 2 + N45
    both("or_small_w23_w45", "or.small", "w23", or_small, ("union", list(range(n_or))), {"or.small": 1})
    nc = 1 + N45
    an_call = ("andnot", [[(0, nc + 1)], [(nc, 2 * nc + 1)]], [[(2 * nc + 1, 2 * nc + 3)]])
    gl = lambda: _group_lists(3)
    general = lambda f, d: {"andnot.general": 1, "ir.groups": 1, "or.small": 1, f: 1, d: 1}
    both("andnot_small", "andnot.small", "w23", gl, an_call, {"andnot.small": 1}, options={"andnot.small": 2})
    both("andnot_general_probe", "andnot.general", "w23", gl, an_call, general("ir.probe", "ir.probe_drop"),
         options=dict(PROBE, **{"andnot.small": 0}))
    both("andnot_general_mark", "andnot.general", "w23", gl, an_call, general("ir.mark", "ir.mark_drop"),
         options=dict(MARK, **{"andnot.small": 0}))
    ir_call = ("intersect_ranges", [[(0, nc + 1)], [(nc, 2 * nc + 1)]])
    both("ir_probe", "ir.probe", "w23", gl, ir_call, {"ir.groups": 1, "or.small": 1, "ir.probe": 1}, options=PROBE)
    both("ir_mark", "ir.mark", "w23", gl, ir_call, {"ir.groups": 1, "or.small": 1, "ir.mark": 1}, options=MARK)
    # a batch: [c23, p23 | (c45_j, p45_j) ... | c23 x 2, its partner | the carriers once more, for the OR]
    def batch_lists():
        out = list(pair23(4, 700))
        for j in range(N45):
            out += pair45(4, j, 300)
        out += pair23(5, 900, reps=2)
        return tuple(out) + (carrier23(4)[0],) + wide_carriers(4)
    nb = 2 + 2 * N45
    bq = [("and", [(0, 2)])] + [("and", [(2 + 2 * j, 4 + 2 * j)]) for j in range(N45)] + [("and", [(nb, nb + 2)]), ("or", [(nb + 2, nb + 3 + N45)])]
    both("batch", "batch", "w23", batch_lists, ("batch", bq), {"batch.tiny": 1, "batch.small": 1, "batch.pack": 1})
    # grouped batch: the AND-of-ORs minus b as one small query; tiny ones: (c45_j AND its partner) minus a plain list
    def gbatch_lists():
        out = list(_group_lists(6))
        for j in range(N45):
            out += pair45(6, j, 300)
        return tuple(out) + plain_lists(6, (300,), 0, 1 << 32)
    g0 = 2 * nc + 3
    gq = [(an_call[1], an_call[2])] + [([[(g0 + 2 * j, g0 + 2 * j + 1)], [(g0 + 2 * j + 1, g0 + 2 * j + 2)]], [[(g0 + 2 * N45, g0 + 2 * N45 + 1)]])
                                       for j in range(N45)]
    both("gbatch", "gbatch", "w23", gbatch_lists, ("gbatch", gq), {"gbatch.tiny": 1, "gbatch.small": 1, "gbatch.pack": 1})
    # -- AND: the tile kernel.  A block with multi-byte gaps spans >= 8192 docs, so the chooser would split the driver's blocks
    # (and.tiles_sub): intersect.submax = 1 keeps it from that where the unsplit instantiations are meant
    both("and_tiles_pair_w23", "and.tiles_pair", "w23", lambda: pair23(7, 1400, reps=2), ("intersect", [0, 1]), {"and.tiles_pair": 1}, options=UNSPLIT)
    c.append(VCase("and_tiles_pair_w23_every_tile_gallops", "and.tiles_pair", "w23", lambda: pair23(7, 1400, reps=2), ("intersect", [0, 1]),
                   {"and.tiles_pair": 1}, options=dict(UNSPLIT, **{"intersect.map_docs": 1})))
    c.append(VCase("and_tiles_pair_w23_carrier_drives", "and.tiles_pair", "w23", lambda: pair23(7, 3000), ("intersect", [0, 1]),
                   {"and.tiles_pair": 1}, options=UNSPLIT))
    per_wide_block("and_tiles_pair", "and.tiles_pair", lambda j: pair45(7, j, 300, pad=8), ("intersect", [0, 1]), {"and.tiles_pair": 1}, options=UNSPLIT)

    def three(pair):
        car, p = pair
        return (car, p) + supersets(p, car, 1, p.size + 200, 77)
    both("and_tiles_w23", "and.tiles", "w23", lambda: three(pair23(8, 1400, reps=2)), ("intersect", [0, 1, 2]), {"and.tiles": 1}, options=UNSPLIT)
    per_wide_block("and_tiles", "and.tiles", lambda j: three(pair45(8, j, 300, pad=8)), ("intersect", [0, 1, 2]), {"and.tiles": 1}, options=UNSPLIT)
    # the partner (two blocks over the carrier's whole doc range) drives, its blocks are split; the carrier has more than
    # PROBE_MIN_BLOCKS blocks in the doc range of each: its blocks are probed sixteen bytes per lane (decode_rows16_any,
    # intersect.hip: "many blocks in range") - with fewer blocks in range the probes go through decode_block_wave
    for submax in (3, 16):
        opt = {"intersect.submax": submax}
        c.append(VCase(f"and_tiles_sub_{submax}_w23", "and.tiles_sub", "w23", lambda: probe_pair(9, None, 500)[:2], ("intersect", [0, 1]), {"and.tiles_sub": 1}, options=opt))
        per_wide_block(f"and_tiles_sub_{submax}", "and.tiles_sub", lambda j: probe_pair(9, j, 300)[:2], ("intersect", [0, 1]), {"and.tiles_sub": 1}, options=opt)

    def wide64(pair):
        car, p = pair
        return (car,) + supersets(p, car, 63, p.size + 100, 640)
    all64 = ("intersect", list(range(64)))
    both("and_tiles_wide_w23", "and.tiles_wide", "w23", lambda: wide64(pair23(10, 0, reps=2)), all64, {"and.tiles_wide": 1}, options=UNSPLIT)
    per_wide_block("and_tiles_wide", "and.tiles_wide", lambda j: wide64(pair45(10, j, 300, pad=8)), all64, {"and.tiles_wide": 1}, options=UNSPLIT)
    both("and_tiles_wide_sub_w23", "and.tiles_wide_sub", "w23", lambda: wide64(pair23(10, 0, reps=2)), all64, {"and.tiles_wide_sub": 1})
    per_wide_block("and_tiles_wide_sub", "and.tiles_wide_sub", lambda j: wide64(pair45(10, j, 300, pad=8)), all64, {"and.tiles_wide_sub": 1})
    # -- AND: the streaming kernels (1024 driver blocks at <= 1100 docs per block; see need = "dense")
    dense = lambda k: (lambda: dense_lists(11, k))
    c += [VCase("and_and2_fused_dense", "and.and2_fused", "dense", dense(2), ("intersect", [0, 1]), {"and.and2_fused": 1}),
          VCase("and_and2_fused_dense_lists_swapped", "and.and2_fused", "dense", dense(2), ("intersect", [1, 0]), {"and.and2_fused": 1}),
          VCase("and_and2_split_dense", "and.and2_split", "dense", dense(2), ("intersect", [0, 1]), {"and.and2_split": 1}, options={"intersect.and2": 2}),
          VCase("and_and2_split_dense_lists_swapped", "and.and2_split", "dense", dense(2), ("intersect", [1, 0]), {"and.and2_split": 1},
                options={"intersect.and2": 2}),
          VCase("and_dense2_dense", "and.dense2", "dense", dense(2), ("intersect", [0, 1]), {"and.dense2": 1}, options={"intersect.and2": 0}),
          VCase("and_dense2_dense_lists_swapped", "and.dense2", "dense", dense(2), ("intersect", [1, 0]), {"and.dense2": 1}, options={"intersect.and2": 0}),
          VCase("and_dense2_bpw_32_dense", "and.dense2", "dense", dense(2), ("intersect", [0, 1]), {"and.dense2": 1}, options={"intersect.dense_bpw": 32}),
          VCase("and_dense3_dense", "and.dense3", "dense", dense(3), ("intersect", [0, 1, 2]), {"and.dense3": 1}, tomb=True),
          VCase("and_dense4_dense", "and.dense4", "dense", dense(4), ("intersect", [0, 1, 2, 3]), {"and.dense4": 1})]
    # -- OR
    rank = lambda: (carrier23(12, 2)[0], carrier23(13, 2)[0]) + wide_carriers(12, pad=8)
    both("or_rank_w23_w45", "or.rank", "w23", rank, ("union", list(range(2 + N45))), {"or.rank": 1})
    for m in (2, 3, 4):
        c.append(VCase(f"or_stream{m}_dense", f"or.stream{m}", "dense", lambda m=m: stream_lists(14, m), ("union", list(range(m))), {f"or.stream{m}": 1},
                       options={"union.rank": 0}, tomb=m == 3))
    tiles = lambda: tuple(carrier23(20 + i, 2)[0] for i in range(7)) + plain_lists(15, (700,) * 3, 0, 9_000_000)
    both("or_tiles_w23", "or.tiles", "w23", tiles, ("union", list(range(10))), {"or.tiles": 1})
    tiles_wide = lambda: tuple(carrier23(20 + i, 2)[0] for i in range(7)) + plain_lists(16, (200,) * 57, 0, 9_000_000)
    both("or_tiles_wide_w23", "or.tiles_wide", "w23", tiles_wide, ("union", list(range(64))), {"or.tiles_wide": 1})
    merge = lambda: tuple(carrier23(30 + i, 2)[0] for i in range(3)) + wide_carriers(14, pad=8)
    both("or_merge_w23_w45", "or.merge", "w23", merge, ("union", list(range(3 + N45))), {"or.merge": 1})
    one_window = lambda: tuple(carrier23(40 + i)[0] for i in range(3))
    assert _windows(one_window()) == 1
    both("or_many_one_window_w23", "or.many", "w23", one_window, ("union_ranges", [(0, 3)]), {"or.many": 1, "or.many_window": 1}, options={"union.many": 1})
    n_win = _windows(one_window(), 17)
    assert n_win >= 4
    c.append(VCase("or_many_small_windows_w23", "or.many", "w23", one_window, ("union_ranges", [(0, 3)]), {"or.many": 1, "or.many_window": n_win},
                   options={"union.many": 1, "union.many_window_log2": 17}, tomb=True))
    n_win = _windows(rank())
    assert n_win >= 2
    both("or_many_windows_w45", "or.many", "w45", rank, ("union_ranges", [(0, 2 + N45)]), {"or.many": 1, "or.many_window": n_win}, options={"union.many": 1})
    names = [x.name for x in c]
    assert len(set(names)) == len(names), "case names are unique"
    return c


VARINT_CASES = _cases()
BY_NAME = {c.name: c for c in VARINT_CASES}

# the cases that reach decode_rows16_any.  Two-list split drivers (intersect.hip: the probe loop of list 1) reach it only with
# PROBE_MIN_BLOCKS blocks of the carrier in the driver block's doc range: PROBED_CASES = {name: (seed, j)} of probe_pair().  The
# 64-list split drivers reach it through the combined pass over lists 2 .. 63, where the carrier - the longest list - sorts last.
PROBED_CASES = {f"and_tiles_sub_{submax}_w23": (9, None) for submax in (3, 16)}
PROBED_CASES.update({f"and_tiles_sub_{submax}_w45_{j}": (9, j) for submax in (3, 16) for j in range(N45)})
COMBINED_PROBE_CASES = tuple(c.name for c in VARINT_CASES if c.consumer == "and.tiles_wide_sub")


# ---- ii2_count_ranges and the merges ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def count_lists():
    """(lists, set ids): every carrier; the set holds the partners' ids (hits around every planted varint, decoys)."""
    cs = [carrier23(50, 2)] + [carrier45(50, j, pad=1) for j in range(N45)]
    ids = functools.reduce(np.union1d, [partner(c, m) for c, m in cs])
    return tuple(c for c, _ in cs), ids.astype(np.uint32)


def _aligned(terms, k):
    """k segments (CSR pairs) from per-term tuples of up to k lists (missing ones: empty)."""
    E = np.empty(0, np.uint32)
    return [csr([t[s] if s < len(t) else E for t in terms]) for s in range(k)]


@functools.lru_cache(maxsize=None)
def merge_small_terms(k):
    """Per-term tuples of lists, fewer than 8192 postings in all (ii2_merge_small): the w23 carrier against a second one, the
    wide blocks two to a term, a few short matrix lists; the same terms serve ii2_merge_segments as a batch of small terms."""
    m = dict(matrix())
    terms = [(carrier23(60)[0], carrier23(61)[0])]
    wide = wide_carriers(60)
    terms += [tuple(wide[i:i + 2]) for i in range(0, N45, 2)]
    terms += [(m["short_5_last_w5"], m["short_2_last_w3"], m["payload_255_short_block"], m["short_3_last_w4"], m["one_posting"])[:k]]
    assert sum(l.size for t in terms for l in t) <= 8192
    return tuple(terms)


@functools.lru_cache(maxsize=None)
def merge_tile_terms(k):
    """Per-term tuples of k lists for the tile kernel: the matrix lists k to a term (batches of small terms), then a large term
    of k two-fold w23 carriers (range tiles), the wide lists behind eight plain blocks as terms of their own and, last, the
    last k wide lists bare as one term: with merge.large_tile = 1000 its doc range is cut in the middle of their blocks, which
    the plan kernels' own decoders (merge.hip: k_merge_tile_runs_*) then walk - straddled_widths() says what they meet."""
    lists = [ids for _, ids in matrix()]
    terms = [tuple(lists[i:i + k]) for i in range(0, len(lists), k)]
    terms.append(tuple(carrier23(70 + s, 2)[0] for s in range(k)))
    wide = wide_carriers(70, pad=8)
    terms += [tuple(wide[i:i + k]) for i in range(0, N45, k)]
    terms.append(wide_carriers(71)[-k:])
    return tuple(terms)


def straddled_widths(case, t):
    """The gap widths of the blocks of term t that a tile bound of the case's plan cuts in two (merge_cases.tile_ranges)."""
    segs, out = case.segs(), set()
    for r in mc.tile_ranges(case.plan(), segs, t)[1:]:
        if r is None:
            continue
        for l in mc.lists_of(segs, t):
            blk, inside = mc._cut_block(l, r[0])
            if inside:
                out |= set(varint_len(np.diff(l[blk * BLOCK:(blk + 1) * BLOCK].astype(np.int64))).tolist())
    return out


def _removed(segs):
    allv = np.unique(np.concatenate([v for _, v in segs]))
    return allv[2::5]


MERGE_CASES = [mc.Case(f"varint_{kind}_k{k}", (lambda f=f, k=k: _aligned(f(k), k)), _removed, encoding=True, options=opt)
               for kind, f, opt in (("small_terms", merge_small_terms, None), ("tiles", merge_tile_terms, {"merge.large_tile": 1000})) for k in (2, 5)]
