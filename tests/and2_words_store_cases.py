"""The pairs of lists that pin where the word-by-word two-list AND (csrc/intersect_words.hip k_and2_words) puts its ids, for the
options intersect.and2_words_store (0 plain stores, 1 write-through stores at 16-byte-aligned addresses: a head of single ids, the
aligned body, a tail) and intersect.and2_words_order (0 both chunks of a wave staged before the first store, 1 chunk 0's stores
first).  tests/test_and2_words_store_cpu.py proves the table sound without a device,
tests/test_gpu_and2_words_store.py runs it.

Every pair is (structure, all docs of the same span): the result is the structure, and the structure is made of all-ones
stretches of words, all-zero stretches and single docs - `run(first doc, docs)` - so every count below is exact by construction.
A workgroup owns W = 2048 words of the window (65 536 docs), a wave 512 of them, a chunk 256 (8192 docs); a chunk's ids leave in
rounds of S = 1536 (AW_STAGE).  The one-launch AND wants >= 1024 blocks in its shorter list: an all-ones tail of five workgroups."""
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

from tests import and2_words_cases as wc
from tests import dense_form_cases as dc

W = wc.W
WG_DOCS = wc.WG_DOCS
WAVE_DOCS = WG_DOCS // 4
CHUNK_DOCS = WAVE_DOCS // 2
S = 1536                        # ids a stage round holds (csrc/intersect_words.hip: AW_STAGE)
FILLER_WGS = 5                  # 5 x 65 536 postings = 1280 blocks


def run(first, n):
    return np.arange(first, first + n, dtype=np.uint32)


def pair_of(parts, wgs):
    """(structure + all-ones filler behind `wgs` workgroups, every doc of the span)"""
    span = (wgs + FILLER_WGS) * WG_DOCS
    x = np.concatenate([np.asarray(p, np.uint32) for p in parts] + [run(wgs * WG_DOCS, FILLER_WGS * WG_DOCS)])
    assert np.all(np.diff(x.astype(np.int64)) > 0)
    return x, run(0, span)


def chunk_counts(words):
    """ids of every chunk of the window: [workgroup, wave, chunk]"""
    pad = np.zeros((-words.size) % W, np.uint32)
    bits = np.unpackbits(np.concatenate([words, pad]).astype("<u4").view(np.uint8))
    return bits.reshape(-1, 4, 2, CHUNK_DOCS).sum(axis=3).astype(np.int64)


def chunk_starts(words):
    """place among the result's ids of every chunk's first id: [workgroup, wave, chunk]"""
    cc = chunk_counts(words)
    return (np.cumsum(cc.reshape(-1)) - cc.reshape(-1)).reshape(cc.shape)


def round_layout(pos, n):
    """(head, body, tail) ids of a round of n ids whose first one goes to place `pos`: the 16-byte stores start at a multiple of 4"""
    h = min((-pos) % 4, n)
    nb = (n - h) // 4 * 4
    return h, nb, n - h - nb


# ---- offset residues: workgroup 2k holds the docs that shift the places by one, workgroup 2k + 1 is all ones but for the
# first R1(k) docs of wave 1's chunk 0 and the first R2(k) of wave 2's chunk 0
RESIDUES = 32


def R1(k):
    return (2 * k + 1) % 32


def R2(k):
    return (4 * k) % 32


def _residues():
    parts = []
    for k in range(RESIDUES):
        g0, g1 = 2 * k * WG_DOCS, (2 * k + 1) * WG_DOCS
        # one id more than the all-ones workgroup before this one lacks: workgroup 2k + 1 starts at residue k (k = 0: 32 ids from
        # doc 0 on, the window starts at word 0)
        parts.append(run(g0, (1 + R1(k - 1) + R2(k - 1)) % 32 if k else 32))
        parts.append(run(g1, WAVE_DOCS))
        parts.append(run(g1 + WAVE_DOCS + R1(k), WAVE_DOCS - R1(k)))
        parts.append(run(g1 + 2 * WAVE_DOCS + R2(k), WAVE_DOCS - R2(k)))
        parts.append(run(g1 + 3 * WAVE_DOCS, WAVE_DOCS))
    return pair_of(parts, 2 * RESIDUES)


def _residues_ok(x, y, r, lo, w):
    st, cc = chunk_starts(w), chunk_counts(w)
    ones = [2 * k + 1 for k in range(RESIDUES)]
    return (lo == 0 and [int(st[g, 0, 0]) % 32 for g in ones] == list(range(32)) and
            all(int(cc[2 * k + 1, 1, 0]) == CHUNK_DOCS - R1(k) for k in range(RESIDUES)) and
            {int(st[g, 1, 1]) % 32 for g in ones} == set(range(32)) and {int(st[g, 2, 0]) % 32 for g in ones} == set(range(32)) and
            {int(st[g, 3, 0]) % 32 for g in ones} == set(range(32)))


def residue_tombstones():
    """one id of the head and one of the body of every all-ones workgroup's first round that has a head, by the reference"""
    x, y = _residues()
    _, w = wc.result_words(x, y)
    st = chunk_starts(w)
    gone = []
    for k in range(RESIDUES):
        p = int(st[2 * k + 1, 0, 0])
        h, nb, _ = round_layout(p, S)
        if h:
            gone += [int(x[p]), int(x[p + h + 9])]
    return np.array(sorted(gone), np.uint32)


def _residues_removed():
    x, y = _residues()
    return x, y, residue_tombstones()


def _residues_removed_ok(x, y, r, lo, w):
    _, w0 = wc.result_words(x, y)
    st = chunk_starts(w0)
    heads = [k for k in range(RESIDUES) if round_layout(int(st[2 * k + 1, 0, 0]), S)[0]]
    return r.size == 2 * len(heads) == 48 and int(chunk_counts(w0).sum() - chunk_counts(w).sum()) == r.size


# ---- round edges: wave i % 4 of workgroup i // 4 holds EDGE_C0[j // 2] ids in chunk 0 and EDGE_C1[j % 2] in chunk 1, j = (i + 2)
# % 12 (the window starts with a doc); then a workgroup whose only ids are in its last half chunk
EDGE_C0 = (0, 1, S - 1, S, S + 1, CHUNK_DOCS)
EDGE_C1 = (0, CHUNK_DOCS)
EDGE_WGS = 4
LAST_HALF = 40                  # ids of workgroup 3, in the last 128 words


def _round_edges():
    parts = []
    for i in range(12):
        d = (i // 4) * WG_DOCS + (i % 4) * WAVE_DOCS
        j = (i + 2) % 12
        parts.append(run(d, EDGE_C0[j // 2]))
        parts.append(run(d + CHUNK_DOCS, EDGE_C1[j % 2]))
    parts.append(run(4 * WG_DOCS - 32 * 100, LAST_HALF))
    return pair_of(parts, EDGE_WGS)


def _round_edges_ok(x, y, r, lo, w):
    cc = chunk_counts(w)
    got = [(int(cc[i // 4, i % 4, 0]), int(cc[i // 4, i % 4, 1])) for i in range(12)]
    return (lo == 0 and got[-2:] + got[:-2] == [(a, b) for a in EDGE_C0 for b in EDGE_C1] and S % 4 == 0 and
            int(cc[3].sum()) == int(cc[3, 3, 1]) == LAST_HALF and not np.any(w[3 * W:4 * W - 128]))


# ---- capacity: two docs, then all ones: every round of the all-ones workgroups has a head of two ids and a tail of two
CAP_WG, CAP_WAVE = 1, 1


def _capacity():
    return pair_of([run(10, 2)], 1)


def capacity_positions(x, y):
    """places inside the head, the aligned body and the tail of the first round of workgroup CAP_WG's wave CAP_WAVE"""
    _, w = wc.result_words(x, y)
    p = int(chunk_starts(w)[CAP_WG, CAP_WAVE, 0])
    h, nb, t = round_layout(p, S)
    return {"head": p + 1, "body": p + h + 6, "tail": p + h + nb + 1}, (p, h, nb, t)


def _capacity_ok(x, y, r, lo, w):
    pos, (p, h, nb, t) = capacity_positions(x, y)
    return lo == 0 and (h, nb, t) == (2, S - 4, 2) and p < pos["head"] < p + h <= pos["body"] < p + h + nb < pos["tail"] < p + S


@dataclass
class Case:
    name: str
    make: Callable[[], tuple]
    check: Callable
    _cache: Optional[tuple] = None

    def data(self):
        if self._cache is None:
            d = self.make()
            self._cache = (d[0], d[1], d[2] if len(d) > 2 else None)
        return self._cache


CASES = [
    Case("residues", _residues, _residues_ok),
    Case("residues_removed", _residues_removed, _residues_removed_ok),
    Case("round_edges", _round_edges, _round_edges_ok),
    Case("capacity", _capacity, _capacity_ok),
]
BY_NAME = {c.name: c for c in CASES}
