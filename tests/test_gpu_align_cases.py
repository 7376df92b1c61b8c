"""GPU: the alignment's case table (tests/align_cases.py) through the kernels of csrc/align.hip.  Every case goes through both
entry points (ii2_align_terms on flat host arrays, ii2_dict_create + ii2_align_dicts on resident dictionaries), in the given and
in the reversed order of its dictionaries, and must give Python's union (sorted(set(...)) of bytes = bytes.Compare order), the
whole table of which term of which dictionary is which union term, and representatives that are the union's terms.  Four cases
then carry posting lists: the aligned views built on the device, one by one and all at once, and the view selected on the host
from Python's table must merge to what numpy computes.  tests/test_align_cases_cpu.py proves, without a GPU, that every case
reaches the branch of the ranking kernel it is there for."""
import random

import numpy as np
import pytest

from tests import align_cases as ac
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def check(al, dicts, flat=None):
    """the alignment equals Python's: size, union terms through the representatives, the whole src table"""
    union, src = ac.expected(dicts)
    got_terms, got_src = al.export()
    if flat is not None:                    # (dictionaries the wrapper holds no terms of: export() hands out the representatives)
        rep = np.asarray(got_terms, np.int64)
        assert rep.size == 0 or (0 <= rep.min() and rep.max() < len(flat))
        got_terms = [flat[int(g)] for g in rep]
    assert al.n_union == len(union) and al.k == len(dicts)
    assert got_terms == union                                   # rep[u] names an input term equal to union term u
    assert got_src.shape == src.shape and np.array_equal(got_src, src)


@pytest.mark.parametrize("name", ac.NAMES)
def test_both_entry_points_equal_python(ctx, name):
    case = ac.table()[name]
    orders = [case.dicts] if name.startswith("k64") else [case.dicts, case.dicts[::-1]]
    for dicts in orders:
        al = ctx.align_terms(dicts)
        check(al, dicts)
        al.free()
        res = [ctx.dictionary(d) for d in dicts]
        al = ctx.align_dicts(res)
        check(al, dicts)
        al.free()
        for d in res:
            d.free()


@pytest.mark.parametrize("name", ["short-ties-staged", "long-ties-global"])
def test_dictionaries_built_on_the_device_align_alike(ctx, name):
    """ii2_dict_build makes the dictionaries from shuffled, repeated terms: the same keys, offsets and long-terms flag"""
    case = ac.table()[name]
    rng = random.Random(5)
    res = []
    for d in case.dicts:
        occ = d + [rng.choice(d) for _ in range(len(d) // 2)]
        rng.shuffle(occ)
        built, _, st = ctx.build_dictionary(occ, want_ids=False)
        assert st.n_unique == len(d)
        res.append(built)
    flat = [t for r in res for t in r.export()]
    assert flat == [t for d in case.dicts for t in d]
    for order in (slice(None), slice(None, None, -1)):
        dicts, rs = case.dicts[order], res[order]
        al = ctx.align_dicts(rs)
        check(al, dicts, flat=[t for d in dicts for t in d])
        al.free()


# ---- aligned views ----
SIZES = (0, 1, 255, 256, 257, 700)          # ids per list, cycling: an empty list, one id, one block less one, a full block, one more, three blocks
DOCS = 40_000                               # the dictionaries' lists draw their ids below this ...
ELSE = (50_000, 60_000)                     # ... and the unrelated lists around them from here
FIRST = 2                                   # unrelated lists in front of a dictionary's lists (and as many behind)


def _list(rng, n, lo, hi):
    if n == 0:
        return np.empty(0, np.uint32)
    return np.sort(rng.choice(hi - lo, n, replace=False)).astype(np.uint32) + np.uint32(lo)


def numpy_merge(dicts, lists, src, removed):
    """(offsets u64 [n_union + 1], ids) of the merge: for union term u the np.unique of its source lists, minus the removed ids"""
    n_union = src.shape[1]
    keys = []
    for s in range(len(dicts)):
        for u in np.flatnonzero(src[s] >= 0):
            l = lists[s][int(src[s, u])]
            keys.append(l.astype(np.uint64) | (np.uint64(u) << np.uint64(32)))
    keys = np.unique(np.concatenate(keys)) if keys else np.empty(0, np.uint64)
    ids = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    keep = ~np.isin(ids, removed)
    keys, ids = keys[keep], ids[keep]
    off = np.zeros(n_union + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount((keys >> np.uint64(32)).astype(np.int64), minlength=n_union))
    return off, ids


@pytest.mark.parametrize("name", ac.VIEW_CASES)
def test_aligned_views_merge_like_numpy(ctx, name):
    case = ac.table()[name]
    dicts = case.dicts
    k = len(dicts)
    rng = np.random.default_rng(len(name))
    lists, segs = [], []
    at = 0
    for d in dicts:
        ls = []
        for _ in d:                                           # (the sizes cycle through the whole case, not per dictionary)
            ls.append(_list(rng, SIZES[at % len(SIZES)], 0, DOCS))
            at += 1
        around = [_list(rng, n, *ELSE) for n in (300, 1, 257, 40)]
        lists.append(ls)
        segs.append(ctx.encode_lists(around[:FIRST] + ls + around[FIRST:]))
    assert any(l.size == 0 for ls in lists for l in ls) and any(l.size == 700 for ls in lists for l in ls)
    assert max(int(l.max()) for ls in lists for l in ls if l.size) < DOCS <= ELSE[0]
    union, src = ac.expected(dicts)
    al = ctx.align_terms(dicts)
    check(al, dicts)
    first = np.full(k, FIRST, np.uint64)
    one_by_one = [ctx.select_aligned(segs[s], al, s, first_list=FIRST) for s in range(k)]
    at_once = ctx.select_aligned_all(segs, al, first_list=first)
    by_host = [ctx.select(segs[s], np.where(src[s] >= 0, src[s] + FIRST, -1)) for s in range(k)]
    removed = np.unique(rng.integers(0, DOCS, 3000)).astype(np.uint32)
    tomb = ctx.tombstones(removed)
    for rem, tb in ((np.empty(0, np.uint32), None), (removed, tomb)):
        want_off, want_ids = numpy_merge(dicts, lists, src, rem)
        assert want_ids.size and int(want_ids.max()) < DOCS
        for how, views in (("one by one", one_by_one), ("at once", at_once), ("by host", by_host)):
            assert all(v.info.n_lists == len(union) for v in views)
            out_off, out_vals, st = ctx.merge(views, tb)
            got_off = out_off.download()
            assert int(st.n_out) == want_ids.size and np.array_equal(got_off, want_off), (how, tb is not None)
            got = out_vals.download(int(st.n_out))
            assert got.size == 0 or int(got.max()) < ELSE[0], "ids of lists outside the dictionary's slice"
            assert np.array_equal(got, want_ids), (how, tb is not None)
    for v in one_by_one + at_once + by_host + segs:
        v.free()
    tomb.free()
    al.free()
