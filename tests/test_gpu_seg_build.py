"""GPU: ii2_seg_build (seg_build.hip) - one segment from unordered (list, value) pairs by a device radix sort.

The reference is numpy: np.unique(list_id << 32 | value), cut per list.  Every case compares the decoded lists, the DV1
arrays byte for byte against the encoder's for the same lists in CSR form (what Context.encode_lists passes to
ii2_seg_encode), and the call's statistics."""
import ctypes as C
import threading

import numpy as np
import pytest

from inverted_index_2_amd import Context, II2Error
from inverted_index_2_amd._lib import II2_DEVICE
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

TILE = 4096      # keys per workgroup of the sort (SB_TILE); the sizes of test_sizes_around_every_boundary bracket it


def expected_csr(lid, val, n_lists):
    keys = np.unique(lid.astype(np.uint64) << np.uint64(32) | val.astype(np.uint64))
    po = np.searchsorted(keys >> np.uint64(32), np.arange(n_lists + 1, dtype=np.uint64)).astype(np.uint64)
    return po, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def n_passes_for(n_lists, n_pairs):
    return 0 if n_pairs == 0 else (32 + int(n_lists - 1).bit_length() + 7) // 8


def same_export(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a.export(), b.export()))


def check_stats(st, n_pairs, n_lists, po):
    assert (st.n_pairs, st.n_postings) == (n_pairs, int(po[-1]))
    assert st.n_nonempty == int(np.count_nonzero(np.diff(po.astype(np.int64))))
    assert st.n_passes == n_passes_for(n_lists, n_pairs)


def check(ctx, lid, val, n_lists, built=None):
    lid, val = np.asarray(lid, np.uint32), np.asarray(val, np.uint32)
    seg, st = built if built is not None else ctx.build_segment(lid, val, n_lists)
    po, uv = expected_csr(lid, val, n_lists)
    got_po, got_v = seg.decode()
    assert np.array_equal(got_po, po) and np.array_equal(got_v, uv)
    assert same_export(seg, ctx.encode(po, uv))
    check_stats(st, lid.size, n_lists, po)
    return seg, po, uv


def test_hand_case(ctx):
    pairs = [(1, 5), (0, 7), (1, 5), (1, 2), (0, 0), (2, 2**32 - 1)]
    lid, val = [p[0] for p in pairs], [p[1] for p in pairs]
    seg, st = ctx.build_segment(lid, val, 4)
    po, v = seg.decode()
    assert [v[po[i]:po[i + 1]].tolist() for i in range(4)] == [[0, 7], [2, 5], [2**32 - 1], []]
    assert (st.n_pairs, st.n_postings, st.n_nonempty) == (6, 5, 3)
    check(ctx, lid, val, 4, built=(seg, st))
    assert same_export(seg, ctx.encode_lists([[0, 7], [2, 5], [2**32 - 1], []]))


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, TILE - 1, TILE, TILE + 1, 8191,
                               8192, 8193, 16383, 16384, 16385, 3 * 16384 + 5])
def test_sizes_around_every_boundary(ctx, n):
    rng = np.random.default_rng(n)
    # 7 lists, values < 5000: the pairs collide often, so runs of duplicates cross wave and tile ends
    check(ctx, rng.integers(0, 7, n), rng.integers(0, 5000, n), 7)


@pytest.mark.parametrize("n_lists", [1, 2, 256, 257, 65536, 65537, 2**24 + 1])
def test_pass_counts(ctx, n_lists):
    rng = np.random.default_rng(n_lists)
    lid = rng.integers(0, n_lists, 3000).astype(np.uint32)
    lid[17], lid[2041] = 0, n_lists - 1
    val = rng.integers(0, 2**32, 3000, dtype=np.uint64).astype(np.uint32)
    assert n_passes_for(1, 1) == 4 and n_passes_for(2**24 + 1, 1) == 8
    if n_lists <= 65537:
        check(ctx, lid, val, n_lists)      # (its statistics include the pass count)
        return
    # 2^24 + 1 lists: the statistics, the postings and the offsets of the non-empty lists only
    seg, st = ctx.build_segment(lid, val, n_lists)
    po, uv = expected_csr(lid, val, n_lists)
    assert st.n_passes == 8
    check_stats(st, 3000, n_lists, po)
    got_po, got_v = seg.decode()
    assert np.array_equal(got_v, uv)
    ne = np.unique(lid).astype(np.int64)
    assert np.array_equal(got_po[ne], po[ne]) and np.array_equal(got_po[ne + 1], po[ne + 1])
    assert got_po[0] == 0 and got_po[-1] == uv.size


def _order_cases():
    rng = np.random.default_rng(7)
    n = 20_000
    lid = rng.integers(0, 300, n).astype(np.uint32)
    val = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    order = np.argsort(lid.astype(np.uint64) << np.uint64(32) | val, kind="stable")
    yield "sorted", lid[order], val[order], 300
    yield "reversed", lid[order][::-1], val[order][::-1], 300
    yield "identical", np.full(n, 211, np.uint32), np.full(n, 123_456_789, np.uint32), 300
    yield "one_list", np.zeros(n, np.uint32), val, 1
    yield "extreme_values", lid, np.where(rng.random(n) < 0.5, 0, 2**32 - 1).astype(np.uint32), 300
    yield "same_low_24_bits", lid, (rng.integers(0, 256, n).astype(np.uint32) << np.uint32(24)) | np.uint32(0xABCDEF), 300
    # one digit bucket holds everything in three of the value passes
    yield "same_high_24_bits", lid, np.uint32(0x5A17C300) | rng.integers(0, 256, n).astype(np.uint32), 300


@pytest.mark.parametrize("name", ["sorted", "reversed", "identical", "one_list", "extreme_values", "same_low_24_bits", "same_high_24_bits"])
def test_orders_and_degenerate_inputs(ctx, name):
    lid, val, n_lists = next(c[1:] for c in _order_cases() if c[0] == name)
    _, po, _ = check(ctx, lid, val, n_lists)
    if name == "identical":
        assert po[-1] == 1


def test_stability_many_repeated_high_digits(ctx):
    # every one of the upper six digits of a key takes only 16 values: an unstable pass would show
    rng = np.random.default_rng(11)
    n, n_lists = 200_000, 2**24
    lists16 = rng.choice(n_lists, 16, replace=False).astype(np.uint32)
    r16 = rng.choice(2**24, 16, replace=False).astype(np.uint32)
    for byte in range(3):
        assert np.unique((lists16 >> (8 * byte)) & 0xFF).size > 1 and np.unique((r16 >> (8 * byte)) & 0xFF).size > 1
    lid = lists16[rng.integers(0, 16, n)]
    val = (r16[rng.integers(0, 16, n)] << np.uint32(8)) | rng.integers(0, 256, n).astype(np.uint32)
    _, po, _ = check(ctx, lid, val, n_lists)
    assert po[-1] > 16 * 16 * 200      # (nearly all of the 65536 possible keys occur)


def test_many_tiles(ctx):
    # more tiles than the device has CUs; one list of exactly 256 postings (one full DV1 block), others longer
    rng = np.random.default_rng(13)
    n, n_lists = 1_500_000, 1000
    lid = rng.integers(0, n_lists, n).astype(np.uint32)
    val = rng.integers(0, 2**20, n).astype(np.uint32)
    lid[lid == 7] = 8
    v256 = rng.choice(2**20, 256, replace=False).astype(np.uint32)
    at = rng.choice(n, 300, replace=False)
    lid[at], val[at] = 7, np.concatenate([v256, v256[:44]])
    assert n // TILE > 256
    _, po, _ = check(ctx, lid, val, n_lists)
    cnt = np.diff(po.astype(np.int64))
    assert cnt[7] == 256 and cnt.max() > 256


def test_device_inputs(ctx):
    rng = np.random.default_rng(17)
    n, n_lists = 50_000, 5000
    lid = rng.integers(0, n_lists, n).astype(np.uint32)
    val = rng.integers(0, 100_000, n).astype(np.uint32)
    d_lid, d_val = ctx.empty(n).upload(lid), ctx.empty(n).upload(val)
    built = ctx.build_segment(d_lid, d_val, n_lists, where=II2_DEVICE)
    seg, _, _ = check(ctx, lid, val, n_lists, built=built)
    assert same_export(seg, ctx.build_segment(lid, val, n_lists)[0])
    assert np.array_equal(d_lid.download(), lid) and np.array_equal(d_val.download(), val)      # inputs are read-only


def _live_bytes(ctx):
    live = C.c_uint64()
    ctx.lib.ii2_devmem_stats(C.byref(live), None)
    return live.value


def test_errors_leave_nothing_behind(ctx):
    rng = np.random.default_rng(19)
    n, n_lists = 10_000, 40
    lid = rng.integers(0, n_lists, n).astype(np.uint32)
    val = rng.integers(0, 1000, n).astype(np.uint32)
    check(ctx, lid, val, n_lists)
    before = _live_bytes(ctx)
    bad = lid.copy()
    bad[4321] = n_lists
    with pytest.raises(II2Error) as e:
        ctx.build_segment(bad, val, n_lists)
    assert e.value.code == -1 and "list_id[4321]" in str(e.value) and "n_lists" in str(e.value)
    assert _live_bytes(ctx) == before
    check(ctx, lid, val, n_lists)
    assert _live_bytes(ctx) == before
    with pytest.raises(II2Error) as e:
        ctx.build_segment(np.zeros(5, np.uint32), val[:5], 0)
    assert e.value.code == -1
    assert _live_bytes(ctx) == before
    check(ctx, lid, val, n_lists)
    # no pairs: the segment of n_lists empty lists, with or without lists
    seg, st = ctx.build_segment([], [], 3)
    assert same_export(seg, ctx.encode_lists([[], [], []])) and (st.n_pairs, st.n_postings, st.n_nonempty, st.n_passes) == (0, 0, 0, 0)


def test_built_segment_is_first_class(ctx):
    rng = np.random.default_rng(23)
    n, n_lists = 30_000, 12
    lid = rng.integers(0, n_lists, n).astype(np.uint32)
    val = rng.integers(0, 200_000, n).astype(np.uint32)
    seg, po, uv = check(ctx, lid, val, n_lists)
    merged, st = ctx.merge_to_segment([seg, seg])
    m_po, m_v = merged.decode()
    assert np.array_equal(m_po, po) and np.array_equal(m_v, uv) and st.n_out == uv.size
    out, cnt = ctx.union([(seg, 2), (seg, 9)])
    assert np.array_equal(out.download(cnt), np.union1d(uv[po[2]:po[3]], uv[po[9]:po[10]]))
    again = ctx.import_dv1(int(po[-1]), *seg.export())
    a_po, a_v = again.decode()
    assert np.array_equal(a_po, po) and np.array_equal(a_v, uv)


def test_two_contexts_on_two_threads(ctx):
    workers = [Context(0), Context(0)]
    inputs = []
    for i in range(2):
        rng = np.random.default_rng(100 + i)
        n = 60_000 + 777 * i
        inputs.append((rng.integers(0, 900, n).astype(np.uint32), rng.integers(0, 50_000, n).astype(np.uint32), 900))
    want = [expected_csr(*inp) for inp in inputs]
    errors, barrier = [], threading.Barrier(2)

    def run(i):
        try:
            c = workers[i]
            barrier.wait()
            for rep in range(5):
                lid, val, n_lists = inputs[(i + rep) % 2]
                seg, st = c.build_segment(lid, val, n_lists)
                po, v = seg.decode()
                w_po, w_v = want[(i + rep) % 2]
                assert np.array_equal(po, w_po) and np.array_equal(v, w_v), (i, rep)
                check_stats(st, lid.size, n_lists, w_po)
                seg.free()
        except BaseException as e:  # noqa: BLE001
            errors.append((i, repr(e)))

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for c in workers:
        c.close()
