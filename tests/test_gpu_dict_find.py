"""GPU: ii2_dict_find (csrc/dict_find.hip) - every case of tests/dict_cases.py through the kernel, with host arrays and with
device arrays; n_found; every argument error with the outputs verified untouched; and
the returned ranges fed verbatim to ii2_query_batch_groups against ranges resolved in Python."""
import ctypes as C

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from inverted_index_2_amd.engine import DeviceArray, II2Error
from tests import dict_cases
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

FILL = 0xABABABABABABABAB


@pytest.fixture(scope="module")
def resident(ctx):
    """the dictionaries of every case, made resident once"""
    made = {c.name: [ctx.dictionary(d) for d in c.dicts] for c in dict_cases.CASES}
    yield made
    for dicts in made.values():
        for d in dicts:
            d.free()


@pytest.fixture(scope="module")
def want():
    return {c.name: dict_cases.expected_table(c) for c in dict_cases.CASES}


def _probe_arrays(case):
    blob, off = dict_cases.flat(case.probes)
    return np.frombuffer(blob, np.uint8).copy(), np.array(off, np.uint64), np.array(case.flags, np.uint8)


@pytest.mark.parametrize("case", dict_cases.CASES, ids=lambda c: c.name)
def test_host_arrays(ctx, resident, want, case):
    blob, off, flags = _probe_arrays(case)
    first, end, found = ctx.dict_find_flat(resident[case.name], blob, off, flags)
    w_first, w_end, w_found = want[case.name]
    assert first.tolist() == w_first and end.tolist() == w_end and found == w_found
    if not any(case.flags):                                    # NULL flags: all exact
        first, end, found = ctx.dict_find_flat(resident[case.name], blob, off, None)
        assert first.tolist() == w_first and end.tolist() == w_end and found == w_found


@pytest.mark.parametrize("case", dict_cases.CASES, ids=lambda c: c.name)
def test_device_arrays(ctx, resident, want, case):
    blob, off, flags = _probe_arrays(case)
    n = len(case.probes) * len(case.dicts)
    d_blob, d_off, d_flags = DeviceArray(ctx, blob.size, np.uint8).upload(blob), DeviceArray(ctx, off.size, np.uint64).upload(off), \
        DeviceArray(ctx, flags.size, np.uint8).upload(flags)
    d_first, d_end = DeviceArray(ctx, n, np.uint64), DeviceArray(ctx, n, np.uint64)
    _, _, found = ctx.dict_find_flat(resident[case.name], d_blob, d_off, d_flags, _lib.II2_DEVICE, d_first, d_end)
    w_first, w_end, w_found = want[case.name]
    assert d_first.download().tolist() == w_first and d_end.download().tolist() == w_end and found == w_found
    for a in (d_blob, d_off, d_flags, d_first, d_end):
        a.free()


def test_many_workgroups(ctx):
    """hundreds of workgroups per dictionary, the last one short"""
    terms = dict_cases._ternary(3000, 11)
    dicts = [ctx.dictionary(terms[s::3]) for s in range(3)]
    rng = np.random.default_rng(5)
    probes = [terms[int(i)] for i in rng.integers(0, len(terms), 100_000 + 77)]
    case = dict_cases.Case("wide", [terms[s::3] for s in range(3)], probes, [0] * len(probes))
    first, end, found = ctx.dict_find(dicts, probes)
    w_first, w_end, w_found = dict_cases.expected_table(case)
    assert first.ravel().tolist() == w_first and end.ravel().tolist() == w_end and found == w_found == len(probes)
    for d in dicts:
        d.free()


def test_no_probes_and_dictionary_find(ctx):
    d = ctx.dictionary([b"a", b"ab", b"b"])
    found = C.c_uint64(9)
    arr = (C.c_void_p * 1)(d.h)
    assert ctx.lib.ii2_dict_find(ctx.h, 1, arr, 0, None, None, None, 0, None, None, C.byref(found)) == 0 and found.value == 0
    first, end = d.find([b"a", b"aa", b"b", b"c"])
    assert first.tolist() == [0, 1, 2, 3] and end.tolist() == [1, 1, 3, 3]
    first, end = d.find([b"a", b"", b"c"], prefix=True)
    assert first.tolist() == [0, 0, 3] and end.tolist() == [2, 3, 3]
    d.free()


def test_argument_errors_leave_the_outputs_untouched(ctx):
    d = ctx.dictionary([b"a", b"ab", b"b"])
    arr = (C.c_void_p * 2)(d.h, d.h)
    blob = np.frombuffer(b"aabb\0", np.uint8).copy()
    off = np.array([0, 1, 3, 4], np.uint64)
    flags = np.array([0, 1, 0], np.uint8)
    first, end = np.full(6, FILL, np.uint64), np.full(6, FILL, np.uint64)
    found = C.c_uint64(FILL)
    p = lambda a: a.ctypes.data if a is not None else None

    def call(k=2, dicts=arr, n=3, b=blob, o=off, f=flags, where=0, lf=first, le=end):
        return ctx.lib.ii2_dict_find(ctx.h, k, dicts, n, p(b), p(o), p(f), where, p(lf), p(le), C.byref(found))

    def untouched():
        return (first == FILL).all() and (end == FILL).all() and found.value == FILL

    for kw in (dict(dicts=None), dict(b=None), dict(o=None), dict(lf=None), dict(le=None), dict(k=0), dict(k=65), dict(where=2),
               dict(dicts=(C.c_void_p * 2)(d.h, None)),
               dict(o=np.array([1, 1, 3, 4], np.uint64)), dict(o=np.array([0, 3, 1, 4], np.uint64)), dict(f=np.array([0, 2, 0], np.uint8))):
        assert call(**kw) == -1, kw
        assert untouched(), kw
    assert call(n=(1 << 32) // 2) == -5 and untouched()             # n_probes * k = 2^32
    assert call(k=1, n=1 << 32) == -5 and untouched()
    # the same faults in arrays that live on the device: found there, nothing written
    d_blob = DeviceArray(ctx, blob.size, np.uint8).upload(blob)
    d_first, d_end = DeviceArray(ctx, 6, np.uint64).upload(first), DeviceArray(ctx, 6, np.uint64).upload(end)
    for o, f in ((np.array([1, 1, 3, 4], np.uint64), flags), (np.array([0, 3, 1, 4], np.uint64), flags), (off, np.array([0, 1, 7], np.uint8))):
        d_off, d_flags = DeviceArray(ctx, 4, np.uint64).upload(o), DeviceArray(ctx, 3, np.uint8).upload(f)
        with pytest.raises(II2Error) as e:
            ctx.dict_find_flat([d, d], d_blob, d_off, d_flags, _lib.II2_DEVICE, d_first, d_end)
        assert e.value.code == -1
        assert (d_first.download() == FILL).all() and (d_end.download() == FILL).all()
    import torch
    if torch.cuda.device_count() > 1:                                  # a dictionary of another device (where there is one)
        from inverted_index_2_amd import Context
        other = Context(1)
        foreign = other.dictionary([b"a"])
        assert call(dicts=(C.c_void_p * 2)(d.h, foreign.h)) == -1 and untouched()
        foreign.free()
        other.close()
    assert call() == 0 and found.value == 6 and first.tolist() == [0, 0, 1, 1, 2, 2] and end.tolist() == [1, 1, 2, 2, 3, 3]
    d.free()


def test_ranges_feed_query_batch_groups_verbatim(ctx):
    """terms -> ii2_dict_find -> ii2_query_batch_groups with group_first[g] = g * k and the k segments tiled, against the same
    batch with the ranges resolved in Python and packed by the engine, and against plain sets"""
    rng = np.random.default_rng(21)
    vocab = dict_cases._ternary(120, 7)
    k = 3
    terms_of = [sorted(vocab[int(i)] for i in rng.choice(len(vocab), n, replace=False)) for n in (90, 60, 25)]
    lists_of = [[np.unique(rng.integers(0, 4000, int(rng.integers(1, 400)))).astype(np.uint32) for _ in terms] for terms in terms_of]
    segs = [ctx.encode_lists(lists) for lists in lists_of]
    dicts = [ctx.dictionary(terms) for terms in terms_of]
    queries = [[vocab[int(i)] for i in rng.choice(len(vocab), int(rng.integers(1, 4)), replace=False)] for _ in range(40)]
    queries[3] = [vocab[0], b"absent-term"]
    flat_terms = [t for q in queries for t in q]
    first, end, _ = ctx.dict_find(dicts, flat_terms)
    n_groups = len(flat_terms)
    query_first = np.zeros(len(queries) + 1, np.uint64)
    query_first[1:] = np.cumsum([len(q) for q in queries])
    group_first = (np.arange(n_groups + 1) * k).astype(np.uint64)
    group_not = np.zeros(n_groups, np.uint8)
    seg_arr = (C.c_void_p * (n_groups * k))(*[s.h for _ in range(n_groups) for s in segs])
    lf, le = np.ascontiguousarray(first.ravel()), np.ascontiguousarray(end.ravel())
    out = ctx.empty(len(queries) * 4000)
    off = np.zeros(len(queries) + 1, np.uint64)
    u64 = lambda a: a.ctypes.data_as(_lib.u64p)
    ctx._ck(ctx.lib.ii2_query_batch_groups(ctx.h, len(queries), u64(query_first), u64(group_first), group_not.ctypes.data_as(_lib.u8p), seg_arr,
                                           u64(lf), u64(le), None, out.ptr, out.count, u64(off)))
    got = out.download(int(off[-1]))
    # the same batch from Python's own lookup, through the packer
    resolved = []
    for q in queries:
        groups = []
        for t in q:
            held = [(segs[s], terms_of[s].index(t), terms_of[s].index(t) + 1) for s in range(k) if t in terms_of[s]]
            groups.append(held or [(segs[0], 0, 0)])
        resolved.append((groups, []))
    out2, off2 = ctx.query_batch_groups(resolved)
    assert off.tolist() == off2.tolist() and got.tolist() == out2.download(int(off2[-1])).tolist()
    assert int(off[4]) == int(off[3]) and int(off[-1]) > 0                 # the absent term empties its query; others do not
    # ... and against plain sets
    for qi, q in enumerate(queries):
        docs = None
        for t in q:
            under = set()
            for s in range(k):
                if t in terms_of[s]:
                    under |= set(lists_of[s][terms_of[s].index(t)].tolist())
            docs = under if docs is None else docs & under
        assert got[int(off[qi]):int(off[qi + 1])].tolist() == sorted(docs), qi
    for x in segs + dicts:
        x.free()
