"""GPU: PutBatch's device route in the host mirror (host/host_index.cpp, SetBuild): the terms sorted, deduplicated and looked up
by ii2_dict_build, the segment built from the indices that never left the device, the dictionary adopted as the segment's
resident one - against the host route (mode 0) on the same docs: the same Read(), PrefixSearch answers and segment files."""
import os

import numpy as np
import pytest

from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def _docs(seed, n_docs, extra=()):
    rng = np.random.default_rng(seed)
    vocab = [bytes(rng.choice(list(b"abcdefghijklmnopqrstuvwxyz\0\xff"), int(rng.integers(1, 14))).tolist()) for _ in range(150)]
    vocab = sorted(set(vocab)) + list(extra)
    return vocab, [([vocab[i] for i in rng.choice(len(vocab), int(rng.integers(1, 7)), replace=False)], int(rng.integers(0, 90))) for _ in range(n_docs)]


def _files(root):
    """{path below root without the segment key: content} - the keys are time stamps, one segment per shard here"""
    out = {}
    for dirpath, _, names in os.walk(root):
        for name in names:
            with open(os.path.join(dirpath, name), "rb") as f:
                out[(os.path.relpath(dirpath, root), name.split("_")[-1])] = f.read()
    return out


def _both(ctx, docs, tmp_path):
    from inverted_index_2_amd.host import InvertedIndex
    made = []
    for mode in (0, 1):
        os.mkdir(tmp_path / str(mode))
        ii = InvertedIndex(ctx, str(tmp_path / str(mode)))
        ii.set_build(mode)
        ii.put_batch(docs)
        made.append(ii)
    return made


def test_device_route_equals_host_route(ctx, tmp_path):
    vocab, docs = _docs(3, 260)
    host, dev = _both(ctx, docs, tmp_path)
    model = {}
    for terms, val in docs:
        for t in terms:
            model.setdefault(t, set()).add(val)
    assert dev.read() == host.read()
    assert sorted(dev.read()) == [(t, sorted(model[t])) for t in sorted(model)]           # (Read goes shard by shard)
    assert dev.read(b"b", b"q") == host.read(b"b", b"q")
    prefixes = [b"a", b"", b"zz", b"\0", b"m\xff"]
    assert dev.prefix_search(prefixes) == host.prefix_search(prefixes)
    assert dev.n_segments == host.n_segments == dev.n_shards
    f_host, f_dev = _files(tmp_path / "0"), _files(tmp_path / "1")
    assert f_host and f_host == f_dev
    for ii in (host, dev):
        ii.close()


def test_a_long_term_takes_the_host_route(ctx, tmp_path):
    vocab, docs = _docs(4, 80, extra=[b"L" * 300])
    docs.append(([b"L" * 300, vocab[0]], 5))
    host, dev = _both(ctx, docs, tmp_path)
    assert dev.read() == host.read() and any(len(t) == 300 for t, _ in dev.read())
    assert _files(tmp_path / "0") == _files(tmp_path / "1")
    for ii in (host, dev):
        ii.close()


def test_intersect_on_the_adopted_dictionary(ctx, tmp_path):
    """the device lookup of a device-built segment uses the dictionary ii2_dict_build left with it"""
    vocab, docs = _docs(5, 300)
    host, dev = _both(ctx, docs, tmp_path)
    model = {}
    for terms, val in docs:
        for t in terms:
            model.setdefault(t, set()).add(val)
    pairs = sorted(((x, y) for x in model for y in model if x < y), key=lambda p: -len(model[p[0]] & model[p[1]]))[:20]
    queries = [([x, y], []) for x, y in pairs] + [([pairs[0][0], b"absent"], [])]
    want = [sorted(model[x] & model[y]) for x, y in pairs] + [[]]
    assert want[0]
    host.set_resolve(0)
    dev.set_resolve(1)
    assert dev.intersect_batch(queries) == host.intersect_batch(queries) == want
    assert dev.intersect(list(pairs[0])) == want[0]
    for ii in (host, dev):
        ii.close()


def test_mode_is_checked_and_shards_take_it(ctx):
    from inverted_index_2_amd.host import Shard
    s = Shard(ctx)
    for bad in (-2, 2):
        with pytest.raises(Exception):
            s.set_build(bad)
    s.set_build(1)
    s.put_batch([([b"beta", b"alpha", b"beta", b"a\0"], 9), ([b"beta"], 2), ([], 4)])
    assert s.read() == [(b"a\0", [9]), (b"alpha", [9]), (b"beta", [2, 9])] and s.n_segments == 1
    s.put_batch([([], 1)])
    s.put_batch([])
    assert s.n_segments == 1
    s.close()


def test_default_mode_decides_by_size(ctx):
    """mode -1: a batch above the measured threshold (8192 term occurrences) and one below it leave what mode 0 leaves"""
    from inverted_index_2_amd.host import Shard
    for n_docs in (1100, 40):
        _, docs = _docs(6, n_docs)
        docs = [(terms + [b"pad%d" % i for i in range(8 - len(terms))], val) for terms, val in docs]        # 8 terms per doc
        reads = []
        for mode in (-1, 0):
            s = Shard(ctx)
            s.set_build(mode)
            s.put_batch(docs)
            reads.append(s.read())
            s.close()
        assert reads[0] == reads[1] and reads[0]
