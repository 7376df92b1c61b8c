"""GPU: PutBatch of the host mirror (host/host_index.cpp) - many puts as ONE merged-quality segment per shard, built by
ii2_seg_build - against the reference model (oracle/ref_model.py), which takes the same docs as single puts."""
import numpy as np
import pytest

from oracle import oracle as orc
from oracle import ref_model
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def _ints(read):
    return [(t, [int(v) for v in vs]) for t, vs in read]


def _workload(seed, n_docs, n_vocab=120, max_val=60):
    # the workload of test_gpu_host_mirror.py::test_random_workload_matches_reference_model
    rng = np.random.default_rng(seed)
    vocab = [bytes(rng.choice(list(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"), int(rng.integers(2, 8))).tolist())
             for _ in range(n_vocab)]
    docs = [([vocab[i] for i in rng.choice(len(vocab), int(rng.integers(1, 6)), replace=False)], int(rng.integers(0, max_val)))
            for _ in range(n_docs)]
    return vocab, docs


def test_index_put_batch_matches_single_puts(ctx):
    from inverted_index_2_amd.host import InvertedIndex
    vocab, docs = _workload(42, 170)
    first, later = docs[:150], docs[150:]
    gpu, ref = InvertedIndex(ctx), ref_model.InvertedIndex()
    gpu.put_batch(first)
    for terms, val in first:
        ref.put(list(terms), val)
    assert gpu.read() == _ints(ref.read())
    assert gpu.read(b"b", b"q") == _ints(ref.read(b"b", b"q"))
    assert gpu.prefix_search([b"a", b"Zq", b"m"]) == ref.prefix_search([b"a", b"Zq", b"m"])
    model = {t: set(int(v) for v in vs) for t, vs in ref.read()}
    # the pair of terms with the largest intersection, and the term that removes most of it
    t1, t2 = max(((x, y) for x in model for y in model if x < y), key=lambda p: len(model[p[0]] & model[p[1]]))
    both = model[t1] & model[t2]
    t3 = max((t for t in model if t not in (t1, t2)), key=lambda t: len(both & model[t]))
    assert both and both & model[t3] and both - model[t3]      # (neither query is trivial)
    assert gpu.intersect([t1, t2]) == sorted(both)
    assert gpu.intersect_except([t1, t2], [t3]) == sorted(both - model[t3])
    # one segment per shard that received a term
    assert gpu.n_shards == len({orc.shard_key(t) for terms, _ in first for t in terms})
    assert gpu.n_segments == gpu.n_shards
    # single puts on top, then everything merged down (the segment counts differ by design: no return value is compared)
    for terms, val in later:
        gpu.put(list(terms), val)
        ref.put(list(terms), val)
    assert gpu.n_segments > gpu.n_shards
    while gpu.merge(2, 100, 2):
        pass
    while ref.merge(2, 100, 2):
        pass
    assert gpu.read() == _ints(ref.read())
    gpu.close()


def test_shard_put_batch_with_removals(ctx):
    from inverted_index_2_amd.host import Shard
    rng = np.random.default_rng(5)
    vocab = [b"t%02d" % i for i in range(30)]
    a = [([vocab[i] for i in rng.choice(29, 4, replace=False)], int(rng.integers(0, 40))) for _ in range(60)]
    b = [([vocab[i] for i in rng.choice(29, 4, replace=False)], int(rng.integers(0, 40))) for _ in range(60)]
    b.append(([vocab[29]], 3))           # a term whose only value is removed ...
    b.append(([vocab[29]], 11))
    removed = [3, 11, 17]
    gpu, ref = Shard(ctx), ref_model.Shard()
    gpu.put_batch(a)
    gpu.put_batch(b)
    assert gpu.n_segments == 2
    for terms, val in a + b:
        ref.put(list(terms), val)
    before = dict(_ints(ref.read()))
    gpu.remove(removed)
    ref.remove(removed)
    assert gpu.merge(2, 100) == 2 and gpu.n_segments == 1
    while ref.merge(2, 100):
        pass
    after = dict(_ints(ref.read()))
    assert vocab[29] in before and vocab[29] not in after                                   # one term lost all its values
    assert any(t in after and 0 < len(after[t]) < len(before[t]) for t in before)           # ... and one lost some
    assert gpu.read() == _ints(ref.read())
    gpu.close()


def test_put_batch_persists(ctx, tmp_path):
    from inverted_index_2_amd.host import InvertedIndex
    _, docs = _workload(9, 80)
    gpu = InvertedIndex(ctx, str(tmp_path))
    gpu.put_batch(docs)
    want = gpu.read()
    n_seg = gpu.n_segments
    gpu.close()
    again = InvertedIndex(ctx, str(tmp_path))
    assert again.read() == want and again.n_segments == n_seg
    ref = ref_model.InvertedIndex()
    for terms, val in docs:
        ref.put(list(terms), val)
    assert want == _ints(ref.read())
    again.close()


def test_put_batch_edge_cases(ctx):
    from inverted_index_2_amd.host import InvertedIndex, Shard
    s = Shard(ctx)
    s.put_batch([])
    assert s.n_segments == 0
    s.put_batch([([], 3)])
    assert s.n_segments == 0 and s.read() == []
    doc = ([b"alpha", b"beta"], 9)
    s.put_batch([doc, ([b"beta"], 2)])
    one = s.read()
    assert one == [(b"alpha", [9]), (b"beta", [2, 9])] and s.n_segments == 1
    twice = Shard(ctx)
    twice.put_batch([doc, doc, ([b"beta"], 2), ([b"beta", b"beta"], 2)])
    assert twice.read() == one and twice.n_segments == 1
    ii = InvertedIndex(ctx)
    ii.put_batch([])
    ii.put_batch([([], 1)])
    assert ii.n_shards == 0 and ii.read() == []
    for t in (s, twice, ii):
        t.close()
