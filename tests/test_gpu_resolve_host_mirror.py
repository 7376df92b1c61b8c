"""GPU: the host mirror's two bulk calls, IntersectMany and IntersectTopBatch (host/host_index.cpp), with their terms looked up
on the device (ii2h_set_resolve mode 1: ii2_dict_find on lazily made resident dictionaries) against the host bisection (mode 0):
bit-identical results on an index of 3 shards x 5 unmerged segments, across a put, a removal and a merge - the segments whose
dictionaries were made are replaced - and on a shard of more than II2_MAX_LISTS segments, which takes several lookups."""
import numpy as np
import pytest

from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def _vocab(rng, n=90):
    # two or more bytes, first byte a / b / c, second a lowercase letter: shard key = first two bytes >> 6, one shard per first byte
    out = set()
    while len(out) < n:
        out.add(bytes([int(rng.choice(list(b"abc")))] + [int(rng.choice(list(b"abcxyz"))) for _ in range(int(rng.integers(1, 10)))]))
    return sorted(out)


ABSENT = [b"az-none", b"bznone-longer-than-the-key", b"cq", b"q", b""]


def _pick(rng, vocab, k, p_absent):
    return [ABSENT[int(rng.integers(0, len(ABSENT)))] if rng.random() < p_absent else vocab[int(rng.integers(0, len(vocab)))] for _ in range(k)]


def _queries(rng, vocab, n=200):
    """(terms, exclude): some required terms absent, some excluded terms absent, some queries empty"""
    out = [([], []), ([], [vocab[0]]), ([ABSENT[0]], []), ([vocab[0]], [ABSENT[1]]), ([vocab[0], vocab[1]], [vocab[0]]), ([vocab[5]] * 2, [])]
    while len(out) < n:
        out.append((_pick(rng, vocab, int(rng.integers(1, 4)), 0.06), _pick(rng, vocab, int(rng.integers(0, 3)), 0.2)))
    return out


def _top_queries(rng, pairs):
    out = []
    for terms, exclude in pairs:
        if not terms:
            terms = [ABSENT[2]]
        out.append((terms, [int(rng.integers(1, 40)) for _ in terms], int(rng.integers(0, 12)), int(rng.integers(1, 3)), exclude))
    return out


def _both_modes(gpu, pairs, tops, stage):
    got = {}
    for mode in (0, 1, 0, 1):
        gpu.set_resolve(mode)
        many, top = gpu.intersect_batch(pairs), gpu.intersect_top_batch(tops)
        assert got.setdefault(mode, (many, top)) == (many, top), (stage, mode)      # (the second round: the dictionaries exist)
    assert got[0] == got[1], stage
    assert gpu.intersect_batch([]) == [] and gpu.intersect_top_batch([]) == []
    return got[0]


def test_device_lookup_equals_the_host_bisection(ctx):
    from inverted_index_2_amd.host import HostError, InvertedIndex
    rng = np.random.default_rng(404)
    vocab = _vocab(rng)
    gpu = InvertedIndex(ctx)
    with pytest.raises(HostError):
        gpu.set_resolve(2)
    gpu.set_resolve(1)
    assert gpu.intersect_batch([([vocab[0]], [])]) == [[]]                  # an empty index: no shard, nothing to probe
    for _ in range(5):                                                      # five bulk puts: one segment per shard each
        docs = [([vocab[int(i)] for i in rng.choice(len(vocab), int(rng.integers(3, 12)), replace=False)], int(rng.integers(0, 3000)))
                for _ in range(120)]
        gpu.put_batch(docs)
    assert gpu.n_shards == 3 and gpu.n_segments == 15
    pairs = _queries(rng, vocab)
    tops = _top_queries(rng, pairs)
    many, top = _both_modes(gpu, pairs, tops, "unmerged")
    assert sum(bool(r) for r in many) > 60 and sum(bool(r) for r in top) > 60 and not many[0] and not many[2] and many[3]
    assert many[:40] == [gpu.intersect_except(t, x) for t, x in pairs[:40]]
    # a put, a removal and a merge: segments that own a resident dictionary go, a merged one without one arrives
    gpu.set_resolve(1)
    gpu.put([vocab[0], vocab[40], vocab[80], b"ab-new-term"], 2999)
    gpu.put_removed([int(v) for v in rng.integers(0, 3000, 200)])
    assert gpu.intersect_batch([([b"ab-new-term"], [])]) == [[2999]]
    before = gpu.n_segments
    assert gpu.merge(2, 4, 1) > 0
    assert gpu.n_segments < before
    many2, _ = _both_modes(gpu, pairs + [([b"ab-new-term"], [])], tops, "merged")
    assert sum(bool(r) for r in many2) > 40
    gpu.set_resolve(-1)                                                     # the default decides by the call's size: same results
    assert gpu.intersect_batch(pairs) == many2[:-1]
    gpu.close()


def test_a_shard_of_more_than_64_segments_takes_several_lookups(ctx):
    from inverted_index_2_amd.host import InvertedIndex
    rng = np.random.default_rng(405)
    vocab = [t for t in _vocab(rng, 60) if t[:1] == b"a"]
    gpu = InvertedIndex(ctx)
    for v in range(70):                                                     # every put is a segment of its own
        gpu.put([vocab[int(i)] for i in rng.choice(len(vocab), 4, replace=False)], v)
    assert gpu.n_shards == 1 and gpu.n_segments == 70
    pairs = [(_pick(rng, vocab, int(rng.integers(1, 3)), 0.05), _pick(rng, vocab, int(rng.integers(0, 2)), 0.2)) for _ in range(60)]
    many, top = _both_modes(gpu, pairs, _top_queries(rng, pairs), "70 segments")
    assert sum(bool(r) for r in many) > 10
    # a term held by segments of both lookups keeps the snapshot's order: the union over all of them is complete
    t = max(vocab, key=lambda t: len(gpu.intersect([t])))
    gpu.set_resolve(1)
    one = gpu.intersect_batch([([t], [])])[0]
    gpu.set_resolve(0)
    assert one == gpu.intersect([t]) and len(one) > 3
    gpu.close()
