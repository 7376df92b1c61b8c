"""GPU: the host mirror's PrefixSearch (host/host_index.cpp) makes ONE ii2_query_batch call for all its prefixes: an index of a
few thousand terms over several shards, unmerged and partly merged, a few hundred prefixes (nested ones, ones that match
nothing) in one call, against the reference model (oracle/ref_model.py)."""
import numpy as np
import pytest

from oracle import ref_model
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def _vocab(rng, n=3000):
    # second bytes from three shard ranges (shard key = first two bytes >> 6): digits, letters, bytes >= 0x80
    tail = list(b"0123abcd") + [0x41, 0x42, 0xC1, 0xC2]
    out = set()
    while len(out) < n:
        first = int(rng.choice(list(b"abmz")))
        out.add(bytes([first] + [int(rng.choice(tail)) for _ in range(int(rng.integers(2, 7)))]))
    return sorted(out)


def _prefixes(rng, vocab, n=300):
    out = [b"", b"a", b"ab", b"ab0", b"ab01", b"zzzz-none", b"\xff", b"q", b"a\xc1", b"mA"]      # nested ones, ones that match nothing
    while len(out) < n:
        t = vocab[int(rng.integers(0, len(vocab)))]
        cut = int(rng.integers(1, len(t) + 1))
        p = t[:cut]
        if rng.random() < 0.15:
            p = p + b"~none"                                                      # matches no term
        out.append(p)
    return out


def test_prefix_search_hundreds_of_prefixes_in_one_call(ctx):
    from inverted_index_2_amd.host import InvertedIndex
    rng = np.random.default_rng(77)
    vocab = _vocab(rng)
    gpu, ref = InvertedIndex(ctx), ref_model.InvertedIndex()
    for _ in range(500):
        terms = [vocab[i] for i in rng.choice(len(vocab), int(rng.integers(4, 16)), replace=False)]
        val = int(rng.integers(0, 100_000))
        gpu.put(list(terms), val)
        ref.put(list(terms), val)
    assert gpu.n_shards >= 6
    prefixes = _prefixes(rng, vocab)
    want = ref.prefix_search(prefixes)
    assert len(want) > 100 and b"zzzz-none" not in want and len(want[b"a"]) > len(want[b"ab"]) > 0
    assert gpu.prefix_search(prefixes) == want                                    # every segment unmerged
    assert gpu.merge(2, 8, 2) == ref.merge(2, 8, 2)                               # partly merged: merged and Put segments side by side
    want = ref.prefix_search(prefixes)
    assert gpu.prefix_search(prefixes) == want
    assert gpu.prefix_search(prefixes[:1]) == ref.prefix_search(prefixes[:1])
    assert gpu.prefix_search([b"zzzz-none", b"q"]) == {}
    gpu.close()
