"""GPU: the host mirror's MatchedTerms (host/host_index.cpp) - one group per term as IntersectTop builds them, one upload of the
ids, ONE ii2_explain_ranges call and one download - on an unmerged index: three Puts, so a term is a group of up to three lists.
The expectation comes from the Python lists that were Put."""
import numpy as np
import pytest

from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

# three shards (shard key = first two bytes >> 6): second bytes from three ranges
VOCAB = [b"a0x", b"a1y", b"a2", b"aAx", b"aBy", b"aB0", b"a\xc1x", b"a\xc2", b"a\xc1y", b"a3z"]
ABSENT = [b"a~none", b"aZnone"]


def _want(under, ids, terms):
    ids = [int(i) for i in ids]
    out = np.zeros((len(ids), (len(terms) + 63) // 64), np.uint64)
    first = {}
    for i, d in enumerate(ids):
        first.setdefault(d, i)
    for i, d in enumerate(ids):
        for j, t in enumerate(terms):
            if first[d] == i and d in under.get(t, ()):
                out[i, j >> 6] |= np.uint64(1 << (j & 63))
    return out


def test_matched_terms_on_an_unmerged_index(ctx):
    from inverted_index_2_amd.host import InvertedIndex
    rng = np.random.default_rng(61)
    gpu = InvertedIndex(ctx)
    under = {}
    puts = []
    for p in range(3):
        docs = []
        for _ in range(40):
            terms = [VOCAB[i] for i in rng.choice(len(VOCAB), int(rng.integers(1, 5)), replace=False)]
            docs.append((terms, int(rng.integers(0, 400))))
        if p == 2:
            docs += puts[0][:6]                                          # (term, doc) pairs Put twice
        puts.append(docs)
        gpu.put_batch(docs)
        for terms, d in docs:
            for t in terms:
                under.setdefault(t, set()).add(d)
    assert gpu.n_shards == 3 and set(under) == set(VOCAB)
    all_docs = sorted(set().union(*under.values()))
    page = [d for d, _ in gpu.intersect_top(VOCAB[:5], 30)]               # a ranked page: not ascending
    assert len(page) == 30 and page != sorted(page)
    id_sets = [page, all_docs, all_docs[::-1], [all_docs[3], 401, all_docs[3], 7, all_docs[0], all_docs[3]], [all_docs[5]], [100_000, 500_000]]
    term_sets = [VOCAB[:5], VOCAB, [VOCAB[1], ABSENT[0], VOCAB[5], ABSENT[1], VOCAB[8]], [VOCAB[4], VOCAB[4], VOCAB[6]],
                 [VOCAB[i % len(VOCAB)] for i in range(63)] + [ABSENT[0], VOCAB[2], VOCAB[9]]]      # 66 terms: two words per row
    some = False
    for ids in id_sets:
        for terms in term_sets:
            got = gpu.matched_terms(ids, terms)
            want = _want(under, ids, terms)
            assert got.dtype == np.uint64 and got.shape == want.shape and np.array_equal(got, want), (ids[:5], terms[:5])
            some = some or bool(want.any())
    assert some
    # the ranked page's scores are the popcounts of its rows
    top = gpu.intersect_top(VOCAB[:5], 30)
    rows = gpu.matched_terms([d for d, _ in top], VOCAB[:5])
    assert [bin(int(r[0])).count("1") for r in rows] == [s for _, s in top]
    # nothing to explain
    assert gpu.matched_terms([], VOCAB[:3]).shape == (0, 1)
    assert gpu.matched_terms(all_docs[:4], []).shape == (4, 0)
    assert not gpu.matched_terms(all_docs[:4], ABSENT).any() and gpu.matched_terms(all_docs[:4], ABSENT).shape == (4, 1)
    gpu.close()
