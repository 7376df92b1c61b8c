"""GPU: the host mirror's MatchedTermsBatch (host/host_index.cpp) - per page the groups MatchedTerms builds, one upload of all ids,
ONE ii2_explain_batch call and one download - equals MatchedTerms page by page, on an unmerged index of three Puts (a term is a
group of up to three lists), under both ways of resolving the terms.  One term is absent from every segment, one page is empty, one
page has only absent terms."""
import numpy as np
import pytest

from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

# three shards (shard key = first two bytes >> 6): second bytes from three ranges
VOCAB = [b"a0x", b"a1y", b"a2", b"aAx", b"aBy", b"aB0", b"a\xc1x", b"a\xc2", b"a\xc1y", b"a3z"]
ABSENT = [b"a~none", b"aZnone"]


def test_matched_terms_batch_equals_matched_terms_page_by_page(ctx):
    from inverted_index_2_amd.host import InvertedIndex
    rng = np.random.default_rng(62)
    gpu = InvertedIndex(ctx)
    under = {}
    for p in range(3):
        docs = []
        for _ in range(40):
            terms = [VOCAB[i] for i in rng.choice(len(VOCAB), int(rng.integers(1, 5)), replace=False)]
            docs.append((terms, int(rng.integers(0, 400))))
        gpu.put_batch(docs)
        for terms, d in docs:
            for t in terms:
                under.setdefault(t, set()).add(d)
    assert gpu.n_shards == 3 and set(under) == set(VOCAB)
    all_docs = sorted(set().union(*under.values()))
    ranked = [d for d, _ in gpu.intersect_top(VOCAB[:5], 30)]               # a ranked page: not ascending
    assert len(ranked) == 30 and ranked != sorted(ranked)
    pages = [(ranked, VOCAB[:5]),
             (all_docs, [VOCAB[1], ABSENT[0], VOCAB[5], VOCAB[8]]),       # a term absent from every segment keeps its bit, never set
             ([], VOCAB[:3]),                                             # an empty page
             ([all_docs[3], 401, all_docs[3], 7, all_docs[0], all_docs[3]], VOCAB),
             (all_docs[:6], ABSENT),                                      # no term in any segment: no group, zero rows of one word
             (all_docs[::-1], [VOCAB[i % len(VOCAB)] for i in range(63)] + [ABSENT[1], VOCAB[2], VOCAB[9]]),      # 66 terms: two words a row
             (all_docs[:4], []),                                          # no term: rows without a word
             (ranked[::-1], VOCAB[5:])]
    want = [gpu.matched_terms(ids, terms) for ids, terms in pages]
    assert any(w.any() for w in want) and not want[4].any() and want[4].shape == (6, 1) and want[5].shape == (len(all_docs), 2)
    assert not (want[1][:, 0] & np.uint64(2)).any() and (want[1][:, 0] & np.uint64(1)).any()
    for mode in (0, 1):                                                   # host bisection, device lookup
        gpu.set_resolve(mode)
        got = gpu.matched_terms_batch(pages)
        assert len(got) == len(pages)
        for p, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == np.uint64 and g.shape == w.shape and np.array_equal(g, w), (mode, p)
    gpu.set_resolve(0)
    # the same against the lists that were Put, for one page
    ids, terms = pages[3]
    first = {}
    for i, d in enumerate(ids):
        first.setdefault(d, i)
    for i, d in enumerate(ids):
        bits = sum(1 << j for j, t in enumerate(terms) if first[d] == i and d in under[t])
        assert int(got[3][i, 0]) == bits
    assert gpu.matched_terms_batch([]) == []
    assert [g.shape for g in gpu.matched_terms_batch([([], VOCAB[:2]), (all_docs[:2], ABSENT)])] == [(0, 1), (2, 1)]
    gpu.close()
