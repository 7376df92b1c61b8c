"""GPU: the host mirror's IntersectTopBatch (host/host_index.cpp) - many IntersectTopWeighted queries, the groups built as that call
builds them, ONE ii2_topk_batch call and one download - over a small unmerged index of 40 Puts: equal to a loop of
intersect_top_weighted and to the numpy reference of tests/topkw_cases.py over Read's lists; an absent term, an excluded term,
removed ids (like IntersectTopWeighted, the mirror applies no tombstone filter: the removed ids stay until a merge)."""
import numpy as np
import pytest

from tests import topkw_cases as wc
from tests.atleast_cases import Case
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

VOCAB = [b"a0x", b"a1y", b"aAx", b"aBy", b"a\xc1x", b"a\xc2"]
ABSENT = b"a~none"


def _want(under, terms, weights, k, min_score, exclude):
    lists = [np.unique(np.asarray(under.get(t, []), np.uint32)) for t in list(terms) + list(exclude)]
    case = Case("mirror", lists, [[i] for i in range(len(terms))], 1, exclude=[[len(terms) + i] for i in range(len(exclude))])
    ids, scores, hist = wc.reference(case, weights, k, min_score)
    return list(zip(ids.tolist(), scores.tolist()))


def test_intersect_top_batch_over_an_unmerged_index(ctx):
    from inverted_index_2_amd.host import InvertedIndex
    rng = np.random.default_rng(53)
    gpu = InvertedIndex(ctx)
    for _ in range(40):
        terms = [VOCAB[i] for i in rng.choice(len(VOCAB), int(rng.integers(2, 5)), replace=False)]
        gpu.put(terms, int(rng.integers(0, 120)))
    assert gpu.n_segments >= 40                                      # left unmerged: every term is a group of one-posting lists
    under = {t: vals for t, vals in gpu.read()}
    assert set(under) == set(VOCAB)
    shapes = [(VOCAB[:4], [4, 1, 2, 1], []),
              ([VOCAB[0], ABSENT, VOCAB[3], VOCAB[5]], [3, 200, 5, 7], []),          # the absent term keeps its slot: 200 goes to nobody
              (VOCAB, [1, 2, 4, 8, 16, 32], []),
              (VOCAB[1:5], [9, 6, 1, 1], [VOCAB[0], ABSENT]),                        # an excluded term, and an absent one that removes nothing
              ([VOCAB[2], VOCAB[2], VOCAB[4]], [5, 5, 3], []),                       # one term twice: two groups, both weights
              ([ABSENT], [3], []), ([], [], []),                                     # nothing to run: the queries keep their places
              ([VOCAB[1], ABSENT], [2, 200], [])]
    queries = [(t, w, k, m, x) for t, w, x in shapes for m in (1, 3, 8) for k in (0, 1, 3, 50)]
    want = [_want(under, t, w, k, m, x) for t, w, k, m, x in queries]
    assert sum(1 for w in want if w) > 30 and sum(1 for (t, w, k, m, x), r in zip(queries, want) if 0 < k == len(r)) > 10
    got = gpu.intersect_top_batch(queries)
    assert got == want
    assert got == [gpu.intersect_top_weighted(t, w, k, m, x) for t, w, k, m, x in queries]
    assert gpu.intersect_top_batch([]) == []
    # removed ids: neither call filters them, so the two still agree
    gpu.put_removed(sorted({int(v) for v in under[VOCAB[0]][:5]}))
    assert gpu.intersect_top_batch(queries) == [gpu.intersect_top_weighted(t, w, k, m, x) for t, w, k, m, x in queries] == want
    for bad in ((VOCAB[:2], [1, 2], 5, 0, []), (VOCAB[:2], [1, 0], 5, 1, []), (VOCAB[:2], [1, 256], 5, 1, []), (VOCAB[:2], [128, 128], 5, 1, []),
                (VOCAB[:2], [1, 2], (1 << 20) + 1, 1, [])):
        with pytest.raises(Exception, match="query 1"):
            gpu.intersect_top_batch([queries[0], bad, queries[1]])
    with pytest.raises(ValueError, match="query 1: one weight per term"):
        gpu.intersect_top_batch([queries[0], (VOCAB[:2], [1], 5, 1, [])])
    gpu.close()
