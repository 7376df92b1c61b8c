"""GPU: the host mirror's IntersectTopWeighted (host/host_index.cpp) - IntersectTop's groups, a weight per term, a term found in no
segment keeping its slot and its weight and matching nothing, ONE ii2_topk_weighted_ranges call and one download - over a small
unmerged index of a few Puts, against the numpy reference of tests/topkw_cases.py over Read's lists."""
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
    return list(zip(ids.tolist(), scores.tolist())), int(hist.sum())


def test_intersect_top_weighted_over_an_unmerged_index(ctx):
    from inverted_index_2_amd.host import InvertedIndex
    rng = np.random.default_rng(47)
    gpu = InvertedIndex(ctx)
    for _ in range(40):
        terms = [VOCAB[i] for i in rng.choice(len(VOCAB), int(rng.integers(2, 5)), replace=False)]
        gpu.put(terms, int(rng.integers(0, 120)))
    under = {t: vals for t, vals in gpu.read()}
    assert set(under) == set(VOCAB)
    queries = [(VOCAB[:4], [4, 1, 2, 1], [], [1, 3, 8]),
               ([VOCAB[0], ABSENT, VOCAB[3], VOCAB[5]], [3, 200, 5, 7], [], [1, 8, 15]),          # the absent term keeps its slot: 200 goes to nobody
               (VOCAB, [1, 2, 4, 8, 16, 32], [], [1, 33]),
               (VOCAB[1:5], [9, 6, 1, 1], [VOCAB[0], ABSENT], [1, 2, 7]),
               ([VOCAB[2], VOCAB[2], VOCAB[4]], [5, 5, 3], [], [1, 10])]                            # one term twice: two groups, both weights
    cuts = 0
    for terms, weights, exclude, min_scores in queries:
        for m in min_scores:
            _, eligible = _want(under, terms, weights, 0, m, exclude)
            for k in sorted({1, 3, max(eligible - 1, 1), max(eligible, 1), eligible + 1, eligible + 50}):
                want, _ = _want(under, terms, weights, k, m, exclude)
                got = gpu.intersect_top_weighted(terms, weights, k, m, exclude)
                assert got == want, (terms, weights, k, m, exclude)
                assert len(got) == min(k, eligible)
                cuts += 0 < k < eligible
    assert cuts >= 5
    # all-one weights are intersect_top
    for terms, _, exclude, _ in queries:
        assert gpu.intersect_top_weighted(terms, [1] * len(terms), 20, 2, exclude) == gpu.intersect_top(terms, 20, 2, exclude)
    assert gpu.intersect_top_weighted([], [], 5) == [] and gpu.intersect_top_weighted([ABSENT], [3], 5) == []
    assert gpu.intersect_top_weighted(VOCAB[:2], [1, 2], 0) == []
    assert gpu.intersect_top_weighted([VOCAB[1], ABSENT], [2, 200], 5, 3) == []                   # min_score above the weights that have postings
    for bad in (dict(terms=VOCAB[:2], weights=[1, 2], k=5, min_score=0), dict(terms=VOCAB[:2], weights=[1, 0], k=5),
                dict(terms=VOCAB[:2], weights=[1, 256], k=5), dict(terms=VOCAB[:2], weights=[128, 128], k=5),
                dict(terms=VOCAB[:2], weights=[1], k=5), dict(terms=VOCAB[:2], weights=[1, 2], k=(1 << 20) + 1)):
        with pytest.raises(Exception):
            gpu.intersect_top_weighted(**bad)
    gpu.close()
