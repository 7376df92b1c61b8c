"""GPU: the host mirror's IntersectAtLeast (host/host_index.cpp) - one group per term, a term found in no segment an empty group,
ONE ii2_atleast_ranges call and one download - on an index of three shards whose terms lie unmerged over many Put segments, then
partly merged, for every threshold 1 .. n with and without excluded terms, against the numpy count over Read's lists."""
import numpy as np
import pytest

from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

# three shards (shard key = first two bytes >> 6): second bytes from three ranges
VOCAB = [b"a0x", b"a1y", b"a2", b"aAx", b"aBy", b"aB0", b"a\xc1x", b"a\xc2", b"a\xc1y", b"a3z"]
ABSENT = [b"a~none", b"aZnone"]


def _want(under, terms, m, exclude):
    groups = [np.unique(np.asarray(under.get(t, []), np.uint32)) for t in terms]
    ids, cnt = np.unique(np.concatenate(groups + [np.empty(0, np.uint32)]), return_counts=True)
    drop = np.concatenate([np.asarray(under.get(t, []), np.uint32) for t in exclude] + [np.empty(0, np.uint32)])
    return np.setdiff1d(ids[cnt >= m], drop).astype(np.uint32).tolist()


def test_intersect_at_least_before_and_after_a_merge(ctx):
    from inverted_index_2_amd.host import InvertedIndex
    rng = np.random.default_rng(41)
    gpu = InvertedIndex(ctx)
    for _ in range(120):
        terms = [VOCAB[i] for i in rng.choice(len(VOCAB), int(rng.integers(2, 6)), replace=False)]
        gpu.put(terms, int(rng.integers(0, 300)))
    assert gpu.n_shards == 3
    queries = [(VOCAB[:4], []), (VOCAB[2:9], [VOCAB[0]]), (VOCAB, []), (VOCAB, [VOCAB[9], ABSENT[1]]),
               ([VOCAB[1], ABSENT[0], VOCAB[5], VOCAB[7]], []), ([VOCAB[1], ABSENT[0], VOCAB[5], ABSENT[1], VOCAB[8]], [VOCAB[3]]),
               ([VOCAB[4], VOCAB[4], VOCAB[6]], [])]
    for stage in ("unmerged", "merged"):
        under = {t: vals for t, vals in gpu.read()}
        assert set(under) == set(VOCAB)
        shrank = absent_kept = 0
        for terms, exclude in queries:
            results = []
            for m in range(1, len(terms) + 1):
                want = _want(under, terms, m, exclude)
                assert gpu.intersect_at_least(terms, m, exclude) == want, (stage, terms, m, exclude)
                results.append(want)
            assert results[0] and all(set(b) <= set(a) for a, b in zip(results, results[1:]))
            shrank += len(results[1]) < len(results[0])
            # a required term found in no segment does not empty the result: it only cannot be matched
            if any(t in ABSENT for t in terms):
                present = sum(t not in ABSENT for t in terms)
                assert results[present - 1] and not results[present]
                absent_kept += 1
            if exclude:
                assert results[0] != _want(under, terms, 1, [])
            # m = n is IntersectExcept, m = 1 without exclusion the union of the terms' lists
            if not any(t in ABSENT for t in terms):
                assert results[-1] == gpu.intersect_except(terms, exclude)
        assert shrank >= 5 and absent_kept == 2
        assert gpu.intersect_at_least([], 1) == [] and gpu.intersect_at_least(ABSENT, 1) == []
        with pytest.raises(Exception):
            gpu.intersect_at_least(VOCAB[:2], 0)
        if stage == "unmerged":
            assert gpu.merge(2, 8, 2) > 0                               # partly merged: merged and Put segments side by side
    gpu.close()
