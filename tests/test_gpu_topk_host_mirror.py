"""GPU: the host mirror's IntersectTop (host/host_index.cpp) - one group per term, a term found in no segment an empty group, ONE
ii2_topk_ranges call and one download of the k (id, score) pairs - on an index of three shards whose terms lie unmerged over many
Put segments, then partly merged, with absent and excluded terms, for k below, at and above the eligible docs, against a Python count
over Read's lists."""
import numpy as np
import pytest

from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

# three shards (shard key = first two bytes >> 6): second bytes from three ranges
VOCAB = [b"a0x", b"a1y", b"a2", b"aAx", b"aBy", b"aB0", b"a\xc1x", b"a\xc2", b"a\xc1y", b"a3z"]
ABSENT = [b"a~none", b"aZnone"]


def _want(under, terms, k, m, exclude):
    score = {}
    for t in terms:
        for d in set(under.get(t, [])):
            score[d] = score.get(d, 0) + 1
    drop = {d for t in exclude for d in under.get(t, [])}
    ranked = sorted(((d, s) for d, s in score.items() if s >= m and d not in drop), key=lambda p: (-p[1], p[0]))
    return ranked[:k], len(ranked)


def test_intersect_top_before_and_after_a_merge(ctx):
    from inverted_index_2_amd.host import InvertedIndex
    rng = np.random.default_rng(43)
    gpu = InvertedIndex(ctx)
    for _ in range(120):
        terms = [VOCAB[i] for i in rng.choice(len(VOCAB), int(rng.integers(2, 6)), replace=False)]
        gpu.put(terms, int(rng.integers(0, 300)))
    assert gpu.n_shards == 3
    queries = [(VOCAB[:4], [], 1), (VOCAB[2:9], [VOCAB[0]], 2), (VOCAB, [], 1), (VOCAB, [VOCAB[9], ABSENT[1]], 3),
               ([VOCAB[1], ABSENT[0], VOCAB[5], VOCAB[7]], [], 1), ([VOCAB[1], ABSENT[0], VOCAB[5], ABSENT[1], VOCAB[8]], [VOCAB[3]], 2),
               ([VOCAB[4], VOCAB[4], VOCAB[6]], [], 1)]
    for stage in ("unmerged", "merged"):
        under = {t: vals for t, vals in gpu.read()}
        assert set(under) == set(VOCAB)
        ties = 0
        for terms, exclude, m in queries:
            _, eligible = _want(under, terms, 1, m, exclude)
            assert eligible > 3
            for k in (1, 3, eligible - 1, eligible, eligible + 1, eligible + 100):
                want, _ = _want(under, terms, k, m, exclude)
                got = gpu.intersect_top(terms, k, m, exclude)
                assert got == want, (stage, terms, k, m, exclude)
                assert len(got) == min(k, eligible)
                ties += k < eligible and sum(1 for _, s in _want(under, terms, eligible, m, exclude)[0] if s == want[-1][1]) > sum(1 for _, s in want if s == want[-1][1])
            if exclude:
                assert _want(under, terms, eligible, m, exclude)[0] != _want(under, terms, eligible, m, [])[0][:eligible]
            # the ids under every present term come first: score n' is IntersectExcept
            present = [t for t in terms if t not in ABSENT]
            full = sorted(d for d, s in gpu.intersect_top(terms, eligible, m, exclude) if s == len(present))
            assert full == gpu.intersect_except(present, exclude)
        assert ties >= 5                                                # some cuts fell inside a score class
        assert gpu.intersect_top([], 5) == [] and gpu.intersect_top(ABSENT, 5) == [] and gpu.intersect_top(VOCAB[:2], 0) == []
        assert gpu.intersect_top([VOCAB[1], ABSENT[0]], 5, 2) == []   # min_match above the terms that have postings
        with pytest.raises(Exception):
            gpu.intersect_top(VOCAB[:2], 5, 0)
        with pytest.raises(Exception):
            gpu.intersect_top(VOCAB[:2], (1 << 20) + 1)
        if stage == "unmerged":
            assert gpu.merge(2, 8, 2) > 0                               # partly merged: merged and Put segments side by side
    gpu.close()
