"""GPU: the host mirror's TermCounts (host/host_index.cpp) - facet counts: the filter result stays on the device, ONE
ii2_count_ranges call over the prefix's run of every segment, terms hit in several segments counted again exactly - on an index of
some 300 docs over 42 terms under four prefixes, built by put_batch, put and a partial merge, with a few (term, doc) pairs Put
twice into different segments.  Expected values from the reference model's read() (oracle/ref_model.py) and Python sets."""
import numpy as np
import pytest

from oracle import ref_model
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

LEVELS = [b"level=debug", b"level=error", b"level=info", b"level=warn"]
HOSTS = [b"host=h%02d" % i for i in range(20)]
SVCS = [b"svc=" + s for s in (b"api", b"auth", b"cache", b"cron", b"db", b"dns", b"mail", b"mq", b"proxy", b"search", b"store", b"web")]
TAGS = [b"tag=" + s for s in (b"batch", b"canary", b"healthcheck", b"retry", b"slow", b"tls")]


def _docs(rng, n):
    vals = rng.choice(100_000, n, replace=False)
    docs = []
    for v in vals:
        terms = [LEVELS[int(rng.integers(0, 4))], HOSTS[int(rng.integers(0, 20))], SVCS[int(rng.integers(0, 12))]]
        terms += [TAGS[i] for i in rng.choice(6, int(rng.integers(0, 3)), replace=False)]
        docs.append((terms, int(v)))
    return docs


def _want(under, prefix, terms=(), exclude=()):
    if terms:
        keep = set.intersection(*[under.get(t, set()) for t in terms])
        for t in exclude:
            keep -= under.get(t, set())
        out = {t: len(s & keep) for t, s in under.items() if t.startswith(prefix)}
    else:
        out = {t: len(s) for t, s in under.items() if t.startswith(prefix)}
    return {t: c for t, c in out.items() if c}


QUERIES = [(b"host=", [b"level=error"], []), (b"host=", [b"level=error"], [b"tag=healthcheck"]),
           (b"svc=", [b"level=info", b"tag=retry"], [b"tag=slow", b"svc=none"]), (b"level=", [b"svc=db"], [b"host=h03", b"host=h04"]),
           (b"tag=", [b"level=warn"], []), (b"", [b"level=error"], [b"svc=db"]), (b"host=h1", [b"level=debug"], [])]


def test_term_counts_before_and_after_a_merge(ctx):
    from inverted_index_2_amd.host import InvertedIndex
    rng = np.random.default_rng(91)
    docs = _docs(rng, 300)
    gpu, ref = InvertedIndex(ctx), ref_model.InvertedIndex()

    def put_all(batch):
        for terms, val in batch:
            gpu.put(list(terms), val)
            ref.put(list(terms), val)

    gpu.put_batch(docs[:150])                                           # one merged-quality segment per shard
    for terms, val in docs[:150]:
        ref.put(list(terms), val)
    put_all(docs[150:260])                                              # one segment per put and shard on top
    again = docs[5:12] + docs[155:160]
    put_all(again)                                                      # (term, doc) pairs a second time, in segments of their own
    for stage in ("unmerged", "merged"):
        under = {t: set(int(v) for v in vals) for t, vals in ref.read()}
        assert len(under) == 42
        nonzero = narrowed = 0
        for prefix, terms, exclude in QUERIES:
            want = _want(under, prefix, terms, exclude)
            assert gpu.term_counts(prefix, terms, exclude) == want, (stage, prefix, terms, exclude)
            nonzero += len(want)
            narrowed += want != _want(under, prefix)
        assert nonzero > 40 and narrowed == len(QUERIES)                 # neither everything empty nor filters that never bite
        # document frequencies: the pairs Put twice count once (their plain per-segment sum would not)
        for prefix in (b"level=", b"host=", b"svc=", b"tag=", b""):
            assert gpu.term_counts(prefix) == _want(under, prefix), (stage, prefix)
        twice = again[0][0][1]
        assert gpu.term_counts(twice)[twice] == len(under[twice])
        assert gpu.term_counts(b"zone=") == {} and gpu.term_counts(b"host=h99", [b"level=error"]) == {}      # a prefix that matches nothing
        assert gpu.term_counts(b"host=", [b"level=error", b"level=none"]) == {}                               # a required term in no segment
        assert gpu.term_counts(b"host=", [b"level=error"], [b"level=error"]) == {}                           # an empty filter result
        if stage == "unmerged":
            before = gpu.n_segments
            assert before > 200 and gpu.merge(2, 8, 2) > 0             # partly merged: merged and Put segments side by side
            assert 4 < gpu.n_segments < before
            put_all(docs[260:] + docs[20:24])                           # ... fresh Put segments and more pairs for the second time
    gpu.close()
