"""GPU: the host mirror's Histogram and TermHistogram (host/host_index.cpp) - a query's docs per value bucket (the result stays on
the device, ONE ii2_histogram_ids call) and TermCounts per value bucket (ONE ii2_histogram_ranges call over the prefix's run of
every segment, terms hit in several segments counted again exactly) - on the index of tests/test_gpu_term_counts_host_mirror.py:
some 300 docs over 42 terms under four prefixes, built by put_batch, put and a partial merge, with a few (term, doc) pairs Put
twice into different segments.  Expected values from the reference model's read() (oracle/ref_model.py) and Python sets."""
import numpy as np
import pytest

from oracle import ref_model
from tests import hist_cases as hc
from tests.gpu_util import ctx  # noqa: F401
from tests.test_gpu_term_counts_host_mirror import QUERIES, _docs

pytestmark = pytest.mark.gpu

VALUES = 100_000          # the docs' values lie in [0, VALUES)


def _keep(under, terms, exclude):
    keep = set.intersection(*[under.get(t, set()) for t in terms])
    for t in exclude:
        keep -= under.get(t, set())
    return keep


def _row(ids, edges):
    b = hc.buckets(edges, sorted(ids))
    return np.bincount(b[b >= 0], minlength=len(edges) - 1).astype(np.uint64)


def _want_terms(under, prefix, edges, terms=(), exclude=()):
    keep = _keep(under, terms, exclude) if terms else None
    out = {}
    for t, s in under.items():
        if t.startswith(prefix):
            row = _row(s if keep is None else s & keep, edges)
            if row.any():
                out[t] = row
    return out


def _same(got, want):
    return sorted(got) == sorted(want) and all(got[t].dtype == np.uint64 and np.array_equal(got[t], want[t]) for t in want)


def test_histograms_before_and_after_a_merge(ctx):
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
    axes = [hc.uniform(0, VALUES, n) for n in (1, 7, 100)] + [hc.uniform(VALUES // 4, 3 * VALUES // 4, 9)]
    for stage in ("unmerged", "merged"):
        under = {t: set(int(v) for v in vals) for t, vals in ref.read()}
        assert len(under) == 42
        for edges in axes:
            full = edges[0] == 0
            nonzero = 0
            for prefix, terms, exclude in QUERIES:
                keep = _keep(under, terms, exclude)
                got = gpu.histogram(terms, edges, exclude)
                assert got.dtype == np.uint64 and np.array_equal(got, _row(keep, edges)), (stage, len(edges), terms, exclude)
                want = _want_terms(under, prefix, edges, terms, exclude)
                got = gpu.term_histogram(prefix, edges, terms, exclude)
                assert _same(got, want), (stage, len(edges), prefix, terms, exclude)
                nonzero += len(want)
                if full:                                                # row sums over a full axis are the facet counts
                    assert {t: int(r.sum()) for t, r in got.items()} == gpu.term_counts(prefix, terms, exclude)
                    assert int(gpu.histogram(terms, edges, exclude).sum()) == len(keep)
            assert nonzero > 10                                         # not everything empty
            # a term's frequency over time: the pairs Put twice count once (their plain per-segment sum would not)
            for prefix in (b"level=", b"host=", b"svc=", b"tag=", b""):
                got = gpu.term_histogram(prefix, edges)
                assert _same(got, _want_terms(under, prefix, edges)), (stage, len(edges), prefix)
                if full:
                    assert {t: int(r.sum()) for t, r in got.items()} == gpu.term_counts(prefix)
        # the exact re-count is taken: a doubled pair's term lies in two segments with the same doc, and still counts it once
        for terms, val in again[:3]:
            t = terms[1]
            row = gpu.term_histogram(t, [0, val, val + 1, VALUES])[t]
            assert row.tolist() == [len([v for v in under[t] if v < val]), 1, len([v for v in under[t] if v > val])]
            assert int(gpu.histogram([t], [val, val + 1])[0]) == 1
        assert gpu.term_histogram(b"zone=", axes[1]) == {} and gpu.term_histogram(b"host=h99", axes[1], [b"level=error"]) == {}
        assert gpu.term_histogram(b"host=", axes[1], [b"level=error", b"level=none"]) == {}                   # a required term in no segment
        assert gpu.term_histogram(b"host=", axes[1], [b"level=error"], [b"level=error"]) == {}               # an empty filter result
        assert gpu.histogram([b"level=error", b"level=none"], axes[1]).tolist() == [0] * 7
        assert gpu.histogram([], axes[1]).tolist() == [0] * 7                                                  # no term: nothing under every term
        with pytest.raises(Exception):
            gpu.histogram([b"level=error"], [5, 5])
        with pytest.raises(Exception):
            gpu.term_histogram(b"host=", [10, 5, 20])
        if stage == "unmerged":
            before = gpu.n_segments
            assert before > 200 and gpu.merge(2, 8, 2) > 0             # partly merged: merged and Put segments side by side
            assert 4 < gpu.n_segments < before
            put_all(docs[260:] + docs[20:24])                           # ... fresh Put segments and more pairs for the second time
    gpu.close()
