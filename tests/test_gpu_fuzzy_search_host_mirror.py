"""GPU: the host mirror's FuzzySearch and FuzzyTerms (host/host_index.cpp) - typo-tolerant search over every segment of every
shard through ii2_dict_fuzzy and one ii2_query_batch call - against plain Python over the same documents: an index of a few
hundred Puts over several shards, partly merged; both distances, a prefix, case folding; a query term that matches nothing; more
than 16 query terms in one call; the order and the limit of FuzzyTerms; and the same two methods of a single Shard of more than
64 segments."""
import numpy as np
import pytest

from tests.fuzzy_cases import NOCASE, TRANSPOSE, distance, matches
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

SERVICES = (b"conn", b"db", b"http", b"Auth", b"queue")
EVENTS = (b"timeout", b"timeuot", b"tmeout", b"timeouts", b"error", b"ERROR", b"eror", b"retry", b"retyr", b"ok")


def _vocab():
    # first bytes c / d / h / A / q: several shards (the shard key is the first two bytes >> 6)
    return sorted({a + b"_" + b + (b"%d" % i if i else b"") for a in SERVICES for b in EVENTS for i in range(3)} | {b"timeout", b"error", b"retry"})


def _docs(rng, vocab, n):
    return [(sorted({vocab[int(i)] for i in rng.integers(0, len(vocab), int(rng.integers(1, 7)))}), doc) for doc in range(1, n + 1)]


def _want(docs, term, d, prefix, flags):
    pre = min(prefix, len(term))                             # a query term shorter than the prefix is compared as a whole
    hit = sorted({t for terms, _ in docs for t in terms if matches(term, t, d, pre, flags)})
    ids = sorted({doc for terms, doc in docs for t in terms if matches(term, t, d, pre, flags)})
    ranked = sorted(((t, distance(term, t, flags)) for t in hit), key=lambda td: (td[1], td[0]))
    return ids, ranked


QUERIES = [b"conn_timeout", b"db_error", b"http_retry1", b"AUTH_OK", b"queue_timeout2", b"timeout", b"eror", b"no-such-thing-at-all", b"", b"db", b"retry"]
SETTINGS = [(1, 0, 0), (2, 0, 0), (2, 3, TRANSPOSE), (2, 0, NOCASE), (1, 5, NOCASE | TRANSPOSE), (0, 0, 0)]


def _check_all(target, docs, stage):
    for d, prefix, flags in SETTINGS:
        got = target.fuzzy_search(QUERIES, d, prefix, flags)
        for q in QUERIES:
            ids, ranked = _want(docs, q, d, prefix, flags)
            assert got.get(q, []) == ids, (stage, q, d, prefix, flags)
            assert (q in got) == bool(ids), (stage, q, d, prefix, flags)      # a query term without a match has no entry
            assert target.fuzzy_terms(q, d, prefix, flags) == ranked, (stage, q, d, prefix, flags)
            assert target.fuzzy_terms(q, d, prefix, flags, 3) == ranked[:3], (stage, q, d, prefix, flags)
    assert target.fuzzy_search([], 2) == {} and target.fuzzy_terms(b"timeout", 2, limit=0) == []


def test_fuzzy_search_and_fuzzy_terms(ctx):
    from inverted_index_2_amd.host import HostError, InvertedIndex
    rng = np.random.default_rng(79)
    vocab = _vocab()
    docs = _docs(rng, vocab, 300)
    gpu = InvertedIndex(ctx)
    for terms, doc in docs[:200]:
        gpu.put(terms, doc)
    assert gpu.lib.ii2h_shard_count(gpu.h) >= 3
    _check_all(gpu, docs[:200], "unmerged")
    gpu.merge(2, 40)                                        # partly merged: some big segments, many direct ones left
    for terms, doc in docs[200:]:
        gpu.put(terms, doc)
    _check_all(gpu, docs, "partly merged")
    # the closer terms come first, ties in byte order
    ids, ranked = _want(docs, b"conn_timeout", 2, 0, 0)
    assert ranked[0] == (b"conn_timeout", 0) and [d for _, d in ranked] == sorted(d for _, d in ranked) and len({d for _, d in ranked}) == 3
    assert any(a[1] == b[1] and a[0] < b[0] for a, b in zip(ranked, ranked[1:]))
    # more than 16 query terms in one call: every term of the vocabulary, and a typo of each
    many = sorted(set(vocab))
    assert len(many) > 64
    got = gpu.fuzzy_search(many, 1)
    for t in many:
        assert got.get(t, []) == _want(docs, t, 1, 0, 0)[0], t
    typos = sorted({t[:3] + t[4:] for t in many} | {t[:-2] + t[-1:] + t[-2:-1] for t in many})
    assert len(typos) > 16
    got = gpu.fuzzy_search(typos, 1, 2, TRANSPOSE)
    for t in typos:
        assert got.get(t, []) == _want(docs, t, 1, 2, TRANSPOSE)[0], t
    # a first buffer of four ids: the union goes through two_call's second call and gives the same
    every = sorted({doc for terms, doc in docs for t in terms if len(t) <= 40})
    before = gpu.second_calls
    gpu.set_first_cap(4)
    assert gpu.fuzzy_search([b""], 40) == {b"": every} and gpu.second_calls == before + 1
    gpu.set_first_cap(1 << 22)
    # removed docs are not filtered, as in read
    gpu.put_removed([1, 2, 3])
    assert gpu.fuzzy_search([b""], 40)[b""] == every
    # errors come back as errors
    with pytest.raises(HostError):
        gpu.fuzzy_search([b"x" * 65], 1)
    with pytest.raises(HostError):
        gpu.fuzzy_search([b"abc"], 1, 0, 0x02)
    with pytest.raises(HostError):
        gpu.fuzzy_search([b"abc"], 256)
    with pytest.raises(HostError):
        gpu.fuzzy_terms(b"a", 1, 0, 0x40)
    gpu.close()


def test_a_single_shard(ctx):
    from inverted_index_2_amd.host import Shard
    rng = np.random.default_rng(80)
    docs = _docs(rng, _vocab(), 70)                        # more than 64 segments: two chunks of dictionaries
    sh = Shard(ctx)
    for terms, doc in docs:
        sh.put(terms, doc)
    assert sh.n_segments == 70
    _check_all(sh, docs, "shard, unmerged")
    sh.merge(2, 30)
    assert sh.n_segments < 70
    _check_all(sh, docs, "shard, partly merged")
    sh.close()
