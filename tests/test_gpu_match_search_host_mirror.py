"""GPU: the host mirror's MatchSearch and MatchTerms (host/host_index.cpp) - substring, suffix and wildcard search over every
segment of every shard through ii2_dict_match and one ii2_query_batch call - against plain Python over the same documents: an
index of a few hundred Puts over several shards, partly merged; every kind, with and without case folding; a pattern that
matches nothing, one that matches every term, more than 64 patterns in one call, a result that needs two_call's second call;
and the same two methods of a single Shard."""
import numpy as np
import pytest

from tests import match_cases
from tests.gpu_util import ctx  # noqa: F401
from tests.match_cases import CONTAINS, GLOB, NOCASE, SUFFIX

pytestmark = pytest.mark.gpu

SERVICES, EVENTS = (b"conn", b"db", b"http", b"Auth", b"queue"), (b"timeout", b"error", b"ERROR", b"retry", b"ok", b"Timeout_ms")


def _vocab():
    # first bytes c / d / h / A / q: several shards (the shard key is the first two bytes >> 6)
    return sorted({a + b"_" + b + (b"%d" % i if i else b"") for a in SERVICES for b in EVENTS for i in range(4)} | {b"x.example.com", b"y.example.org", b"example.com"})


def _docs(rng, vocab, n):
    return [(sorted({vocab[int(i)] for i in rng.integers(0, len(vocab), int(rng.integers(1, 7)))}), doc) for doc in range(1, n + 1)]


def _want(docs, kind, pattern):
    m = match_cases.matcher(kind, pattern)
    ids = sorted({doc for terms, doc in docs for t in terms if m(t)})
    terms = sorted({t for terms, _ in docs for t in terms if m(t)})
    return ids, terms


PATTERNS = {
    CONTAINS: [b"timeout", b"_e", b"example", b"no-such-thing", b"", b"1"],
    CONTAINS | NOCASE: [b"TIMEOUT", b"error", b"auth_"],
    SUFFIX: [b"timeout", b"1", b".com", b"", b"zz"],
    SUFFIX | NOCASE: [b"ERROR", b"OK3"],
    GLOB: [b"*", b"*.example.com", b"db_*", b"?b_*", b"*_retry?", b"*timeout*", b"conn_ok", b"nothing*", b"*\\_ok", b""],
    GLOB | NOCASE: [b"auth_*", b"*TIMEOUT*", b"*_error?"],
}


def _check_all(target, docs, stage):
    for kind, patterns in PATTERNS.items():
        got = target.match_search(patterns, kind)
        for p in patterns:
            ids, terms = _want(docs, kind, p)
            assert got.get(p, []) == ids, (stage, kind, p)
            assert (p in got) == bool(ids), (stage, kind, p)              # a pattern without a match has no entry
            assert target.match_terms(p, kind) == terms, (stage, kind, p)
            assert target.match_terms(p, kind, 3) == terms[:3], (stage, kind, p)
    assert target.match_search([], GLOB) == {} and target.match_terms(b"*", GLOB, 0) == []


def test_match_search_and_match_terms(ctx):
    from inverted_index_2_amd.host import HostError, InvertedIndex
    rng = np.random.default_rng(77)
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
    # every term: as many ids as there are docs, every term of the index
    every, all_terms = _want(docs, GLOB, b"*")
    assert every == list(range(1, 301)) and gpu.match_search([b""], CONTAINS)[b""] == every and gpu.match_terms(b"", SUFFIX) == all_terms
    # more than 64 patterns in one call: every term as a literal glob, and its first five bytes as a substring
    many = sorted(set(vocab))
    assert len(many) > 64
    got = gpu.match_search([t.replace(b"_", b"\\_") for t in many], GLOB)
    for t in many:
        assert got.get(t.replace(b"_", b"\\_"), []) == _want(docs, GLOB, t.replace(b"_", b"\\_"))[0], t
    heads = sorted({t[:5] for t in many} | {t[-4:] for t in many} | {b"%c" % c for c in b"abcdefghijklmnopqrstuvwxyz_.0123"})
    assert len(heads) > 64
    got = gpu.match_search(heads, CONTAINS | NOCASE)
    for h in heads:
        assert got.get(h, []) == _want(docs, CONTAINS | NOCASE, h)[0], h
    # a first buffer of four ids: the union goes through two_call's second call and gives the same
    before = gpu.second_calls
    gpu.set_first_cap(4)
    assert gpu.match_search([b"timeout", b"*"], GLOB) == {b"*": every} and gpu.second_calls == before + 1
    gpu.set_first_cap(1 << 22)
    # removed docs are not filtered, as in read
    gpu.put_removed([1, 2, 3])
    assert gpu.match_search([b"*"], GLOB)[b"*"] == every
    # errors come back as errors
    with pytest.raises(HostError):
        gpu.match_search([b"oops\\"], GLOB)
    with pytest.raises(HostError):
        gpu.match_search([b"x" * 65], CONTAINS)
    with pytest.raises(HostError):
        gpu.match_terms(b"a", 7)
    gpu.close()


def test_many_runs_in_one_segment(ctx):
    """Alternate terms of ONE segment match: 300 runs of one term each, all in the same segment.  The union's bound counts that
    segment once (tests/test_match_search_bound_cpu.py pins the arithmetic), and the result is the same through a first buffer
    that holds it and through one that does not."""
    from inverted_index_2_amd.host import InvertedIndex
    terms = [b"k%04d%s" % (i, b"a" if i % 2 == 0 else b"b") for i in range(600)]
    docs = [([t, b"k9all"], i + 1) for i, t in enumerate(terms)]
    gpu = InvertedIndex(ctx)
    gpu.put_batch(docs)
    assert gpu.n_segments == 1
    want = {b"a": list(range(1, 601, 2)), b"b": list(range(2, 601, 2)), b"l": list(range(1, 601))}
    assert gpu.match_terms(b"a", SUFFIX) == terms[0::2]
    assert gpu.match_search([b"a", b"b", b"l", b"zz"], SUFFIX) == want and gpu.second_calls == 0
    gpu.set_first_cap(1000)                                # 1200 ids in all: the batch's second call, once
    assert gpu.match_search([b"a", b"b", b"l"], SUFFIX) == want and gpu.second_calls == 1
    gpu.set_first_cap(100)
    assert gpu.match_search([b"a"], SUFFIX) == {b"a": want[b"a"]} and gpu.second_calls == 2
    assert gpu.prefix_search([b"k0", b"k9", b"q"]) == {b"k0": want[b"l"], b"k9": want[b"l"]} and gpu.second_calls == 3
    gpu.close()


def test_a_single_shard(ctx):
    from inverted_index_2_amd.host import Shard
    rng = np.random.default_rng(78)
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
