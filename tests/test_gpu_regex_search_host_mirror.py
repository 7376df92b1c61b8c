"""GPU: the host mirror's RegexSearch and RegexTerms (host/host_index.cpp) - regular-expression search over every segment of
every shard through ii2_dict_regex and one ii2_query_batch call - against plain Python (`re`) over the same documents: an index of
a few hundred Puts over several shards, unmerged and partly merged; case folding; a pattern that matches nothing and one that
matches every term; more than 8 patterns in one call; a result that needs two_call's second call; a pattern that does not parse;
the order and the limit of RegexTerms; and the same two methods of a single Shard of more than 64 segments."""
import numpy as np
import pytest

from tests.gpu_util import ctx  # noqa: F401
from tests.regex_cases import NOCASE, matches

pytestmark = pytest.mark.gpu

SERVICES = (b"conn", b"db", b"http", b"Auth", b"queue")
EVENTS = (b"timeout", b"timeouts", b"error", b"ERROR", b"error503", b"fail404", b"retry", b"retries", b"req-17-a", b"ok")


def _vocab():
    # first bytes c / d / h / A / q: several shards (the shard key is the first two bytes >> 6)
    return sorted({a + b"_" + b + (b"%d" % i if i else b"") for a in SERVICES for b in EVENTS for i in range(3)} | {b"timeout", b"error", b"retry"})


def _docs(rng, vocab, n):
    return [(sorted({vocab[int(i)] for i in rng.integers(0, len(vocab), int(rng.integers(1, 7)))}), doc) for doc in range(1, n + 1)]


def _want(docs, pattern, flags):
    hit = sorted({t for terms, _ in docs for t in terms if matches(pattern, t, flags)})
    ids = sorted({doc for terms, doc in docs for t in terms if matches(pattern, t, flags)})
    return ids, hit


PATTERNS = [b".*time.*", b"(conn|db)_.*", b".*_(error|fail)[0-9]{3}[0-9]?", b".*_re(try|tries)[12]?", b"z+", b".*", b"[a-z]+_req-[0-9]+-.*", b"auth_.*", b"", b"timeout",
            b"[^_]*_ok", b"(http|queue)_[A-Z]+\\d"]
assert len(PATTERNS) > 8


def _check_all(target, docs, stage):
    for flags in (0, NOCASE):
        got = target.regex_search(PATTERNS, flags)
        for q in PATTERNS:
            ids, hit = _want(docs, q, flags)
            assert got.get(q, []) == ids, (stage, q, flags)
            assert (q in got) == bool(ids), (stage, q, flags)      # a pattern without a match has no entry
            assert target.regex_terms(q, flags) == hit, (stage, q, flags)
            assert target.regex_terms(q, flags, 3) == hit[:3], (stage, q, flags)
    assert target.regex_search([]) == {} and target.regex_terms(b".*", limit=0) == []


def test_regex_search_and_regex_terms(ctx):
    from inverted_index_2_amd.host import HostError, InvertedIndex
    rng = np.random.default_rng(83)
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
    # nothing and everything; the fold decides
    every = sorted({doc for _, doc in docs})
    assert _want(docs, b"z+", 0) == ([], []) and _want(docs, b".*", 0)[0] == every and len(_want(docs, b".*", 0)[1]) == len({t for terms, _ in docs for t in terms})
    assert _want(docs, b"auth_.*", 0)[0] == [] and _want(docs, b"auth_.*", NOCASE)[0]
    # more than 8 patterns in one call: every term of the vocabulary, escaped, is a pattern of its own
    many = sorted(set(vocab))
    assert len(many) > 64
    got = gpu.regex_search([t.replace(b"-", b"\\-") for t in many])
    for t in many:
        assert got.get(t.replace(b"-", b"\\-"), []) == sorted({doc for terms, doc in docs if t in terms}), t
    # a first buffer of four ids: the union goes through two_call's second call and gives the same
    before = gpu.second_calls
    gpu.set_first_cap(4)
    assert gpu.regex_search([b".*"]) == {b".*": every} and gpu.second_calls == before + 1
    gpu.set_first_cap(1 << 22)
    # removed docs are not filtered, as in read
    gpu.put_removed([1, 2, 3])
    assert gpu.regex_search([b".*"])[b".*"] == every
    # a pattern that does not parse fails the whole call, and the index stays usable
    for bad in ([b".*", b"a("], [b"a**"], [b"a{65}"], [b"x" * 257], [b"^a"]):
        with pytest.raises(HostError):
            gpu.regex_search(bad)
    with pytest.raises(HostError):
        gpu.regex_search([b"abc"], 0x01)
    with pytest.raises(HostError):
        gpu.regex_terms(b"[b-a]")
    with pytest.raises(HostError):
        gpu.regex_terms(b"a", 0x40)
    assert gpu.regex_search([b".*"])[b".*"] == every and gpu.regex_terms(b"timeout") == _want(docs, b"timeout", 0)[1]
    gpu.close()


def test_a_single_shard(ctx):
    from inverted_index_2_amd.host import Shard
    rng = np.random.default_rng(84)
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
