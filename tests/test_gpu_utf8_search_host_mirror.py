"""GPU: the host mirror's FuzzySearch, FuzzyTerms and MatchSearch (host/host_index.cpp) with II2_MATCH_UTF8 - over a small index
spread over several shards and segments, partly merged, against plain Python over the same documents (tests/utf8_cases.py): edits
and the prefix count symbols, a query term shorter than the prefix IN SYMBOLS is compared as a whole, FuzzyTerms ranks by the
symbol distance, and the glob's `?` takes a symbol."""
import numpy as np
import pytest

from tests import utf8_cases
from tests.gpu_util import ctx  # noqa: F401
from tests.utf8_cases import GLOB, NOCASE, TRANSPOSE, UTF8

pytestmark = pytest.mark.gpu

WORDS = ("café", "cafe", "cafés", "caffè", "thé", "the", "naïve", "naive", "naïf", "日本語", "日本话", "日本", "éa", "èa", "éà", "àé", "über", "uber", "Über", "señor", "senor")


def _vocab():
    # first bytes across the byte range: several shards (the shard key is the first two bytes >> 6)
    return sorted({w.encode("utf-8") for w in WORDS} | {p + w.encode("utf-8") for p in (b"A_", b"q_") for w in WORDS[:12]})


def _docs(rng, vocab, n):
    return [(sorted({vocab[int(i)] for i in rng.integers(0, len(vocab), int(rng.integers(1, 6)))}), doc) for doc in range(1, n + 1)]


def _want(docs, term, d, prefix, flags):
    pre = min(prefix, utf8_cases.positions(term, flags))     # a query term shorter than the prefix, in symbols under the flag, is compared as a whole
    hit = sorted({t for terms, _ in docs for t in terms if utf8_cases.matches(term, t, d, pre, flags)})
    ids = sorted({doc for terms, doc in docs for t in terms if utf8_cases.matches(term, t, d, pre, flags)})
    ranked = sorted(((t, utf8_cases.distance(term, t, flags)) for t in hit), key=lambda td: (td[1], td[0]))
    return ids, ranked


QUERIES = [w.encode("utf-8") for w in ("café", "日本語", "éà", "éa", "é", "q_café", "Über", "señor", "zzzz", "")]
SETTINGS = [(1, 0, UTF8), (1, 0, 0), (2, 0, UTF8), (1, 1, UTF8), (1, 2, UTF8), (1, 2, 0), (1, 3, UTF8 | TRANSPOSE), (1, 0, UTF8 | NOCASE)]


def _check_all(target, docs, stage):
    for d, prefix, flags in SETTINGS:
        got = target.fuzzy_search(QUERIES, d, prefix, flags)
        for q in QUERIES:
            ids, ranked = _want(docs, q, d, prefix, flags)
            assert got.get(q, []) == ids, (stage, q, d, prefix, flags)
            assert target.fuzzy_terms(q, d, prefix, flags) == ranked, (stage, q, d, prefix, flags)
    for kind, pats in ((GLOB | UTF8, [b"caf?", b"??", "日本?".encode(), b"*\xc3\xa9*", b"?ber"]), (GLOB, [b"caf?", b"??"]), (GLOB | UTF8 | NOCASE, [b"?BER"]),
                       (UTF8, ["é".encode()])):
        got = target.match_search(pats, kind)
        for p in pats:
            m = utf8_cases.matcher(kind, p)
            assert got.get(p, []) == sorted({doc for terms, doc in docs for t in terms if m(t)}), (stage, p, kind)


def test_search_by_symbols(ctx):
    from inverted_index_2_amd.host import HostError, InvertedIndex
    rng = np.random.default_rng(83)
    vocab = _vocab()
    docs = _docs(rng, vocab, 160)
    gpu = InvertedIndex(ctx)
    for terms, doc in docs[:100]:
        gpu.put(terms, doc)
    assert gpu.lib.ii2h_shard_count(gpu.h) >= 3
    _check_all(gpu, docs[:100], "unmerged")
    gpu.merge(2, 30)
    for terms, doc in docs[100:]:
        gpu.put(terms, doc)
    _check_all(gpu, docs, "partly merged")
    e = lambda s: s.encode("utf-8")
    # the flag decides: `cafe` is one symbol from café, two bytes
    assert e("cafe") in dict(gpu.fuzzy_terms(e("café"), 1, 0, UTF8)) and e("cafe") not in dict(gpu.fuzzy_terms(e("café"), 1, 0, 0))
    assert dict(gpu.fuzzy_terms(e("日本語"), 1, 0, UTF8))[e("日本话")] == 1 and dict(gpu.fuzzy_terms(e("日本語"), 2, 0, 0))[e("日本话")] == 2      # distances in symbols
    # the clamp: é is ONE symbol and two bytes - prefix 2 is clamped to the one symbol with the flag (so èa fails, éa passes) ...
    assert _want(docs, e("é"), 1, 2, UTF8)[1] == gpu.fuzzy_terms(e("é"), 1, 2, UTF8) and e("éa") in dict(gpu.fuzzy_terms(e("é"), 1, 2, UTF8))
    assert e("èa") not in dict(gpu.fuzzy_terms(e("é"), 2, 2, UTF8))
    # ... and an unclamped prefix of 2 symbols would be an error for the one-symbol pattern: the search must not raise
    assert gpu.fuzzy_search([e("é"), e("日本")], 1, 3, UTF8).keys() <= {e("é"), e("日本")}
    with pytest.raises(HostError):
        gpu.fuzzy_search([b"\xff"], 1, 0, UTF8)                  # an ill-formed query term with the flag
    assert isinstance(gpu.fuzzy_search([b"\xff"], 1, 0, 0), dict)
    with pytest.raises(HostError):
        gpu.match_search([b"\xc3"], GLOB | UTF8)
    with pytest.raises(HostError):
        gpu.regex_search([b"a"], UTF8)
    gpu.close()
