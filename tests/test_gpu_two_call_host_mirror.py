"""GPU: the host mirror's two-call output protocol (host/host_index.cpp: two_call) - a call whose result does not fit its first
buffer is made a second time with the size the first one reported.  With the default first buffer of 2^22 ids no test workload gets
there, so set_first_cap(1) shrinks it: every form that goes through two_call - prefix_search, intersect, intersect_except,
intersect_at_least, intersect_batch, intersect_top_batch and term_counts' filter - must give the same result as at the default,
the model's (oracle/ref_model.py and Python sets), with exactly one second call; the single ranked forms allocate exactly 2k and
never retry.  One further case pins that a single query and a batch of one lay their groups out alike (Plan::add), on the host
lookup and on the device lookup.  An index of 300 Puts over several shards, unmerged and then partly merged."""
import numpy as np
import pytest

from oracle import ref_model
from tests.gpu_util import ctx  # noqa: F401

pytestmark = pytest.mark.gpu

ABSENT = [b"zz-none", b"a~none", b"q"]
DEFAULT_CAP = 1 << 22


def _vocab(rng, n=60):
    # few terms, so that every one has many postings; second bytes from three shard ranges (shard key = first two bytes >> 6)
    tail = list(b"0123abcd") + [0x41, 0x42, 0xC1, 0xC2]
    out = set()
    while len(out) < n:
        first = int(rng.choice(list(b"abmz")))
        out.add(bytes([first] + [int(rng.choice(tail)) for _ in range(int(rng.integers(2, 5)))]))
    return sorted(out)


def _scores(under, terms, weights, exclude):
    score = {}
    for t, w in zip(terms, weights):
        for v in under.get(t, set()):
            score[v] = score.get(v, 0) + w
    for t in exclude:
        for v in under.get(t, set()):
            score.pop(v, None)
    return score


def _and(under, terms, exclude=()):
    if not terms:
        return []
    return sorted(v for v, s in _scores(under, terms, [1] * len(terms), exclude).items() if s == len(terms))


def _at_least(under, terms, m, exclude=()):
    return sorted(v for v, s in _scores(under, terms, [1] * len(terms), exclude).items() if s >= m)


def _top(under, terms, weights, k, min_score, exclude=()):
    ranked = sorted((-s, v) for v, s in _scores(under, terms, weights, exclude).items() if s >= min_score)
    return [(v, -s) for s, v in ranked[:k]]


def _counts(under, prefix, terms, exclude):
    keep = set(_and(under, terms, exclude))
    out = {t: len(s & keep) for t, s in under.items() if t.startswith(prefix)}
    return {t: c for t, c in out.items() if c}


def _first(candidates, enough):
    """the first candidate query that `enough` accepts: the queries are picked from the model, not from what the index answers"""
    for c in candidates:
        if enough(c):
            return c
    raise AssertionError("no candidate query has a result of 3 ids")


@pytest.fixture(scope="module")
def filled(ctx):  # noqa: F811
    from inverted_index_2_amd.host import InvertedIndex
    rng = np.random.default_rng(2024)
    vocab = _vocab(rng)
    gpu, ref = InvertedIndex(ctx), ref_model.InvertedIndex()
    for _ in range(300):
        terms = [vocab[i] for i in rng.choice(len(vocab), int(rng.integers(4, 16)), replace=False)]
        val = int(rng.integers(0, 100_000))
        gpu.put(list(terms), val)
        ref.put(list(terms), val)
    assert gpu.n_shards >= 4
    yield gpu, ref, vocab
    gpu.close()


def _forms(ref, vocab):
    """one query per form, each with a result of at least 3 ids in the model: (name, call on the index, the model's answer)"""
    under = {t: set(int(v) for v in vals) for t, vals in ref.read()}
    pairs = [(a, b) for i, a in enumerate(vocab) for b in vocab[i + 1:]]
    triples = [(a, b, c) for (a, b) in pairs[::7] for c in vocab[::5] if c not in (a, b)]
    # two prefixes, one a prefix of the other: the run of the shorter one is cut where the longer one's ends (the reference's rule)
    prefixes = _first(([t[:1], t[:2]] for t in vocab), lambda p: all(len(ref.prefix_search(p).get(x, [])) >= 3 for x in p))
    both = _first(pairs, lambda q: len(_and(under, q)) >= 3)
    minus = _first(triples, lambda q: 3 <= len(_and(under, q[:2], q[2:])) < len(_and(under, q[:2])))
    some = _first(triples, lambda q: len(_at_least(under, q, 2, [vocab[0]])) >= 3 and vocab[0] not in q)
    batch = [(list(both), []), (list(minus[:2]), [minus[2]]), ([both[0], ABSENT[0]], []), ([], [vocab[1]]), ([vocab[2]], [ABSENT[1]]),
             ([vocab[3]], [vocab[4]]), ([vocab[5], vocab[6]], []), ([ABSENT[2]], [vocab[3]]), ([vocab[7]], [])]
    tops = [(list(some), [3, 2, 1], 5, 1, []), (list(both), [4, 1], 3, 5, [ABSENT[0]]), ([ABSENT[0], ABSENT[1]], [7, 9], 4, 1, [vocab[1]]),
            ([vocab[2], ABSENT[2]], [2, 200], 6, 1, []), ([vocab[3]], [5], 0, 1, []), ([], [], 3, 1, []), ([vocab[5], vocab[6]], [1, 1], 50, 1, [vocab[7]]),
            (list(minus[:2]), [8, 16], 2, 1, [minus[2]]), ([vocab[8]], [255], 1, 1, [])]
    facet = _first(((both[0][:1], [t], [x]) for t in vocab for x in vocab[::9] if x != t),
                   lambda q: len(_and(under, q[1], q[2])) >= 3 and len(_counts(under, *q)) >= 2)
    forms = [
        ("prefix_search", lambda ix: ix.prefix_search(prefixes), ref.prefix_search(prefixes)),
        ("intersect", lambda ix: ix.intersect(list(both)), _and(under, both)),
        ("intersect_except", lambda ix: ix.intersect_except(list(minus[:2]), [minus[2]]), _and(under, minus[:2], minus[2:])),
        ("intersect_at_least", lambda ix: ix.intersect_at_least(list(some), 2, [vocab[0]]), _at_least(under, some, 2, [vocab[0]])),
        ("intersect_batch", lambda ix: ix.intersect_batch(batch), [_and(under, t, x) for t, x in batch]),
        ("intersect_top_batch", lambda ix: ix.intersect_top_batch(tops), [_top(under, t, w, k, m, x) for t, w, k, m, x in tops]),
        ("term_counts", lambda ix: ix.term_counts(*facet), _counts(under, *facet)),
    ]
    assert len(batch) >= 8 and len(tops) >= 8
    assert sum(len(r) for r in forms[4][2]) >= 3 and sum(len(r) for r in forms[5][2]) >= 3
    ranked = [
        ("intersect_top", lambda ix: ix.intersect_top(list(some), 4, 2, [vocab[0]]), _top(under, some, [1, 1, 1], 4, 2, [vocab[0]])),
        ("intersect_top_weighted", lambda ix: ix.intersect_top_weighted(list(some), [3, 2, 1], 5, 1, []), _top(under, some, [3, 2, 1], 5, 1)),
    ]
    assert all(len(want) >= 3 for _, _, want in ranked)
    return forms, ranked


def test_second_call_gives_the_same_result(filled):
    gpu, ref, vocab = filled
    for stage in ("unmerged", "merged"):
        forms, ranked = _forms(ref, vocab)
        for name, call, want in forms:
            before = gpu.second_calls
            at_default = call(gpu)
            assert gpu.second_calls == before, (stage, name)             # the default first buffer is never too small here
            gpu.set_first_cap(1)
            at_one = call(gpu)
            gpu.set_first_cap(DEFAULT_CAP)
            assert gpu.second_calls == before + 1, (stage, name)         # exactly one second call, in the one place
            assert at_default == at_one == want, (stage, name)
        for name, call, want in ranked:                                  # exactly 2k entries allocated: nothing to retry
            before = gpu.second_calls
            at_default = call(gpu)
            gpu.set_first_cap(1)
            at_one = call(gpu)
            gpu.set_first_cap(DEFAULT_CAP)
            assert gpu.second_calls == before, (stage, name)
            assert at_default == at_one == want, (stage, name)
        if stage == "unmerged":
            assert gpu.merge(2, 8, 2) == ref.merge(2, 8, 2)             # partly merged: merged and Put segments side by side


def test_first_cap_range(filled):
    gpu = filled[0]
    for bad in (0, 2**22 + 1):
        with pytest.raises(Exception, match="set first cap"):
            gpu.set_first_cap(bad)
    gpu.set_first_cap(2**22)
    gpu.set_first_cap(1)
    gpu.set_first_cap(DEFAULT_CAP)


def test_one_query_and_a_batch_of_one_lay_out_alike(filled):
    gpu, ref, vocab = filled
    under = {t: set(int(v) for v in vals) for t, vals in ref.read()}
    a, b = _first(((a, b) for i, a in enumerate(vocab) for b in vocab[i + 1:]), lambda q: len(_and(under, q, [vocab[0]])) >= 3 and vocab[0] not in q)
    for mode in (0, 1):
        gpu.set_resolve(mode)
        # an excluded term found in no segment is dropped, in either form
        t, x = [a, b], [ABSENT[0], vocab[0]]
        assert gpu.intersect_batch([(t, x)])[0] == gpu.intersect_except(t, x) == _and(under, t, x), mode
        q = (t, [3, 5], 4, 1, x)
        assert gpu.intersect_top_batch([q])[0] == gpu.intersect_top_weighted(*q) == _top(under, *q), mode
        # a required term found in no segment: an empty query for the AND forms, an empty group for the ranked ones
        t = [a, ABSENT[1], b]
        assert gpu.intersect_batch([(t, x)])[0] == gpu.intersect_except(t, x) == [], mode
        q = (t, [3, 200, 5], 4, 1, x)
        want = _top(under, *q)
        assert len(want) >= 3 and gpu.intersect_top_batch([q])[0] == gpu.intersect_top_weighted(*q) == want, mode
    gpu.set_resolve(-1)
