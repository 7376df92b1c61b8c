"""Dictionaries aimed at the seams of the term alignment (ii2_align_terms / ii2_align_dicts, csrc/align.hip: k_align_rank), one
table for the CPU test of the claims and the GPU test of the kernel.

The ranking kernel gives every workgroup a stretch of one dictionary's terms, finds the bracket of every other dictionary that
the stretch can meet, and bisects there: in LDS when the bracket fits the staging buffer, in global memory when it does not, not
at all when it is empty.  Ties of the 8-byte keys are decided by the lengths alone when no term of any dictionary is longer than
8 bytes (the short-terms shortcut) and by the bytes otherwise.  A wrong tie-break or a wrong bracket edge shows only where
distinct terms share a key, where a bracket sits at the staging limit, where a workgroup holds one term, where a dictionary is
empty, and where all 64 dictionaries hold the same term.  Every case is (name, dictionaries, claims): `dictionaries` are k
sorted, duplicate-free lists of bytes; `claims` names the regime the case is there for - tests/test_align_cases_cpu.py checks
each claim against ii2_align_plan (the library's own account of the brackets) and against plain Python counts.

The table is built from the plan's own constants, build(terms_per_workgroup, staged_cap): no size of the kernel is written here.

The expectation is computed here from Python's own order of bytes (= bytes.Compare), never from the library:
  union       sorted(set(all terms))
  src[s][u]   the index of union term u in dictionary s, or -1

Claims (all optional):
  long_terms         the plan's long_terms
  all_staged         no bracket in global memory, at least one in LDS
  staged / global    exact counts of brackets in LDS / in global memory
  global_min, empty_min    at least so many brackets in global memory / empty
  max_bracket        the largest bracket, exactly
  workgroups         the plan's n_workgroups, exactly
  wgs_per_dict_min   every dictionary has at least so many workgroups
  one_term_workgroup some dictionary's last workgroup holds exactly one term
  shared_keys_min    at least so many 8-byte keys are shared by distinct terms of the case
  shared_terms_min   at least so many terms are present in more than one dictionary
  short_dict         that dictionary alone has no term longer than 8 bytes
  far_and_near       (sparse, dense): consecutive terms of the sparse dictionary lie more than 8 entries of the dense one apart
                     twice in a row somewhere, and at most 8 apart twice in a row somewhere (of two adjacent pairs of
                     consecutive terms at least one belongs to one thread: both the bisect-again and the walk branch run)
  union              the size of the union
  ties               the case is a tie case: its order is also checked against the oracle's compare_terms
"""
import bisect
import functools
import itertools
import json
import os
import random
from typing import Dict, List, NamedTuple

import numpy as np

MAX_LISTS = 64                 # II2_MAX_LISTS (include/ii2.h)


class Case(NamedTuple):
    name: str
    dicts: List[List[bytes]]
    claims: Dict[str, object]


def key_of(t):
    """the 8-byte key of a term: its first 8 bytes, zero padded"""
    return t[:8].ljust(8, b"\0")


def expected(dicts):
    """(union, src): src int64 [k][n_union]"""
    union = sorted(set(t for d in dicts for t in d))
    pos = {t: u for u, t in enumerate(union)}
    src = np.full((len(dicts), len(union)), -1, np.int64)
    for s, d in enumerate(dicts):
        if d:
            src[s, [pos[t] for t in d]] = np.arange(len(d))
    return union, src


def flat(dicts):
    """(bytes, term_off, seg_first) as ii2_align_terms / ii2_align_plan take them, the bytes padded by one"""
    terms = [t for d in dicts for t in d]
    off = np.zeros(len(terms) + 1, np.uint64)
    if terms:
        off[1:] = np.cumsum([len(t) for t in terms])
    first = np.zeros(len(dicts) + 1, np.uint64)
    first[1:] = np.cumsum([len(d) for d in dicts])
    return np.frombuffer(b"".join(terms) + b"\0", np.uint8), off, first


def shared_keys(dicts):
    """number of 8-byte keys that distinct terms of the case share"""
    keys = {}
    for t in set(t for d in dicts for t in d):
        keys[key_of(t)] = keys.get(key_of(t), 0) + 1
    return sum(1 for n in keys.values() if n > 1)


def shared_terms(dicts):
    """number of terms present in more than one dictionary"""
    seen = {}
    for d in dicts:
        for t in d:
            seen[t] = seen.get(t, 0) + 1
    return sum(1 for n in seen.values() if n > 1)


def gaps(sparse, dense, upper):
    """for consecutive terms of `sparse`: how many entries of `dense` lie between their bounds (upper: the dense dictionary comes
    first, the bound counts the terms <= x; else the terms < x)"""
    bound = bisect.bisect_right if upper else bisect.bisect_left
    at = [bound(dense, t) for t in sparse]
    return [b - a for a, b in zip(at, at[1:])]


def _strings(alphabet, maxlen):
    out = []
    for n in range(maxlen + 1):
        out.extend(bytes(p) for p in itertools.product(alphabet, repeat=n))
    return sorted(out)


# all 9,841 strings of length 0 .. 8 over {\0, a, b}: many distinct terms differ only in trailing zeros, so they share a key
SHORT = _strings(b"\0ab", 8)
# the 8-byte prefix "tiebreak" + all 8,191 strings of length 0 .. 12 over {\0, a}: every key ties, the bytes decide everything
LONG = [b"tiebreak" + t for t in _strings(b"\0a", 12)]


def _sample(rng, pool, n):
    return sorted(rng.sample(pool, n))


def _sparse_around(rng, dense, pool):
    """4 - 5 terms: the dense dictionary's first and last, one it holds whose successor shares its key, one it lacks that shares
    a key with one it holds, one more it holds"""
    held = set(dense)
    tied = [t for t, nxt in zip(dense, dense[1:]) if key_of(t) == key_of(nxt)]
    lacks = [t for t in pool if t not in held and dense[0] < t < dense[-1] and
             any(key_of(n) == key_of(t) for n in dense[max(bisect.bisect_left(dense, t) - 1, 0):bisect.bisect_left(dense, t) + 1])]
    return sorted({dense[0], dense[-1], rng.choice(tied), rng.choice(lacks), rng.choice(dense[1:-1])})


def _ref_kat_dicts():
    """the reference's own test terms: every Put of a recorded test script is one dictionary (tests/golden/ref_kats.json)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_kats.json")
    with open(path) as f:
        scripts = json.load(f)["scripts"]
    out = []
    for name in ("TestIngestion", "TestPut", "TestReadScoped", "TestSearchByPrefix"):
        puts = [sorted(set(t.encode() for t in c[1])) for c in scripts[name]["script"] if c[0] == "put"]
        assert 2 <= len(puts) <= MAX_LISTS
        out.append((name, puts))
    return out


def build(terms_per_workgroup, staged_cap):
    T, CAP = int(terms_per_workgroup), int(staged_cap)
    rng = random.Random(20)
    cases = []

    def case(name, dicts, **claims):
        dicts = [list(d) for d in dicts]
        claims.setdefault("union", len(set(t for d in dicts for t in d)))
        cases.append(Case(name, dicts, claims))

    # ---- the short-terms shortcut: no term longer than 8 bytes, ties of the keys decided by the lengths ----
    tie_pool = [t for t in SHORT if len(t) < 8 or t.endswith(b"\0")]        # terms whose key another term shares
    rest = [t for t in SHORT if not (len(t) < 8 or t.endswith(b"\0"))]
    case("short-ties-staged", [sorted(rng.sample(tie_pool, 450) + rng.sample(rest, 150)) for _ in range(3)],
         long_terms=0, all_staged=True, shared_keys_min=50, shared_terms_min=50, ties=True)
    dense = _sample(rng, SHORT, CAP + CAP // 2)
    sparse = _sparse_around(rng, dense, SHORT)
    case("short-ties-global-sparse-first", [sparse, dense], long_terms=0, global_min=1, shared_keys_min=50, ties=True)
    case("short-ties-global-sparse-last", [dense, sparse], long_terms=0, global_min=1, shared_keys_min=50, ties=True)

    # ---- long terms: every key ties, the bytes decide ----
    dense = _sample(rng, LONG, CAP + CAP // 2)
    case("long-ties-global", [_sparse_around(rng, dense, LONG), dense, _sparse_around(rng, dense, LONG)],
         long_terms=1, global_min=2, ties=True)
    case("long-ties-staged-multi-wg", [_sample(rng, LONG, 2 * T + 450 + 7 * s) for s in range(3)],
         long_terms=1, all_staged=True, wgs_per_dict_min=3, shared_terms_min=50, ties=True)
    short_only = sorted(set(rng.sample(SHORT, 120)) | {b"", b"t", b"tiebre", b"tiebrea", b"tiebrea\0", b"tiebreaj", b"tiebreak", b"tiebreal",
                                                        b"tiebreb", b"u"})
    # (every term of LONG lies between "tiebrea" and "tiebreal" of the short dictionary, which holds "tiebreak" = LONG[0] itself)
    case("mixed-lengths", [short_only, sorted(set(rng.sample(LONG, 300)) | {LONG[0], LONG[1]})],
         long_terms=1, short_dict=0, staged=2, shared_terms_min=1, ties=True)

    # ---- a bracket at the staging limit and one entry over it ----
    for name, n in (("bracket-at-cap", CAP), ("bracket-over-cap", CAP + 1)):
        run = SHORT[1000:1000 + n]
        glob = 0 if n <= CAP else 1
        case(name, [run, [run[0], run[-1]]], long_terms=0, max_bracket=n, ties=True, **{"global": glob})

    # ---- dictionaries of T - 1, T and T + 1 terms: the last workgroup is nearly full, full, or holds one term ----
    for name, n in (("wg-edge-T-1", T - 1), ("wg-edge-T", T), ("wg-edge-T+1", T + 1)):
        claims = dict(long_terms=0, all_staged=True, workgroups=2 * ((n + T - 1) // T))
        if n % T == 1:
            claims["one_term_workgroup"] = True
        case(name, [SHORT[2000:2000 + n], SHORT[2000 + n // 2:2000 + n // 2 + n]], **claims)

    # ---- a sparse dictionary against a dense one: a thread's consecutive terms lie far apart and close together ----
    near = _sample(rng, SHORT, 200)
    far = _sample(rng, SHORT, CAP - 48)
    case("far-and-near", [near, far], long_terms=0, all_staged=True, far_and_near=(0, 1))

    # ---- disjoint dictionaries and empty ones, first, in the middle and last: equal first workgroups, empty brackets ----
    case("disjoint-and-empty", [[], _sample(rng, SHORT, 300), [], _sample(rng, LONG, 300), []], long_terms=1, staged=0, empty_min=1)
    case("disjoint-and-empty-short", [[], SHORT[:300], [], SHORT[5000:5300], []], long_terms=0, staged=0, empty_min=1)

    # ---- k = II2_MAX_LISTS ----
    case("k64-one-term", [[b"x"]] * MAX_LISTS, union=1, k=MAX_LISTS, long_terms=0)
    same = _sample(rng, LONG, T + 76)
    case("k64-identical", [same] * MAX_LISTS, union=len(same), k=MAX_LISTS, long_terms=1, all_staged=True, ties=True)
    pool = _sample(rng, tie_pool, 900)
    sizes = [0, 1, 2, 33, 640, 0, 33, 2, 0, 640, 1, 33] + [rng.choice((0, 1, 2, 33, 640)) for _ in range(MAX_LISTS - 12)]
    case("k64-unequal", [_sample(rng, pool, n) for n in sizes], k=MAX_LISTS, long_terms=0, all_staged=True, empty_min=1, shared_terms_min=50)

    # ---- the reference's own test terms ----
    for name, dicts in _ref_kat_dicts():
        case("ref-" + name, dicts)
    return cases


# the names, known without the library (the tests are parametrised by them; the table itself needs the plan's constants)
NAMES = ["short-ties-staged", "short-ties-global-sparse-first", "short-ties-global-sparse-last", "long-ties-global", "long-ties-staged-multi-wg",
         "mixed-lengths", "bracket-at-cap", "bracket-over-cap", "wg-edge-T-1", "wg-edge-T", "wg-edge-T+1", "far-and-near", "disjoint-and-empty",
         "disjoint-and-empty-short", "k64-one-term", "k64-identical", "k64-unequal"] + ["ref-" + name for name, _ in _ref_kat_dicts()]


@functools.lru_cache(maxsize=None)
def table():
    """{name: Case}, built from the constants that ii2_align_plan itself reports"""
    from inverted_index_2_amd import _lib, engine
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    plan = engine.align_plan([[b"a"], [b"b"]])
    cases = build(plan.terms_per_workgroup, plan.staged_cap)
    assert [c.name for c in cases] == NAMES
    return {c.name: c for c in cases}


# the GPU test's aligned-view cases
VIEW_CASES = ("short-ties-global-sparse-first", "long-ties-staged-multi-wg", "disjoint-and-empty", "k64-unequal")
