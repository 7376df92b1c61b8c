"""CPU: the alignment's case table (tests/align_cases.py) without a GPU.  ii2_align_plan counts the brackets of the ranking
kernel (csrc/align.hip: k_align_rank) by the kernel's own constants and bracket function (csrc/align_plan.h) and the shared
comparison (csrc/term_device.h), so every case proves here that it reaches the regime it names; the places of all terms in the
k-way merge, computed from ii2_term_bounds by the formula in align.hip's header, pin the shared comparison on the host before
tests/test_gpu_align_cases.py runs the same table through the kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib, engine
from tests import align_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _lib_or_build():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def plan_of(dicts):
    _lib_or_build()
    return engine.align_plan(dicts)


# ---- wiring ----
def test_header_declares_the_plan():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "ii2.h"), flags=re.S)
    assert re.search(r"\bint\s+ii2_align_plan\s*\(\s*uint32_t\s+k\s*,\s*const\s+uint8_t\s*\*", header)
    assert re.search(r"\}\s*ii2_align_plan_info\s*;", header)
    args = re.search(r"\bii2_align_plan\s*\(([^;]*)\)\s*;", header).group(1)
    assert len(args.split(",")) == len(_lib.PROTOTYPES["ii2_align_plan"][1]) == 5
    # the struct of the binding is the header's, field for field
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*ii2_align_plan_info\s*;", header).group(1)
    fields = [(m.group(1), n.strip()) for m in re.finditer(r"(uint64_t|uint32_t)\s+([^;]*);", body) for n in m.group(2).split(",")]
    ctype = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    assert [(n, ctype[t]) for t, n in fields] == list(_lib.AlignPlan._fields_)
    assert C.sizeof(_lib.AlignPlan) == 64


def test_library_carries_the_symbol_and_the_wrapper_calls_it():
    assert "ii2_*" in _read("inverted_index_2_amd", "csrc", "exports.map")
    lib = _lib_or_build()
    assert hasattr(lib, "ii2_align_plan")
    p = engine.align_plan([[b"a", b"b"], [b"a", b"tiebreakx"]])
    assert (p.n_terms, p.n_workgroups, p.brackets_staged, p.brackets_global, p.brackets_empty, p.max_bracket, p.long_terms) == (4, 2, 2, 0, 0, 2, 1)


def test_kernel_and_plan_share_one_header():
    mk = _read("inverted_index_2_amd", "csrc", "Makefile")
    assert "align_plan.h" in mk
    shared = _read("inverted_index_2_amd", "csrc", "align_plan.h")
    align = _read("inverted_index_2_amd", "csrc", "align.hip")
    assert '#include "align_plan.h"' in align
    for name in ("AL_T", "AL_LCAP", "AL_THREADS"):
        assert re.search(r"constexpr\s+uint32_t\s+%s\s*=" % name, shared), name
        assert not re.search(r"constexpr\s+uint32_t\s+%s\s*=" % name, align), name      # defined once
    assert re.search(r"uint32_t\s+align_bracket\s*\(", shared) and "term_bound(" in shared
    # the kernel and the plan both take their brackets from that function
    kernel = align[align.index("void k_align_rank("):align.index("void k_align_number(")]
    plan = align[align.index("int ii2_align_plan("):align.index("int ii2_align_info(")]
    assert "align_bracket(" in kernel and plan.count("align_bracket(") == 2
    assert "AL_LCAP" in plan and "AL_T" in plan and not re.search(r"\b(1024|2048)\b", plan)


def test_the_table_names_no_size_of_the_kernel():
    text = _read("tests", "align_cases.py")
    assert not re.search(r"\b(1024|2048)\b", text)
    assert re.search(r"def build\(terms_per_workgroup, staged_cap\)", text)


# ---- the table ----
def test_the_pools_are_what_the_table_says():
    assert len(ac.SHORT) == 9841 == len(set(ac.SHORT)) and max(map(len, ac.SHORT)) == 8 and set(b"".join(ac.SHORT)) == set(b"\0ab")
    assert len(ac.LONG) == 8191 == len(set(ac.LONG)) and all(t.startswith(b"tiebreak") for t in ac.LONG) and max(map(len, ac.LONG)) == 20
    assert ac.SHORT == sorted(ac.SHORT) and ac.LONG == sorted(ac.LONG)
    assert len({ac.key_of(t) for t in ac.LONG}) == 1 and ac.shared_keys([ac.SHORT]) > 2000


def test_names_and_shapes():
    table = ac.table()
    assert list(table) == ac.NAMES and len(set(ac.NAMES)) == len(ac.NAMES)
    assert set(ac.VIEW_CASES) <= set(table)
    assert any(n.startswith("ref-") for n in ac.NAMES)                  # the reference's own test terms are there
    for n in ("k64-one-term", "k64-identical", "k64-unequal"):
        assert len(table[n].dicts) == ac.MAX_LISTS == table[n].claims["k"]
    sizes = [len(d) for d in table["k64-unequal"].dicts]
    assert set(sizes) == {0, 1, 2, 33, 640} and sizes.count(0) >= 3
    assert table["k64-one-term"].dicts == [[b"x"]] * ac.MAX_LISTS
    assert all(d == table["k64-identical"].dicts[0] for d in table["k64-identical"].dicts)
    de = table["disjoint-and-empty"].dicts
    assert [bool(d) for d in de] == [False, True, False, True, False] and de[1][-1] < de[3][0]
    for n in ("short-ties-global-sparse-first", "short-ties-global-sparse-last"):
        dense, sparse = sorted(table[n].dicts, key=len, reverse=True)
        assert 4 <= len(sparse) <= 5 and sparse[0] == dense[0] and sparse[-1] == dense[-1]
    assert table["short-ties-global-sparse-first"].dicts == table["short-ties-global-sparse-last"].dicts[::-1]
    a, dense, b = table["long-ties-global"].dicts
    assert 4 <= len(a) <= 5 and 4 <= len(b) <= 5 and {a[0], b[0]} == {dense[0]} and {a[-1], b[-1]} == {dense[-1]}


@pytest.mark.parametrize("name", ac.NAMES)
def test_every_case_is_well_formed(name):
    from oracle import oracle as orc
    case = ac.table()[name]
    assert 1 <= len(case.dicts) <= ac.MAX_LISTS
    for d in case.dicts:
        assert d == sorted(set(d)) and all(isinstance(t, bytes) for t in d)
        if case.claims.get("ties"):                 # Python's order of bytes is the reference's on the very terms that tie
            assert all(orc.compare_terms(a, b) < 0 and orc.compare_terms(b, a) > 0 for a, b in zip(d, d[1:]))
    union, src = ac.expected(case.dicts)
    assert len(union) == case.claims["union"] and src.shape == (len(case.dicts), len(union))
    assert all((src[s] >= 0).sum() == len(d) for s, d in enumerate(case.dicts))
    if case.claims.get("ties"):
        assert all(orc.compare_terms(a, b) < 0 for a, b in zip(union, union[1:]))
        assert orc.compare_terms(union[0], union[0]) == 0


@pytest.mark.parametrize("name", ac.NAMES)
def test_every_claim_holds(name):
    case = ac.table()[name]
    p = plan_of(case.dicts)
    T, cap = p.terms_per_workgroup, p.staged_cap
    print(name, "staged", p.brackets_staged, "global", p.brackets_global, "empty", p.brackets_empty, "max", p.max_bracket, "long_terms", p.long_terms,
          "workgroups", p.n_workgroups, "terms", p.n_terms, "union", case.claims["union"])
    # what holds for every case: the plan counts what plain Python counts
    wgs = [(len(d) + T - 1) // T for d in case.dicts]
    assert p.n_terms == sum(len(d) for d in case.dicts) and p.n_workgroups == sum(wgs)
    assert p.brackets_staged + p.brackets_global + p.brackets_empty == sum(wgs) * (len(case.dicts) - 1)
    assert p.long_terms == int(any(len(t) > 8 for d in case.dicts for t in d))
    assert (p.brackets_global > 0) == (p.max_bracket > cap)
    known = {"long_terms", "all_staged", "staged", "global", "global_min", "empty_min", "max_bracket", "workgroups", "wgs_per_dict_min",
             "one_term_workgroup", "shared_keys_min", "shared_terms_min", "short_dict", "far_and_near", "union", "ties", "k"}
    assert set(case.claims) <= known
    c = case.claims
    if "long_terms" in c:
        assert p.long_terms == c["long_terms"]
    if c.get("all_staged"):
        assert p.brackets_global == 0 and p.brackets_staged > 0 and p.max_bracket <= cap
    if "staged" in c:
        assert p.brackets_staged == c["staged"]
    if "global" in c:
        assert p.brackets_global == c["global"]
    if "global_min" in c:
        assert p.brackets_global >= c["global_min"]
    if "empty_min" in c:
        assert p.brackets_empty >= c["empty_min"]
    if "max_bracket" in c:
        assert p.max_bracket == c["max_bracket"]
    if "workgroups" in c:
        assert p.n_workgroups == c["workgroups"]
    if "wgs_per_dict_min" in c:
        assert min(wgs) >= c["wgs_per_dict_min"]
    if c.get("one_term_workgroup"):
        assert any(len(d) % T == 1 and len(d) > 1 for d in case.dicts)
    if "shared_keys_min" in c:
        assert ac.shared_keys(case.dicts) >= c["shared_keys_min"]
    if "shared_terms_min" in c:
        assert ac.shared_terms(case.dicts) >= c["shared_terms_min"]
    if "short_dict" in c:
        assert all(len(t) <= 8 for t in case.dicts[c["short_dict"]])
    if "k" in c:
        assert len(case.dicts) == c["k"]
    if "far_and_near" in c:
        s, d = c["far_and_near"]
        sparse, dense = case.dicts[s], case.dicts[d]
        assert len(dense) >= 8 * len(sparse)
        g = ac.gaps(sparse, dense, upper=d < s)
        assert any(a > 8 and b > 8 for a, b in zip(g, g[1:])), "no two far gaps in a row"
        assert any(a <= 8 and b <= 8 for a, b in zip(g, g[1:])), "no two near gaps in a row"


def test_the_claims_together_cover_the_regimes():
    table = ac.table()
    plans = {n: plan_of(c.dicts) for n, c in table.items()}
    T, cap = plans["k64-one-term"].terms_per_workgroup, plans["k64-one-term"].staged_cap
    for lt in (0, 1):
        of = [p for p in plans.values() if p.long_terms == lt]
        assert any(p.brackets_staged for p in of) and any(p.brackets_global for p in of) and any(p.brackets_empty for p in of), lt
        claimed = [c.claims for n, c in table.items() if c.claims.get("long_terms") == lt]
        assert any(c.get("all_staged") for c in claimed) and any(c.get("global_min") for c in claimed) and any(c.get("empty_min") for c in claimed), lt
    assert plans["bracket-at-cap"].max_bracket == cap and plans["bracket-at-cap"].brackets_global == 0
    assert plans["bracket-over-cap"].max_bracket == cap + 1 and plans["bracket-over-cap"].brackets_global == 1
    assert [len(table[n].dicts[0]) for n in ("wg-edge-T-1", "wg-edge-T", "wg-edge-T+1")] == [T - 1, T, T + 1]
    assert [plans[n].n_workgroups for n in ("wg-edge-T-1", "wg-edge-T", "wg-edge-T+1")] == [2, 2, 4]
    assert sum(1 for c in table.values() if len(c.dicts) == ac.MAX_LISTS) >= 3


# ---- the plan's errors ----
def test_align_plan_argument_errors():
    lib = _lib_or_build()
    blob = np.frombuffer(b"abtiebreakxc\0", np.uint8)
    off = np.array([0, 1, 2, 11, 12], np.uint64)             # a, b | tiebreakx | c
    first = np.array([0, 2, 3, 4], np.uint64)
    plan = _lib.AlignPlan()
    args = [3, blob.ctypes.data, off.ctypes.data, first.ctypes.data, C.byref(plan)]
    assert lib.ii2_align_plan(*args) == 0 and (plan.n_terms, plan.long_terms, plan.n_workgroups) == (4, 1, 3)

    def bad(i, v, code=-1):
        a = list(args)
        a[i] = v
        marked = _lib.AlignPlan()
        C.memset(C.byref(marked), 0x5A, C.sizeof(marked))
        if i != 4:
            a[4] = C.byref(marked)
        assert lib.ii2_align_plan(*a) == code, (i, v)
        assert bytes(marked) == b"\x5a" * C.sizeof(marked)          # nothing written

    bad(4, None)
    bad(0, 0)
    bad(0, ac.MAX_LISTS + 1)
    bad(2, None)
    bad(3, None)
    bad(1, None)                                             # bytes named by the offsets, none given
    late, down, huge = np.array([1, 2, 3, 4], np.uint64), np.array([0, 3, 2, 4], np.uint64), np.array([0, 2, 3, 1 << 31], np.uint64)
    bad(3, late.ctypes.data)                                 # seg_first does not start at 0
    bad(3, down.ctypes.data)                                 # seg_first descends
    bad(3, huge.ctypes.data, -5)                             # 2^31 terms
    bad(2, np.array([0, 1, 2, 1, 12], np.uint64).ctypes.data)     # term_off descends
    # dictionaries that do not ascend strictly: what ii2_dict_create refuses
    for terms in ([b"a", b"a"], [b"b", b"a"], [b"tiebreakb", b"tiebreaka"], [b"a\0", b"a"]):
        b2, o2, f2 = ac.flat([[b"0"], terms])
        a = [2, b2.ctypes.data, o2.ctypes.data, f2.ctypes.data]
        marked = _lib.AlignPlan()
        C.memset(C.byref(marked), 0x5A, C.sizeof(marked))
        assert lib.ii2_align_plan(*a, C.byref(marked)) == -1 and bytes(marked) == b"\x5a" * C.sizeof(marked), terms
        with pytest.raises(engine.II2Error):
            engine.align_plan([[b"0"], terms])
    # the same terms in two dictionaries are no error, and no terms at all neither (the bytes may then be NULL)
    assert engine.align_plan([[b"a"], [b"a"]]).brackets_staged == 2
    none = np.zeros(1, np.uint64)
    assert lib.ii2_align_plan(1, None, none.ctypes.data, np.zeros(2, np.uint64).ctypes.data, C.byref(plan)) == 0
    assert (plan.n_terms, plan.n_workgroups, plan.brackets_empty, plan.max_bracket) == (0, 0, 0, 0)


# ---- the places of all terms in the k-way merge, from ii2_term_bounds ----
def _bounds(lib, cache, dicts_flat, s, t):
    """(number of terms of dictionary s below t, number of its terms up to and including t), by ii2_term_bounds"""
    blob, off, ident = dicts_flat[s]
    got = cache.get((ident, t))
    if got is None:
        pr = np.frombuffer(t + b"\0", np.uint8)
        first, end = C.c_uint64(), C.c_uint64()
        assert lib.ii2_term_bounds(blob.ctypes.data, off.ctypes.data, off.size - 1, pr.ctypes.data, len(t), 0, C.byref(first), C.byref(end)) == 0
        got = cache[(ident, t)] = (first.value, end.value)
    return got


@pytest.mark.parametrize("name", ac.NAMES)
def test_places_from_term_bounds_are_the_k_way_merge(name):
    """place(term i of dictionary s) = i + sum over s' < s of |{y in s': y <= x}| + sum over s' > s of |{y in s': y < x}|"""
    lib = _lib_or_build()
    case = ac.table()[name]
    idents = {}
    dicts_flat = []
    for d in case.dicts:                     # (equal dictionaries share their answers: the k = 64 cases repeat theirs)
        blob, off, _ = ac.flat([d])
        dicts_flat.append((blob, off, idents.setdefault(tuple(d), len(idents))))
    cache = {}
    k = len(case.dicts)
    n = sum(len(d) for d in case.dicts)
    at = [None] * n
    for s, d in enumerate(case.dicts):
        for i, t in enumerate(d):
            place = i
            for sp in range(k):
                if sp != s and case.dicts[sp]:
                    below, upto = _bounds(lib, cache, dicts_flat, sp, t)
                    place += upto if sp < s else below
            assert 0 <= place < n and at[place] is None, (name, s, i)       # a permutation of 0 .. n - 1
            at[place] = (t, s, i)
    # in place order the terms ascend, equal terms in dictionary order: the run heads number the union
    assert at == sorted(at)
    union, src = ac.expected(case.dicts)
    u = -1
    for place, (t, s, i) in enumerate(at):
        head = place == 0 or at[place - 1][0] != t
        u += head
        assert union[u] == t and src[s, u] == i
    assert u == len(union) - 1
