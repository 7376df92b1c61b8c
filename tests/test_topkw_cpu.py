"""CPU: ii2_topk_weighted_ranges is wired through every layer - header, export map, binding, Go texts, host mirror, the Python
faces -, its add kernel lives in topk.hip beside the kernels it feeds and waits for no other workgroup, the weighted add and the late
rule are defined once (topk_count.h), and the two host-only exports that run the kernels' own functions agree with plain integer
arithmetic: ii2_topkw_word with per-bit sums, ii2_topkw_plan with a ten-line restatement of the late rule.  The case table of the
GPU test is checked here too: it is what its docstrings say."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import topk_cases as tc
from tests import topkw_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inverted_index_2_amd", "csrc")
OK, EINVAL, ERANGE = 0, -1, -5
FIELDS = ["n_counted", "n_eligible", "n_cut", "total_weight", "max_score", "cut_score", "n_planes", "n_windows", "n_marks", "n_late", "pad"]
WEIGHTS = [1, 2, 3, 4, 7, 8, 85, 127, 128, 170, 255]


def _header():
    return open(os.path.join(ROOT, "include", "ii2.h")).read()


def _header_symbols():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return set(re.findall(r"\b(ii2_[a-z0-9_]+)\s*\(", text))


def _lib_built():
    from inverted_index_2_amd import host
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(host.HOST_LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- wiring ------------------------------------------------------------------------------------------------------------------
def test_topkw_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    exported = re.search(r"global:(.*?);\s*local:", text, flags=re.S).group(1)
    for name, arity in (("ii2_topk_weighted_ranges", 16), ("ii2_topkw_word", 6), ("ii2_topkw_plan", 10)):
        assert name in _header_symbols()
        assert any(fnmatch.fnmatchcase(name, pat.strip()) for pat in exported.split(";") if pat.strip())
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == arity
        assert hasattr(_lib_built(), name)
    go = open(os.path.join(ROOT, "bindings", "go", "ii2.go")).read()
    assert "C.ii2_topk_weighted_ranges(" in go and "func (c *Ctx) TopKWeightedRanges(" in go and "C.ii2_topkw_stats" in go
    assert "func IntersectTopWeighted(" in open(os.path.join(ROOT, "bindings", "go", "index.go")).read()


def test_topkw_stats_layout():
    assert [f[0] for f in _lib.TopkwStats._fields_] == FIELDS
    assert C.sizeof(_lib.TopkwStats) == 56
    body = re.search(r"typedef struct \{([^}]*)\}\s*ii2_topkw_stats;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert [n for decl in re.findall(r"uint(?:32|64)_t ([^;]+);", body) for n in re.split(r",\s*", decl.strip())] == FIELDS
    # ii2_topk_stats keeps its layout
    assert C.sizeof(_lib.TopkStats) == 48


def test_the_option_is_documented_and_set():
    assert re.search(r"^ \*   topk\.late ", _header(), flags=re.M)
    assert '"topk.late"' in open(os.path.join(CSRC, "api.cpp")).read()


def test_the_add_kernel_lives_in_topk_hip_and_the_arithmetic_is_defined_once():
    src = open(os.path.join(CSRC, "topk.hip")).read()
    assert "lookback.h" not in src and "ii2_lookback_launch" not in src
    for k in ("k_top_add", "top_add_weighted<", "launch_top_add("):
        assert k in src, k
    assert "atomic" not in src[src.index("void k_top_add("):src.index("hipError_t launch_top_add(")]
    host = open(os.path.join(CSRC, "setop.cpp")).read()
    assert "launch_top_add(" in host and "launch_thr_add(" in host and "top_add_weighted<" in host and "top_late_set(" in host
    count_h = open(os.path.join(CSRC, "topk_count.h")).read()
    for fn in ("void top_add_weighted(", "uint32_t top_late_set("):
        assert fn in count_h, fn
        for name in os.listdir(CSRC):
            if name != "topk_count.h" and os.path.isfile(os.path.join(CSRC, name)):
                assert fn not in open(os.path.join(CSRC, name), errors="replace").read(), (fn, name)
    # the counting form's kernels are untouched and still not copied
    assert "k_thr_add" not in re.sub(r"//.*", "", src) and "k_top_add" not in open(os.path.join(CSRC, "atleast.hip")).read()


def test_the_path_enum_still_did_not_grow():
    lib = _lib_built()
    names = []
    while (n := lib.ii2_path_name(len(names))) is not None:
        names.append(n.decode())
    assert len(names) == 40 and not any("topk" in n for n in names)


def test_null_context_is_einval():
    lib = _lib_built()
    assert lib.ii2_topk_weighted_ranges(None, 0, None, None, None, 1, 1, None, None, None, None, None, None, None, None, None) == EINVAL


def test_host_library_exports_intersect_top_weighted():
    from inverted_index_2_amd import host
    _lib_built()
    C.CDLL(_lib.LIB_PATH)        # dependency first
    lib = C.CDLL(host.HOST_LIB_PATH)
    assert hasattr(lib, "ii2h_intersect_top_weighted")


def test_python_faces():
    from inverted_index_2_amd import Context, host
    assert callable(getattr(Context, "topk_weighted_ranges", None))
    assert callable(getattr(host.InvertedIndex, "intersect_top_weighted", None))


# ---- the weighted add --------------------------------------------------------------------------------------------------------------
def _word(lib, planes, adds, weights, mask=0xFFFFFFFF):
    arr = (C.c_uint32 * max(len(adds), 1))(*[int(a) for a in adds])
    wts = (C.c_uint32 * max(len(weights), 1))(*[int(w) for w in weights])
    scores = (C.c_uint32 * 32)(*([0x5A5A5A5A] * 32))
    rc = lib.ii2_topkw_word(planes, arr, wts, len(adds), mask, scores)
    return rc, list(scores)


def _sums(adds, weights, mask=0xFFFFFFFF):
    total = np.zeros(32, np.int64)
    for a, w in zip(adds, weights):
        total += ((int(a) >> np.arange(32)) & 1) * int(w)
    return [int(c) if (mask >> i) & 1 else 0 for i, c in enumerate(total)]


def _fitting_run(rng, planes, n):
    """n random (word, weight) adds whose per-bit sums stay below 2^planes: a bit that would pass it is cleared from the word"""
    top = (1 << planes) - 1
    fit = [w for w in WEIGHTS if w <= top]
    adds, weights, total = [], [], np.zeros(32, np.int64)
    for _ in range(n):
        w = int(rng.choice(fit))
        word = int(rng.integers(0, 1 << 32, dtype=np.uint64))
        bits = ((word >> np.arange(32)) & 1).astype(np.int64)
        bits[total + bits * w > top] = 0
        total += bits * w
        adds.append(int(sum(int(b) << i for i, b in enumerate(bits))))
        weights.append(w)
    return adds, weights


@pytest.mark.parametrize("planes", range(1, 9))
def test_word_scores_against_integer_sums(planes):
    lib = _lib_built()
    rng = np.random.default_rng(100 + planes)
    top = (1 << planes) - 1
    for n in (0, 1, 2, 5, 40):
        adds, weights = _fitting_run(rng, planes, n)
        rc, scores = _word(lib, planes, adds, weights)
        assert rc == OK and scores == _sums(adds, weights) and max(scores) <= top, (planes, n)
    # every weight that fits, alone and on top of a counter of 1: the add starts at plane ctz(w) and carries from there
    for w in (w for w in WEIGHTS if w <= top):
        rc, scores = _word(lib, planes, [0xFFFF0000], [w])
        assert rc == OK and scores == [0] * 16 + [w] * 16, (planes, w)
        if w + 1 <= top:
            rc, scores = _word(lib, planes, [0x0F0F0F0F, 0x00FFFF00], [1, w])
            assert rc == OK and scores == _sums([0x0F0F0F0F, 0x00FFFF00], [1, w]), (planes, w)
    # masks: docs outside get 0
    adds, weights = _fitting_run(rng, planes, 12)
    for mask in (0, 1, 0x80000000, 0x0F0F0F0F, int(rng.integers(0, 1 << 32, dtype=np.uint64))):
        rc, scores = _word(lib, planes, adds, weights, mask)
        assert rc == OK and scores == _sums(adds, weights, mask), (planes, hex(mask))
    # an overshooting run saturates to all ones and never wraps - and stays there
    fit = [w for w in WEIGHTS if w <= top]
    over_w = [fit[i % len(fit)] for i in range(2 * top + 4)]
    over = [0xFFFFFFFF if i % 2 == 0 else int(rng.integers(0, 1 << 32, dtype=np.uint64)) | 1 for i in range(len(over_w))]
    for n in range(1, len(over) + 1):
        rc, scores = _word(lib, planes, over[:n], over_w[:n])
        assert rc == OK and scores == [min(s, top) for s in _sums(over[:n], over_w[:n])], (planes, n)
    assert scores == [top] * 32
    # a weight the planes cannot hold saturates too
    if planes < 8:
        rc, scores = _word(lib, planes, [0x0000FFFF], [1 << planes])
        assert rc == OK and scores == [top] * 16 + [0] * 16


@pytest.mark.parametrize("planes", range(1, 9))
def test_all_one_weights_equal_the_unweighted_word(planes):
    lib = _lib_built()
    rng = np.random.default_rng(planes)
    top = (1 << planes) - 1
    adds = [int(x) for x in rng.integers(0, 1 << 32, top + 3, dtype=np.uint64)]           # (the last three saturate)
    for n in sorted({0, 1, top // 2, top, top + 3}):
        arr = (C.c_uint32 * max(n, 1))(*adds[:n])
        plain = (C.c_uint32 * 32)()
        assert lib.ii2_topk_word(planes, arr, n, 0xFFFFFFFF, plain) == OK
        assert _word(lib, planes, adds[:n], [1] * n) == (OK, list(plain)), (planes, n)


def test_word_rejects_bad_arguments():
    lib = _lib_built()
    for planes in (0, 9, 100):
        assert _word(lib, planes, [1], [1]) == (EINVAL, [0x5A5A5A5A] * 32)
    for w in (0, 256, 1 << 31):
        assert _word(lib, 8, [1, 1], [1, w]) == (EINVAL, [0x5A5A5A5A] * 32)
    one = (C.c_uint32 * 1)(1)
    scores = (C.c_uint32 * 32)(*([7] * 32))
    assert lib.ii2_topkw_word(3, one, one, 1, 0xFFFFFFFF, None) == EINVAL
    assert lib.ii2_topkw_word(3, None, one, 1, 0xFFFFFFFF, scores) == EINVAL and list(scores) == [7] * 32
    assert lib.ii2_topkw_word(3, one, None, 1, 0xFFFFFFFF, scores) == EINVAL and list(scores) == [7] * 32
    assert lib.ii2_topkw_word(3, None, None, 0, 0xFFFFFFFF, scores) == OK and list(scores) == [0] * 32


# ---- the plan --------------------------------------------------------------------------------------------------------------------
def _plan(lib, weights, postings, min_score, wlog2=30):
    n = len(weights)
    w = (C.c_uint32 * max(n, 1))(*weights)
    p = (C.c_uint64 * max(n, 1))(*postings)
    late = (C.c_uint8 * max(n, 1))(*([9] * max(n, 1)))
    total, planes, win, n_late = C.c_uint32(77), C.c_uint32(77), C.c_uint64(77), C.c_uint32(77)
    rc = lib.ii2_topkw_plan(n, w, p, min_score, wlog2, C.byref(total), C.byref(planes), C.byref(win), late, C.byref(n_late))
    return rc, (total.value, planes.value, win.value, list(late)[:n], n_late.value)


def _atleast_window(lib, planes, wlog2):
    """ii2_atleast_plan's window at `planes` planes: min_match = 2^(planes - 1) needs exactly that many"""
    m = 1 << (planes - 1)
    b, win, late = C.c_uint32(), C.c_uint64(), C.c_uint64()
    assert lib.ii2_atleast_plan(m, m, wlog2, C.byref(b), C.byref(win), C.byref(late)) == OK and b.value == planes
    return win.value


def test_plan_against_the_late_rule():
    lib = _lib_built()
    rng = np.random.default_rng(11)
    shapes = [([1, 6, 9], [6000, 47, 25]), ([1, 1, 1], [5, 5, 5]), ([2, 1, 2, 1], [10, 10, 10, 10]), ([255], [3]), ([1], [1]),
              ([3, 3, 3, 3], [1, 2, 2, 1]), ([100, 100, 55], [7, 7, 7]), ([128, 64, 32, 16, 8, 4, 2, 1], [128] * 8)]
    for _ in range(30):
        n = int(rng.integers(1, 12))
        shapes.append(([int(x) for x in rng.integers(1, 255 // n + 1, n)], [int(x) for x in rng.integers(1, 6, n) * 100]))      # (ties in postings)
    for weights, postings in shapes:
        total = sum(weights)
        for min_score in sorted({1, 2, max(total // 2, 1), max(total - 1, 1), total, total + 1, total + 100}):
            for wlog2 in (30, 11):
                rc, got = _plan(lib, weights, postings, min_score, wlog2)
                what = (weights, postings, min_score, wlog2)
                if min_score > total:
                    assert (rc, got) == (OK, (0, 0, 0, [0] * len(weights), 0)), what
                    continue
                late = wc.late_rule(weights, postings, min_score)
                planes = total.bit_length()
                assert (rc, got) == (OK, (total, planes, _atleast_window(lib, planes, wlog2), late, sum(late))), what
                if min_score == 1:
                    assert not any(late), what
                assert sum(w for w, f in zip(weights, late) if f) <= min_score - 1 and not all(late), what
    # hand-made: the stop-word shape of the case table, and ties broken by index
    assert _plan(lib, [1, 6, 9], [6000, 47, 25], 2)[1][3:] == ([1, 0, 0], 1)
    assert _plan(lib, [1, 6, 9], [6000, 47, 25], 7)[1][3:] == ([1, 0, 0], 1)
    assert _plan(lib, [1, 6, 9], [6000, 47, 25], 8)[1][3:] == ([1, 1, 0], 2)
    assert _plan(lib, [1, 6, 9], [6000, 47, 25], 16)[1][3:] == ([1, 1, 0], 2)
    assert _plan(lib, [2, 1, 2, 1], [10, 10, 10, 10], 4)[1][3:] == ([1, 1, 0, 0], 2)
    assert _plan(lib, [1, 1, 1], [5, 9, 9], 2)[1][3:] == ([0, 1, 0], 1)
    # no group at all: nothing runs
    assert _plan(lib, [], [], 1) == (OK, (0, 0, 0, [], 0))


def test_plan_rejects_bad_arguments():
    lib = _lib_built()
    untouched = (77, 77, 77, [9, 9], 77)
    assert _plan(lib, [1, 2], [5, 5], 0) == (EINVAL, untouched)
    assert _plan(lib, [1, 0], [5, 5], 1) == (EINVAL, untouched)
    assert _plan(lib, [1, 256], [5, 5], 1) == (ERANGE, untouched)
    assert _plan(lib, [128, 128], [5, 5], 1) == (ERANGE, untouched)
    assert _plan(lib, [128, 127], [5, 5], 1)[0] == OK
    w, p, late = (C.c_uint32 * 2)(1, 2), (C.c_uint64 * 2)(5, 5), (C.c_uint8 * 2)(9, 9)
    a, b, c, d = C.c_uint32(77), C.c_uint32(77), C.c_uint64(77), C.c_uint32(77)
    full = [2, w, p, 1, 30, C.byref(a), C.byref(b), C.byref(c), late, C.byref(d)]
    for i in (1, 2, 5, 6, 7, 8, 9):
        args = list(full)
        args[i] = None
        assert lib.ii2_topkw_plan(*args) == EINVAL, i
    assert (a.value, b.value, c.value, list(late), d.value) == untouched
    assert lib.ii2_topkw_plan(*full) == OK


# ---- the case table --------------------------------------------------------------------------------------------------------------
def test_every_ranked_case_appears_under_every_weight_vector():
    for t in tc.CASES:
        tags = [w.tag for w in wc.CASES if w.case is t.case]
        assert tags[0] == "ones" and set(tags) <= {"ones", "pow2", "odd"}, t.name
        assert len(tags) == 3 or t.case.n_counted > 40, t.name            # (only a case of many groups caps a vector down to all ones)
    for w in wc.CASES:
        assert len(w.weights) == len(w.case.groups) and all(1 <= x <= 255 for x in w.weights), w.name
        assert 1 <= w.total_weight <= 255 and w.min_scores[0] == 1 and w.total_weight in w.min_scores, w.name
        if w.tag == "ones":
            for m in w.min_scores:
                for got, want in zip(wc.reference(w.case, w.weights, 7, m, True), tc.reference(w.case, 7, m, True)):
                    assert np.array_equal(got, want), (w.name, m)
    assert any(x & (x - 1) == 0 and x > 1 for w in wc.CASES if w.tag == "pow2" for x in w.weights)


def test_the_new_cases_are_what_they_say():
    t = wc.BY_NAME["every_score_binary-binary"]
    ids, scores, hist = wc.reference(t.case, t.weights, 1000)
    assert hist[0] == 0 and np.all(hist[1:] == 2) and ids.size == 510
    low = ids < 65536
    assert np.array_equal(scores[low], ids[low]) and ids[~low].min() >= 65536 + 2048 and np.unique(ids[~low] // 2048).size > 1
    t = wc.BY_NAME["full_carry-carry"]
    ids, scores, _ = wc.reference(t.case, t.weights, 100)
    assert dict(zip(ids.tolist(), scores.tolist())) == {3: 255, 70000: 255, 2: 254, 4: 128, 5: 128, 1: 127, 6: 1}
    t = wc.BY_NAME["late_stopwords-stop"]
    assert t.postings[0] == 6000 and max(t.postings[1:]) < 50 and {2, 7} <= set(t.min_scores)
    early = np.unique(np.concatenate(t.case.lists[1:]) // 2048)
    chunks = np.unique(t.case.lists[0] // 2048)
    assert 0 < early.size < chunks.size and np.all(np.isin(early, chunks))      # chunks with an early doc, and chunks with none
    for m in (2, 7):
        assert wc.late_rule(t.weights, t.postings, m) == [1, 0, 0]
    t = wc.BY_NAME["tie_mixed_sets-mixed"]
    ids, scores, hist = wc.reference(t.case, t.weights, 6)
    assert ids.tolist() == [5000, 9, 10, 2999, 3000, 70000] and scores.tolist() == [10, 5, 5, 5, 5, 5] and hist[5] == 5
    assert wc.reference(t.case, t.weights, 3)[0].tolist() == [5000, 9, 10]       # the cut falls between 3 + 2 and 4 + 1
