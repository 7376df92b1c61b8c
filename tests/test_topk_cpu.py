"""CPU: ii2_topk_ranges is wired through every layer - header, export map, binding, Makefile, Go texts, host mirror, the Python faces -
its kernels keep to the rule that no workgroup waits for another, the score arithmetic is defined once (topk_count.h), and the two
host-only exports that run the kernels' own functions agree with plain integer arithmetic: ii2_topk_word with per-bit counting,
ii2_topk_cut with numpy."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib
from tests import topk_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inverted_index_2_amd", "csrc")
EINVAL, ERANGE = -1, -5
FIELDS = ["n_counted", "n_eligible", "n_cut", "max_score", "cut_score", "n_planes", "n_windows", "n_marks", "pad"]


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "ii2.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ii2_[a-z0-9_]+)\s*\(", text))


def _lib_built():
    from inverted_index_2_amd import host
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(host.HOST_LIB_PATH)):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- wiring ------------------------------------------------------------------------------------------------------------------
def test_topk_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    exported = re.search(r"global:(.*?);\s*local:", text, flags=re.S).group(1)
    for name, arity in (("ii2_topk_ranges", 15), ("ii2_topk_cut", 6), ("ii2_topk_word", 5)):
        assert name in _header_symbols()
        assert any(fnmatch.fnmatchcase(name, pat.strip()) for pat in exported.split(";") if pat.strip())
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == arity
    go = open(os.path.join(ROOT, "bindings", "go", "ii2.go")).read()
    assert "C.ii2_topk_ranges(" in go and "func (c *Ctx) TopKRanges(" in go
    assert "IntersectTop(" in open(os.path.join(ROOT, "bindings", "go", "index.go")).read()


def test_topk_stats_layout():
    assert [f[0] for f in _lib.TopkStats._fields_] == FIELDS
    assert C.sizeof(_lib.TopkStats) == 48
    header = open(os.path.join(ROOT, "include", "ii2.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*ii2_topk_stats;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == FIELDS
    assert re.search(r"#define II2_TOPK_MAX \(1u << 20\)", header) and _lib.II2_TOPK_MAX == 1 << 20


def test_topk_object_is_in_the_makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "build/topk.o" in next(line for line in mk.splitlines() if line.startswith("OBJS")).split()
    assert "topk_count.h" in next(line for line in mk.splitlines() if line.startswith("HDRS")).split()


def test_topk_kernels_have_no_inter_workgroup_waits_and_share_the_arithmetic():
    src = open(os.path.join(CSRC, "topk.hip")).read()
    assert "lookback.h" not in src and "ii2_lookback_launch" not in src
    for k in ("k_top_hist", "k_top_count", "k_top_emit", "top_score<", "top_eq_word<", "thr_ge_word<", '#include "topk_count.h"'):
        assert k in src, k
    host = open(os.path.join(CSRC, "setop.cpp")).read()
    assert '#include "topk_count.h"' in host and "top_cut(" in host and "top_score<" in host
    # the arithmetic is defined once, and the counters' kernels are reused, not copied
    count_h = open(os.path.join(CSRC, "topk_count.h")).read()
    for fn in ("uint32_t top_score(", "void top_cmp_word(", "uint32_t top_eq_word(", "void top_cut("):
        assert fn in count_h and fn not in src and fn not in host, fn
    assert "k_thr_add" not in re.sub(r"//.*", "", src) and "k_um_mark" not in re.sub(r"//.*", "", src)
    assert "launch_thr_add(" in host and "launch_union_many_mark(" in host


def test_the_path_enum_did_not_grow():
    lib = _lib_built()
    names = []
    while (n := lib.ii2_path_name(len(names))) is not None:
        names.append(n.decode())
    assert len(names) == 40 and not any("topk" in n for n in names)


def test_null_context_is_einval():
    lib = _lib_built()
    assert lib.ii2_topk_ranges(None, 0, None, None, 1, 1, None, None, None, None, None, None, None, None, None) == EINVAL


def test_host_library_exports_intersect_top():
    from inverted_index_2_amd import host
    _lib_built()
    C.CDLL(_lib.LIB_PATH)        # dependency first
    lib = C.CDLL(host.HOST_LIB_PATH)
    assert hasattr(lib, "ii2h_intersect_top") and hasattr(lib, "ii2h_scores_copy")


def test_python_faces():
    from inverted_index_2_amd import Context, host
    assert callable(getattr(Context, "topk_ranges", None))
    assert callable(getattr(host.InvertedIndex, "intersect_top", None))


# ---- the score extraction --------------------------------------------------------------------------------------------------------
def _word(lib, planes, adds, mask=0xFFFFFFFF):
    arr = (C.c_uint32 * max(len(adds), 1))(*[int(a) for a in adds])
    scores = (C.c_uint32 * 32)(*([0x5A5A5A5A] * 32))
    rc = lib.ii2_topk_word(planes, arr, len(adds), mask, scores)
    return rc, list(scores)


def _counts(adds, mask=0xFFFFFFFF):
    cnt = np.zeros(32, np.int64)
    for a in adds:
        cnt += (int(a) >> np.arange(32)) & 1
    return [int(c) if (mask >> i) & 1 else 0 for i, c in enumerate(cnt)]


@pytest.mark.parametrize("planes", range(1, 9))
def test_word_scores_against_integer_counts(planes):
    lib = _lib_built()
    rng = np.random.default_rng(planes)
    top = (1 << planes) - 1
    # random words, as many as the counters hold without saturating
    adds = [int(x) for x in rng.integers(0, 1 << 32, top, dtype=np.uint64)]
    for n in sorted({0, 1, 2, top // 2, top}):
        rc, scores = _word(lib, planes, adds[:n])
        assert rc == 0 and scores == _counts(adds[:n]), (planes, n)
    # every count 0 .. 2^B - 1 at some bit: bit i is set in the first (i * top) // 31 words
    ramp = [sum(1 << i for i in range(32) if j < (i * top) // 31) for j in range(top)]
    rc, scores = _word(lib, planes, ramp)
    assert rc == 0 and scores == _counts(ramp) and max(scores) == top and min(scores) == 0
    # sparse words: every bit position gets its own count
    sparse = [1 << (i % 32) | 1 << ((i * 7) % 32) for i in range(top // 2 + 1)]
    rc, scores = _word(lib, planes, sparse)
    assert rc == 0 and scores == _counts(sparse) and max(scores) <= top
    # masks: docs outside get 0
    for mask in (0, 1, 0x80000000, 0x0F0F0F0F, int(rng.integers(0, 1 << 32, dtype=np.uint64))):
        rc, scores = _word(lib, planes, ramp, mask)
        assert rc == 0 and scores == _counts(ramp, mask), (planes, hex(mask))


def test_word_rejects_bad_arguments():
    lib = _lib_built()
    for planes in (0, 9, 100):
        rc, scores = _word(lib, planes, [1])
        assert rc == EINVAL and scores == [0x5A5A5A5A] * 32
    arr = (C.c_uint32 * 1)(1)
    assert lib.ii2_topk_word(3, arr, 1, 0xFFFFFFFF, None) == EINVAL
    scores = (C.c_uint32 * 32)(*([7] * 32))
    assert lib.ii2_topk_word(3, None, 1, 0xFFFFFFFF, scores) == EINVAL and list(scores) == [7] * 32
    assert lib.ii2_topk_word(3, None, 0, 0xFFFFFFFF, scores) == 0 and list(scores) == [0] * 32


# ---- the cut -----------------------------------------------------------------------------------------------------------------------
def _cut(lib, hist, k):
    h = np.ascontiguousarray(hist, np.uint64)
    mx, c, above, n_cut = C.c_uint32(77), C.c_uint32(77), C.c_uint64(77), C.c_uint64(77)
    rc = lib.ii2_topk_cut(h.ctypes.data_as(_lib.u64p), int(k), C.byref(mx), C.byref(c), C.byref(above), C.byref(n_cut))
    return rc, (mx.value, c.value, above.value, n_cut.value)


def test_cut_against_numpy():
    lib = _lib_built()
    rng = np.random.default_rng(5)
    hists = [np.zeros(256, np.uint64)]
    single = np.zeros(256, np.uint64)
    single[9] = 5
    hists.append(single)
    ends = np.zeros(256, np.uint64)
    ends[0], ends[255] = 3, 2
    hists.append(ends)
    for density in (0.02, 0.3, 1.0):
        h = rng.integers(0, 1000, 256, dtype=np.uint64) * (rng.random(256) < density)
        hists.append(h.astype(np.uint64))
    big = np.zeros(256, np.uint64)
    big[200], big[100] = (1 << 40) + 1, 1 << 41
    hists.append(big)
    for h in hists:
        total = int(h.sum())
        bounds = np.cumsum(h[::-1].astype(object)).tolist()            # k at exact class boundaries, one below, one above
        ks = {0, 1, 2, total, total + 1, total + 1000, max(total - 1, 0)}
        for b in bounds[::17] + bounds[-3:]:
            ks |= {max(int(b) - 1, 0), int(b), int(b) + 1}
        for k in sorted(ks):
            rc, got = _cut(lib, h, k)
            assert rc == 0 and got == tc.cut(h, k), (k, got, tc.cut(h, k))
    # hand-made: 5 docs of score 9
    assert _cut(lib, single, 3) == (0, (9, 9, 0, 3)) and _cut(lib, single, 5) == (0, (9, 9, 0, 5)) and _cut(lib, single, 6) == (0, (9, 9, 0, 5))
    assert _cut(lib, ends, 2) == (0, (255, 255, 0, 2)) and _cut(lib, ends, 3) == (0, (255, 0, 2, 1)) and _cut(lib, ends, 9) == (0, (255, 0, 2, 3))
    assert _cut(lib, single, 0) == (0, (0, 0, 0, 0)) and _cut(lib, hists[0], 4) == (0, (0, 0, 0, 0))


def test_cut_rejects_null_arguments():
    lib = _lib_built()
    h = np.zeros(256, np.uint64)
    a, b, c, d = C.c_uint32(77), C.c_uint32(77), C.c_uint64(77), C.c_uint64(77)
    hp = h.ctypes.data_as(_lib.u64p)
    assert lib.ii2_topk_cut(None, 1, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == EINVAL
    assert lib.ii2_topk_cut(hp, 1, None, C.byref(b), C.byref(c), C.byref(d)) == EINVAL
    assert lib.ii2_topk_cut(hp, 1, C.byref(a), None, C.byref(c), C.byref(d)) == EINVAL
    assert lib.ii2_topk_cut(hp, 1, C.byref(a), C.byref(b), None, C.byref(d)) == EINVAL
    assert lib.ii2_topk_cut(hp, 1, C.byref(a), C.byref(b), C.byref(c), None) == EINVAL
    assert (a.value, b.value, c.value, d.value) == (77, 77, 77, 77)
