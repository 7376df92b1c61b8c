"""CPU: ii2_atleast_ranges is wired through every layer - header, export map, binding, Makefile, host mirror, the Python faces - its
kernels keep to the rule that no workgroup waits for another, and the counting form's arithmetic (ii2_atleast_word, ii2_atleast_plan:
host-only exports that run the kernels' own functions) agrees with per-bit integer counting."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

from inverted_index_2_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inverted_index_2_amd", "csrc")
EINVAL, ERANGE = -1, -5
FIELDS = ["n_counted", "bound", "form", "n_planes", "n_windows", "n_late"]


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
def test_atleast_is_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    exported = re.search(r"global:(.*?);\s*local:", text, flags=re.S).group(1)
    for name, arity in (("ii2_atleast_ranges", 13), ("ii2_atleast_plan", 6), ("ii2_atleast_word", 5)):
        assert name in _header_symbols()
        assert any(fnmatch.fnmatchcase(name, pat.strip()) for pat in exported.split(";") if pat.strip())
        res, args = _lib.PROTOTYPES[name]
        assert res is C.c_int and len(args) == arity
    go = open(os.path.join(ROOT, "bindings", "go", "ii2.go")).read()
    assert "C.ii2_atleast_ranges(" in go and "func (c *Ctx) AtLeastRanges(" in go
    assert "IntersectAtLeast(" in open(os.path.join(ROOT, "bindings", "go", "index.go")).read()


def test_atleast_stats_layout():
    assert [f[0] for f in _lib.AtleastStats._fields_] == FIELDS
    assert C.sizeof(_lib.AtleastStats) == 32
    header = open(os.path.join(ROOT, "include", "ii2.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*ii2_atleast_stats;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == FIELDS
    forms = dict(re.findall(r"#define (II2_ATLEAST_\w+) (\d+)u", header))
    assert forms == {"II2_ATLEAST_NONE": "0", "II2_ATLEAST_SMALL": "1", "II2_ATLEAST_COUNT": "2", "II2_ATLEAST_AND": "3", "II2_ATLEAST_OR": "4"}
    assert (_lib.II2_ATLEAST_NONE, _lib.II2_ATLEAST_SMALL, _lib.II2_ATLEAST_COUNT, _lib.II2_ATLEAST_AND, _lib.II2_ATLEAST_OR) == (0, 1, 2, 3, 4)


def test_atleast_object_is_in_the_makefile():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    objs = next(line for line in mk.splitlines() if line.startswith("OBJS"))
    assert "build/atleast.o" in objs.split()
    assert "atleast_count.h" in next(line for line in mk.splitlines() if line.startswith("HDRS")).split()


def test_atleast_kernels_have_no_inter_workgroup_waits_and_share_the_arithmetic():
    src = open(os.path.join(CSRC, "atleast.hip")).read()
    assert "lookback.h" not in src and "ii2_lookback_launch" not in src and "atomic" not in re.sub(r"//.*", "", src)
    for k in ("k_thr_add", "k_thr_select", "thr_add_word", "thr_ge_word", '#include "atleast_count.h"'):
        assert k in src, k
    host = open(os.path.join(CSRC, "setop.cpp")).read()
    assert '#include "atleast_count.h"' in host and "thr_add_word" in host and "thr_ge_word" in host
    # the arithmetic is defined once
    assert "void thr_add_word(" not in src and "void thr_add_word(" not in host


def test_the_path_enum_did_not_grow():
    lib = _lib_built()
    names = []
    while (n := lib.ii2_path_name(len(names))) is not None:
        names.append(n.decode())
    assert len(names) == 40 and not any("atleast" in n or "thr" in n for n in names)


def test_null_context_is_einval():
    lib = _lib_built()
    assert lib.ii2_atleast_ranges(None, 0, None, None, 1, None, None, None, None, None, 0, None, None) == EINVAL


def test_host_library_exports_intersect_at_least():
    from inverted_index_2_amd import host
    _lib_built()
    C.CDLL(_lib.LIB_PATH)        # dependency first
    assert hasattr(C.CDLL(host.HOST_LIB_PATH), "ii2h_intersect_at_least")


def test_python_faces():
    from inverted_index_2_amd import Context, host
    assert callable(getattr(Context, "atleast_ranges", None))
    assert callable(getattr(host.InvertedIndex, "intersect_at_least", None))


# ---- the counter arithmetic ----------------------------------------------------------------------------------------------------
def _word(lib, planes, m, adds):
    arr = (C.c_uint32 * max(len(adds), 1))(*[int(a) for a in adds])
    mask = C.c_uint32(0x5A5A5A5A)
    rc = lib.ii2_atleast_word(planes, m, arr, len(adds), C.byref(mask))
    return rc, mask.value


def _count_mask(adds, m):
    cnt = np.zeros(32, np.int64)
    for a in adds:
        cnt += (int(a) >> np.arange(32)) & 1
    return int(sum(1 << i for i in range(32) if cnt[i] >= m))


def _thresholds(planes):
    lo, hi = 1 << (planes - 1), (1 << planes) - 1
    return list(range(lo, hi + 1)) if planes <= 4 else sorted({lo, lo + 1, (lo + hi) // 2, hi - 1, hi})


@pytest.mark.parametrize("planes", range(1, 9))
def test_word_arithmetic_against_integer_counts(planes):
    lib = _lib_built()
    rng = np.random.default_rng(planes)
    adds = [int(x) for x in rng.integers(0, 1 << 32, 40, dtype=np.uint64)] + [0xFFFFFFFF, 0]
    for m in _thresholds(planes):
        assert m.bit_length() == planes
        for n in (0, 1, 2, 7, len(adds)):
            rc, mask = _word(lib, planes, m, adds[:n])
            assert rc == 0 and mask == _count_mask(adds[:n], m), (planes, m, n)
        # more than 2^B adds of all ones, between random words: the counters saturate and never wrap
        many = adds[:5] + [0xFFFFFFFF] * ((1 << planes) + 3) + adds[5:9]
        for n in range(5 + (1 << planes), len(many) + 1):
            rc, mask = _word(lib, planes, m, many[:n])
            assert rc == 0 and mask == 0xFFFFFFFF == _count_mask(many[:n], m), (planes, m, n)
        # sparse words: every bit position gets its own count
        sparse = [1 << (i % 32) | 1 << ((i * 7) % 32) for i in range(3 * m + 5)]
        rc, mask = _word(lib, planes, m, sparse)
        assert rc == 0 and mask == _count_mask(sparse, m), (planes, m)


def test_word_rejects_bad_arguments():
    lib = _lib_built()
    for planes, m in ((0, 1), (9, 1), (2, 0), (2, 4), (8, 256)):
        rc, mask = _word(lib, planes, m, [1])
        assert rc == EINVAL and mask == 0x5A5A5A5A
    assert lib.ii2_atleast_word(1, 1, None, 0, None) == EINVAL


def _plan(lib, n, m, wlog2):
    planes, win, late = C.c_uint32(77), C.c_uint64(77), C.c_uint64(77)
    rc = lib.ii2_atleast_plan(n, m, wlog2, C.byref(planes), C.byref(win), C.byref(late))
    return rc, planes.value, win.value, late.value


def test_plan():
    lib = _lib_built()
    for n, m in ((3, 1), (3, 2), (3, 3), (8, 4), (40, 20), (260, 255), (300, 255), (255, 255), (1000, 128)):
        for wlog2 in (5, 11, 20, 27, 28, 29, 30, 40):
            rc, planes, win, late = _plan(lib, n, m, wlog2)
            assert rc == 0 and planes == m.bit_length() and late == n - m + 1
            cap = 1 << 30
            while cap * planes > 1 << 30:
                cap >>= 1
            assert win == min(1 << min(max(wlog2, 11), 30), cap)
            assert win & (win - 1) == 0 and planes * win // 8 <= 128 << 20
    assert _plan(lib, 300, 256, 30)[0] == ERANGE                   # the counters hold eight bits
    assert _plan(lib, 1 << 20, 70000, 30)[0] == ERANGE
    assert _plan(lib, 3, 0, 30) == (EINVAL, 77, 77, 77)
    assert _plan(lib, 3, 4, 30) == (0, 0, 0, 0)                    # min_match above n': nothing runs
    assert _plan(lib, 256, 256, 30) == (0, 0, 0, 0)                # min_match = n' > 255: always the AND hand-off
    assert lib.ii2_atleast_plan(3, 1, 30, None, None, None) == EINVAL
